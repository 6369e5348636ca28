"""GPU: reproject_kernel and the three remap kernels at the sizes and values the small cases of test_gpu_rigs.py never reach.

Reprojection: rows of more than one block in both modes (four pixels per thread with the LDS transpose, one pixel per thread),
the whole int16 range of disparities, W = 0, 65535 rows, a misaligned disparity tensor -- against exact rational arithmetic on
sampled pixels and a numpy.longdouble evaluation of whole frames (oracle/rig_oracle.py), with the derived bound
    |got - t| <= 0.5 ulp32(t) + |t| * 8 * 2^-53 * (kX + kW).
Remap: destinations large enough for the grid-stride loops to iterate, coordinates on the 1/64-pixel rounding edge, and NaN /
+-inf / out-of-range coordinates (border value 0, as defined in rig_oracle.remap_bilinear) -- byte for byte against the
per-pixel oracle and the numpy host path."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RIGRECT = os.path.join(G, "rig_example2_rigRect.json")

SPECIAL_D = (0, -1, -32768, 32767)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import simplestereo_amd as ss
    return ss, torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------------------ reprojection
def _rig_Q(ss, dest):
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=dest)
    return np.ascontiguousarray(rig.getQ(), dtype=np.float64)


@pytest.fixture(scope="module")
def matrices(env):
    """name -> Q: the example rig at three destination sizes, a dense matrix with no zero entry, and a rig-like one with
    dyadic entries whose W = 8 d - 296 is exactly 0 at disparity 37, X = x - 5 is 0 in column 5 and Y = y - 1 in row 1"""
    ss, _ = env
    rng = np.random.default_rng(77)
    dense = rng.uniform(0.25, 2.0, (4, 4)) * rng.choice([-1.0, 1.0], (4, 4))
    wzero = np.array([[1, 0, 0, -5.0], [0, 1, 0, -1.0], [0, 0, 0, 1000.0], [0, 0, 8.0, -8.0 * 37]])
    assert (dense != 0).all()
    return {"rig1920": _rig_Q(ss, (1920, 1080)), "rig640": _rig_Q(ss, (640, 360)), "rig4096": _rig_Q(ss, (4096, 2160)),
            "dense": dense, "wzero": wzero}


def _disparities(h, w, seed, zero_at=37):
    """the whole int16 range; 0, -1, -32768, 32767 (and the W = 0 disparity) in every position of a quad and in the first and
    last pixel of every row"""
    rng = np.random.default_rng(seed)
    d = rng.integers(-32768, 32768, (h, w)).astype(np.int16)
    vals = SPECIAL_D + (zero_at,)
    for y in range(h):
        for i, v in enumerate(vals):
            for p in range(4):
                x = 8 + 4 * (i * 4 + p) + p + 4 * y
                if x < w - 1:
                    d[y, x] = v
                x2 = w - 9 - (4 * (i * 4 + p) + (3 - p)) - 4 * y          # the same near the end of the row (its last block)
                if x2 > 0:
                    d[y, x2] = v
        d[y, 0] = vals[y % len(vals)]
        d[y, w - 1] = vals[(y + 1) % len(vals)]
        if w > 5:
            d[y, 5] = zero_at                                               # column 5: X = 0 where W = 0 for the `wzero` matrix
    return np.ascontiguousarray(d)


def _reproject(torch, d, Q):
    from simplestereo_amd import _native
    h, w = d.shape
    td = torch.from_numpy(d).cuda()
    out = torch.full((h, w, 3), 12345.0, dtype=torch.float32, device="cuda")          # (a pixel left unwritten must show)
    Qc = np.ascontiguousarray(Q, dtype=np.float64)
    _native.check(_native.lib().ssamd_reproject_device(td.data_ptr(), h, w, Qc.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                       out.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_points(got, d, Q, name, n_exact=250, rows=None):
    """the whole frame against the longdouble evaluation; the forced pixels, both ends of every row, both sides of every block
    boundary and a random sample against exact rational arithmetic"""
    from oracle import rig_oracle
    nbad, first = rig_oracle.reproject_check_longdouble(got, d, Q, rows)
    assert nbad == 0, "%s: %d components outside the bound, first (row, x, component) %s" % (name, nbad, first)
    h, w = d.shape
    rng = np.random.default_rng(h * 7919 + w)
    pix = {(y, x) for y in sorted(set(range(min(h, 8))) | {h - 1}) for x in (0, 1, 2, 3, 5, w - 4, w - 3, w - 2, w - 1) if 0 <= x < w}
    for b in (255, 256, 257, 1023, 1024, 1025, 1027, 1028, 2047, 2048):         # last / first pixel of a block, both modes
        pix |= {(y, b) for y in range(min(h, 2)) if b < w}
    ys, xs = np.nonzero(np.isin(d, SPECIAL_D + (37,)))
    pick = rng.permutation(len(ys))[:n_exact]
    pix |= {(int(ys[i]), int(xs[i])) for i in pick}
    pix |= {(int(rng.integers(0, h)), int(rng.integers(0, w))) for _ in range(n_exact)}
    for y, x in sorted(pix):
        msg = rig_oracle.reproject_check_exact(got[y, x], Q, x, y if rows is None else int(rows[y]), int(d[y, x]))
        assert msg is None, "%s: %s" % (name, msg)


QUAD_WIDTHS = [4, 252, 256, 260, 1020, 1024, 1028, 1920, 4096, 16388]
SCALAR_WIDTHS = [255, 257, 513, 1023, 1921, 4095]


@pytest.mark.parametrize("w", QUAD_WIDTHS + SCALAR_WIDTHS)
def test_reproject_widths_int16_range_every_matrix(env, matrices, w):
    _, torch = env
    h = 1 + w % 3
    d = _disparities(h, w, w)
    for name, Q in matrices.items():
        got = _reproject(torch, d, Q)
        _check_points(got, d, Q, "%s %dx%d" % (name, h, w), n_exact=60)
    # five rows: each of 0, -1, -32768, 32767 and the W = 0 disparity is the first and the last pixel of some row
    d = _disparities(5, w, w + 1)
    assert all(set(d[:, c].tolist()) == set(SPECIAL_D + (37,)) for c in (0, w - 1))
    for name in ("rig640", "wzero"):
        _check_points(_reproject(torch, d, matrices[name]), d, matrices[name], "%s 5x%d" % (name, w), n_exact=60)
    # W = 0: the class exactly -- +inf / -inf by the sign of the numerator, NaN where that is 0 too
    got = _reproject(torch, d, matrices["wzero"])
    z = d == 37
    assert z.any() or w <= 5                                                    # (column 5 of every row holds it)
    assert np.isinf(got[z][:, 2]).all() and (got[z][:, 2] > 0).all()            # Z = 1000 > 0
    ys, xs = np.nonzero(z)
    for y, x in zip(ys.tolist(), xs.tolist()):
        gx, gy = got[y, x, 0], got[y, x, 1]
        assert (np.isnan(gx) if x == 5 else np.isinf(gx) and (gx > 0) == (x > 5)), (y, x, gx)
        assert (np.isnan(gy) if y == 1 else np.isinf(gy) and (gy > 0) == (y > 1)), (y, x, gy)
    if w > 5:
        assert np.isnan(got[0, 5, 0])


@pytest.mark.parametrize("wh,step", [((1920, 1080), 1), ((4096, 2160), 8)], ids=["1920x1080", "4096x2160"])
def test_reproject_full_frames(env, matrices, wh, step):
    """whole frames (2 and 4 blocks per row); with the rig's matrix the longdouble comparison covers every row of 1920 x 1080
    and every 8th row (and the last) of 4096 x 2160, with the W = 0 matrix a quarter of those"""
    _, torch = env
    w, h = wh
    d = _disparities(h, w, 5)
    for name, every in (("rig%d" % w, step), ("wzero", 4 * step)):
        Q = matrices[name]
        got = _reproject(torch, d, Q)
        rows = np.unique(np.concatenate([np.arange(0, h, every), [h - 1]]))
        for lo in range(0, len(rows), 128):
            sel = rows[lo:lo + 128]
            _check_points(got[sel], d[sel], Q, "%s %dx%d rows %d.." % (name, w, h, sel[0]), n_exact=20, rows=sel)


def test_reproject_through_the_rig_equals_the_direct_call(env, matrices):
    ss, torch = env
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=(1920, 1080))
    d = _disparities(3, 1920, 9)
    pts = rig.get3DPoints(torch.from_numpy(d).cuda()).cpu().numpy()
    assert np.array_equal(pts.view(np.uint32), _reproject(torch, d, matrices["rig1920"]).view(np.uint32))


def test_reproject_65535_rows_run_65536_refused(env, matrices):
    """the grid's y dimension: 65535 rows of 4 pixels run; 65536 rows are refused by the host-side check (code -5)"""
    ss, torch = env
    from simplestereo_amd import _native
    d = _disparities(65535, 4, 3)
    got = _reproject(torch, d, matrices["rig640"])
    _check_points(got, d, matrices["rig640"], "65535x4", n_exact=100)
    d2 = np.zeros((65536, 4), np.int16)
    td = torch.from_numpy(d2).cuda()
    out = torch.empty((65536, 4, 3), dtype=torch.float32, device="cuda")
    Q = matrices["rig640"]
    rc = _native.lib().ssamd_reproject_device(td.data_ptr(), 65536, 4, Q.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                              out.data_ptr(), _stream(torch))
    assert rc == -5 and _native.lib().ssamd_last_error().decode() == "more than 65535 rows"
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=(640, 360))
    with pytest.raises(_native.NativeError) as e:
        rig.get3DPoints(td)
    assert e.value.code == -5 and e.value.message == "more than 65535 rows"


def test_reproject_disparity_view_at_an_odd_storage_offset(env, matrices):
    """a contiguous int16 tensor whose storage offset is not a multiple of 8 bytes, with W % 4 == 0: a legitimate tensor"""
    ss, torch = env
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=(640, 360))
    H, W = 5, 1024
    d = _disparities(H, W, 13)
    for off in (1, 2, 3):
        buf = torch.zeros(off + H * W + 8, dtype=torch.int16, device="cuda")
        view = buf[off:off + H * W].view(H, W)
        view.copy_(torch.from_numpy(d).cuda())
        assert view.is_contiguous() and view.data_ptr() % 8 != 0
        pts = rig.get3DPoints(view)
        assert pts.is_cuda and tuple(pts.shape) == (H, W, 3)
        got = pts.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), _reproject(torch, d, matrices["rig640"]).view(np.uint32))
        _check_points(got, d, matrices["rig640"], "offset %d" % off, n_exact=40)


# ------------------------------------------------------------------------------------------------------------------- remap
def _remap_dev(torch, img, mx, my, interp):
    from simplestereo_amd import _native
    hs, ws = img.shape[:2]
    hd, wd = mx.shape
    t, dmx, dmy = torch.from_numpy(img).cuda(), torch.from_numpy(mx).cuda(), torch.from_numpy(my).cuda()
    out = torch.full((hd, wd, 3), 0xA5, dtype=torch.uint8, device="cuda")             # (a pixel left unwritten must show)
    _native.check(_native.lib().ssamd_remap_bgr_device(t.data_ptr(), hs, ws, dmx.data_ptr(), dmy.data_ptr(), hd, wd, interp,
                                                       out.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("wd,hd", [(4096, 2160), (4097, 1025)], ids=["4096x2160", "4097x1025"])
def test_remap_plain_kernel_second_grid_stride_iteration(env, wd, hd):
    """more than 4 194 304 destination pixels (4096 blocks x 256 threads x 4 pixels): the quad loop iterates a second time; pixel
    count = 0 and = 1 mod 4.  Equal to the numpy host path byte for byte, and to the per-pixel oracle on sampled pixels."""
    _, torch = env
    from oracle import rig_oracle
    from simplestereo_amd import _rigs
    assert wd * hd > 4194304 and (wd * hd) % 4 == (0 if wd == 4096 else 1)
    hs, ws = 700, 1000
    rng = np.random.default_rng(wd)
    img = rng.integers(1, 256, (hs, ws, 3)).astype(np.uint8)
    # a smooth warp (neighbouring pixels read neighbouring source pixels) plus noise, reaching outside on every side
    y, x = np.mgrid[0:hd, 0:wd].astype(np.float32)
    mx = (x * np.float32((ws + 6) / wd) - 3 + rng.normal(0, 0.7, (hd, wd)).astype(np.float32)).astype(np.float32)
    my = (y * np.float32((hs + 6) / hd) - 3 + rng.normal(0, 0.7, (hd, wd)).astype(np.float32)).astype(np.float32)
    n = wd * hd
    sample = np.unique(np.concatenate([rng.integers(0, n, 1500), np.arange(4194304 - 8, 4194304 + 1032),
                                       np.arange(0, 8), np.arange(n - 8, n)]))
    smx, smy = mx.reshape(1, -1)[:, sample], my.reshape(1, -1)[:, sample]
    for interp in (1, 0):
        got = _remap_dev(torch, img, mx, my, interp)
        want = _rigs._remap(img, mx, my, interp)
        assert np.array_equal(got, want), (interp, int(np.count_nonzero((got != want).any(-1))))
        ora = rig_oracle.remap_bilinear(img, smx, smy, nearest=(interp == 0))
        assert np.array_equal(got.reshape(-1, 3)[sample], ora[0])


def test_fused_remap_kernels_second_grid_stride_iteration(env):
    """compute(raw1, raw2, rectify=rig) at 1280 x 720: 2 x 720 x 1280 items for 2048 blocks of 256 threads, so the loops of
    remap_lab_records_pair_kernel (ASW) and remap_pack_pair_kernel (GSW) iterate; equal to rectifyImages followed by compute"""
    ss, torch = env
    from simplestereo_amd.synth import make_pair
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=(1280, 720))
    assert 2 * 720 * 1280 > 524288
    w, h = rig.res1
    L, R, _ = make_pair(h, w, 12, 5)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    rect = rig.rectifyImages(tL, tR)
    hostrect = rig.rectifyImages(L, R)
    assert np.array_equal(rect[0].cpu().numpy(), hostrect[0]) and np.array_equal(rect[1].cpu().numpy(), hostrect[1])
    for consistent in (False, True):
        m = ss.passive.StereoASW(winSize=5, maxDisparity=8, consistent=consistent)
        fused = m.compute(tL, tR, rectify=rig)
        assert tuple(fused.shape) == (720, 1280) and torch.equal(fused, m.compute(*rect))
    g = ss.passive.StereoGSW(winSize=5, maxDisparity=8)
    assert torch.equal(g.compute(tL, tR, rectify=rig), g.compute(*rect))


def test_remap_coordinates_on_the_64th_pixel_grid(env):
    """coordinates k / 64: k odd lies exactly between two 1/32 cells and cvRound (half to even) decides, on the negative side
    too (-1/64 -> cell 0, fraction 0; -3/64 -> cell -1, fraction 30/32); in x and in y, from before the first pixel to past the last"""
    _, torch = env
    from oracle import rig_oracle
    from simplestereo_amd import _rigs
    hs, ws = 5, 6
    rng = np.random.default_rng(64)
    img = rng.integers(1, 256, (hs, ws, 3)).astype(np.uint8)
    kx = np.arange(-3 * 64, (ws + 2) * 64 + 1, dtype=np.float32) / np.float32(64)
    ky = np.arange(-3 * 64, (hs + 2) * 64 + 1, dtype=np.float32) / np.float32(64)
    fixed_y = np.array([0.0, -1 / 64, -3 / 64, 0.5, 1 + 33 / 64, hs - 1, hs - 1 + 1 / 64, hs - 1 + 3 / 64, hs - 65 / 64], np.float32)
    fixed_x = np.array([0.0, -1 / 64, -3 / 64, 0.5, 2 + 31 / 64, ws - 1, ws - 1 + 1 / 64, ws - 1 + 3 / 64, ws - 65 / 64], np.float32)
    mx = np.concatenate([np.tile(kx, (len(fixed_y), 1)).ravel(), np.tile(fixed_x[:, None], (1, len(ky))).ravel()])
    my = np.concatenate([np.tile(fixed_y[:, None], (1, len(kx))).ravel(), np.tile(ky, (len(fixed_x), 1)).ravel()])
    mx, my = np.ascontiguousarray(mx[None, :]), np.ascontiguousarray(my[None, :])
    for interp in (1, 0):
        got = _remap_dev(torch, img, mx, my, interp)
        assert np.array_equal(got, rig_oracle.remap_bilinear(img, mx, my, nearest=(interp == 0))), interp
        assert np.array_equal(got, _rigs._remap(img, mx, my, interp)), interp
    # the two named cases, spelled out
    two = _remap_dev(torch, img, np.array([[-1 / 64, -3 / 64]], np.float32), np.zeros((1, 2), np.float32), 1)
    assert np.array_equal(two[0, 0], img[0, 0])                                              # cell 0, fraction 0
    assert np.array_equal(two[0, 1], (30 * 32 * img[0, 0].astype(np.int64) + 512) >> 10)     # cell -1, fraction 30: 30/32 of pixel 0


OUTSIDE = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 2.0 ** 26, -2.0 ** 26]


def _outside_maps(hd, wd, ws, hs, seed):
    """valid random maps with every value of OUTSIDE in mapx alone, in mapy alone and in both (next to in-range values of
    the other coordinate, (0, 0) among them)"""
    rng = np.random.default_rng(seed)
    mx = rng.uniform(0, ws - 1, (hd, wd)).astype(np.float32)
    my = rng.uniform(0, hs - 1, (hd, wd)).astype(np.float32)
    where = []
    pos = rng.permutation(hd * wd)[:6 * len(OUTSIDE)]
    for i, v in enumerate(OUTSIDE):
        for j in range(6):
            p = int(pos[6 * i + j])
            if j % 3 != 1:
                mx.flat[p] = v
            if j % 3 != 0:
                my.flat[p] = v
            if j >= 3:                             # the other coordinate exactly 0: NaN converted to 0 would sample pixel (0, 0)
                if j % 3 == 0:
                    my.flat[p] = 0
                if j % 3 == 1:
                    mx.flat[p] = 0
            where.append(p)
    return mx, my, np.array(sorted(where))


def test_remap_coordinates_outside_every_range_plain_kernel(env):
    """NaN, +-inf, +-1e30, +-2^31, +-2^26 in mapx, mapy or both: the border value 0 in both interpolation modes, as the oracle
    defines it (cvRound gives INT_MIN) and as the numpy host path computes"""
    _, torch = env
    from oracle import rig_oracle
    from simplestereo_amd import _rigs
    hs, ws = 9, 11
    img = np.random.default_rng(1).integers(1, 256, (hs, ws, 3)).astype(np.uint8)             # no zero byte in the source
    mx, my, where = _outside_maps(23, 37, ws, hs, 2)
    for interp in (1, 0):
        got = _remap_dev(torch, img, mx, my, interp)
        with np.errstate(invalid="ignore"):
            host = _rigs._remap(img, mx, my, interp)
        ora = rig_oracle.remap_bilinear(img, mx, my, nearest=(interp == 0))
        assert (ora.reshape(-1, 3)[where] == 0).all() and (ora.reshape(-1, 3) == 0).all(1).sum() == len(where)
        assert np.array_equal(host, ora), interp
        assert np.array_equal(got, ora), (interp, np.argwhere((got != ora).any(-1))[:5].tolist())


def test_remap_coordinates_outside_every_range_fused_kernels(env):
    """the same through compute(raw1, raw2, rectify=rig): a rig whose map arrays are replaced by ones that carry the values.
    The device remap equals the host path (0 at those pixels), and the fused ASW / GSW calls equal remap-then-compute."""
    ss, torch = env
    from simplestereo_amd.synth import make_pair
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=(160, 90))
    w, h = rig.res1
    L, R, _ = make_pair(h, w, 12, 7)
    L, R = np.maximum(L, 1), np.maximum(R, 1)
    L[:3, :3] = 255
    R[:3, :3] = 255                                 # what a NaN converted to 0 would sample
    keep = [rig.mapx1, rig.mapy1, rig.mapx2, rig.mapy2]          # (kept alive: the device-map cache goes by array address)
    ox1, oy1, where1 = _outside_maps(90, 160, w, h, 3)
    ox2, oy2, where2 = _outside_maps(90, 160, w, h, 4)
    m1, m2 = np.zeros(90 * 160, bool), np.zeros(90 * 160, bool)
    m1[where1], m2[where2] = True, True
    m1, m2 = m1.reshape(90, 160), m2.reshape(90, 160)
    rig.mapx1, rig.mapy1 = np.where(m1, ox1, keep[0]).astype(np.float32), np.where(m1, oy1, keep[1]).astype(np.float32)
    rig.mapx2, rig.mapy2 = np.where(m2, ox2, keep[2]).astype(np.float32), np.where(m2, oy2, keep[3]).astype(np.float32)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    for interp in (1, 0):
        with np.errstate(invalid="ignore"):
            h1, h2 = rig.rectifyImages(L, R, interpolation=interp)
        assert (h1[m1] == 0).all() and (h2[m2] == 0).all()
        r1, r2 = rig.rectifyImages(tL, tR, interpolation=interp)
        assert np.array_equal(r1.cpu().numpy(), h1) and np.array_equal(r2.cpu().numpy(), h2)
        a = ss.passive.StereoASW(winSize=5, maxDisparity=10)
        assert torch.equal(a.compute(tL, tR, rectify=rig, interpolation=interp), a.compute(r1, r2))
        # the matchers see the pixels: the map from frames with those pixels at the value of source pixel (0, 0) differs
        w1, w2 = r1.clone(), r2.clone()
        w1[torch.from_numpy(m1).cuda()] = 255
        w2[torch.from_numpy(m2).cuda()] = 255
        assert not torch.equal(a.compute(w1, w2), a.compute(r1, r2))
        g = ss.passive.StereoGSW(winSize=5, maxDisparity=10)
        assert torch.equal(g.compute(tL, tR, rectify=rig, interpolation=interp), g.compute(r1, r2))
        assert not torch.equal(g.compute(w1, w2), g.compute(r1, r2))
