"""GPU tier of ss.active.GrayCode / grayCodeDecode: the three HIP kernels (decode, scan, cloud) against the numpy restatement
tests/_graycode_ref.py.  Every comparison is exact: the decoded pixels by value, the float64 points on their bit patterns (NaN where
the restatement has NaN).  Shapes are the smallest at which a path can go wrong: a block is 1024 consecutive region pixels (256
threads x 4), the scan walks 1024 blocks per round."""
import os

import numpy as np
import pytest

import _graycode_ref as G

pytestmark = pytest.mark.gpu
BLOCK = 1024


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _decode_both(ss, torch, stack, res, want, **kw):
    """grayCodeDecode on the host array and on the device tensor, both against `want`"""
    got = ss.active.grayCodeDecode(stack, res, **kw)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want)
    if "maps" in kw and kw["maps"] is not None:
        kw = dict(kw, maps=tuple(torch.from_numpy(m).cuda() for m in kw["maps"]))
    dev = ss.active.grayCodeDecode(torch.from_numpy(stack).cuda(), res, **kw)
    assert dev.is_cuda and dev.dtype == torch.int32 and np.array_equal(_np(dev), want)
    return got


def _cloud_all_routes(ss, torch, gc, stack, want_dense, decoded, roi=None):
    """getCloud compacted and dense, on the host array and on the device tensor, against the restatement"""
    want = G.compact(want_dense, decoded)
    t = torch.from_numpy(stack).cuda()
    for images in (stack, t):
        pts = gc.getCloud(images, roi=roi)
        assert (pts.is_cuda if images is t else isinstance(pts, np.ndarray))
        assert tuple(pts.shape) == want.shape and G.same_points(_np(pts), want)
        dense = gc.getCloud(images, roi=roi, dense=True)
        assert G.same_points(_np(dense), want_dense)
    return want


# ------------------------------------------------------------------------------------------------ decode without maps
def test_decode_random_stack(ss, torch):
    stack = G.random_stack(21, 14, 37, 67)
    want = G.decode(stack, 13, 6, 5)
    valid = want[..., 0] >= 0
    assert 0.2 < valid.mean() < 0.8
    _decode_both(ss, torch, stack, (13, 6), want)
    extra = np.concatenate([stack, G.random_stack(22, 3, 37, 67)])             # M > N: the extra images are not read
    _decode_both(ss, torch, extra, (13, 6), want)
    got = ss.active.grayCodeDecode(list(stack), (13, 6))                       # a sequence of planes is stacked on the host
    assert np.array_equal(got, want)


@pytest.mark.parametrize("thr", [0, 1, 5, 256])
def test_decode_contrast_at_the_threshold(ss, torch, thr):
    """per bit and pixel a contrast of white_thr - 1 (an error), white_thr (none) or 0 (an error unless white_thr is 0; bit 0)"""
    rng = np.random.default_rng(30 + thr)
    px, py = rng.integers(0, 13, (37, 67)), rng.integers(0, 6, (37, 67))
    choices = np.array([max(thr - 1, 0), min(thr, 255), 0, min(thr, 255), min(thr, 255), min(thr, 255), min(thr, 255), min(thr, 255)])
    contrast = choices[rng.integers(0, len(choices), (7, 37, 67))]
    stack = G.render(px, py, 13, 6, contrast)
    want = G.decode(stack, 13, 6, thr)
    valid = want[..., 0] >= 0
    if thr == 0:
        assert valid.sum() > 0                                                  # nothing is low contrast; codes may leave the projector
    elif thr == 256:
        assert not valid.any()                                                  # no difference of bytes reaches 256
    else:
        assert 0 < valid.sum() < valid.size
    _decode_both(ss, torch, stack, (13, 6), want, white_thr=thr)


def test_codes_beyond_the_projector_are_flagged(ss, torch):
    yy, xx = np.mgrid[0:8, 0:16]                                                # every 4-bit x 3-bit code once
    stack = G.render(xx, yy, 13, 6, 50)
    want = G.decode(stack, 13, 6, 5)
    inside = (xx < 13) & (yy < 6)
    assert np.array_equal(want[..., 0] >= 0, inside) and np.array_equal(want[inside], np.stack([xx, yy], -1)[inside])
    _decode_both(ss, torch, stack, (13, 6), want)


# ------------------------------------------------------------------------------------------------ decode with maps
def test_decode_through_the_undistortion_maps(ss, torch):
    from simplestereo_amd import _rigs
    import _stereo_ftp_ref as S
    r = G.rig((67, 37), (13, 6), "none", dist1=[0.9, 0.3, 0.002, -0.003, 0.02])
    mx, my = S.undistort_maps(np.array(r["intrinsic1"]), r["distCoeffs1"], (67, 37))
    assert mx.min() < -1 and mx.max() > 67 and my.min() < -1 and my.max() > 37      # taps fall outside the image at the border
    stack = G.random_stack(23, 14, 37, 67)
    und = G.remap_stack(stack, mx, my)
    assert np.array_equal(und, np.stack([_rigs._remap(p, mx, my, _rigs.INTER_LINEAR) for p in stack]))
    assert np.array_equal(und, G.remap_stack_taps_once(stack, mx, my))
    want = G.decode(und, 13, 6, 5)
    assert 0 < (want[..., 0] >= 0).sum() < want[..., 0].size
    _decode_both(ss, torch, stack, (13, 6), want, maps=(mx, my))
    _decode_both(ss, torch, stack, (13, 6), G.decode(und, 13, 6, 0), maps=(mx, my), white_thr=0)


def test_decode_with_non_finite_map_entries(ss, torch):
    rng = np.random.default_rng(24)
    mx = rng.uniform(-2, 69, (37, 67)).astype(np.float32)
    my = rng.uniform(-2, 39, (37, 67)).astype(np.float32)
    mx[0, 0], mx[0, 1], mx[0, 2] = np.nan, np.inf, 2.0 ** 27
    my[1, 0], my[1, 1], my[1, 2] = np.nan, -np.inf, -2.0 ** 27
    stack = G.random_stack(25, 14, 37, 67)
    und = G.remap_stack(stack, mx, my)
    assert not und[:, 0, :3].any() and not und[:, 1, :3].any()
    for thr in (0, 5):                                                          # a pixel that samples nothing: (0, 0) with thr 0, an error otherwise
        want = G.decode(und, 13, 6, thr)
        assert (want[0, :3] == (0 if thr == 0 else -1)).all()
        _decode_both(ss, torch, stack, (13, 6), want, maps=(mx, my), white_thr=thr)


# ------------------------------------------------------------------------------------------------ shapes and roi
@pytest.fixture(scope="module")
def wide(ss):
    """a 1030 x 40 camera, a 13 x 6 projector with lens distortion on both: the stack, its maps, the full frame decoded as it is
    and through the maps"""
    import _stereo_ftp_ref as S
    r = G.rig((1030, 40), (13, 6), "d8", dist1=[-0.1, 0.03, 0.001, -0.001, 0.0])
    stack = G.scene(26, (1030, 40), (13, 6), noise=2, holes=0.3)
    mx, my = S.undistort_maps(np.array(r["intrinsic1"]), r["distCoeffs1"], (1030, 40))
    und = G.remap_stack_taps_once(stack, mx, my)
    return {"rig": r, "gc": ss.active.GrayCode(G.make_rig(ss, r)), "stack": stack, "maps": (mx, my), "plain": G.decode(stack, 13, 6, 5),
            "decoded": G.decode(und, 13, 6, 5), "geom": G.geometry(r)}


@pytest.mark.parametrize("w", [1, 63, 64, 65, 129, 257])
def test_region_widths_heights_and_odd_origins(ss, torch, wide, w):
    for h in (1, 2, 5):
        for x0, y0 in ((3, 1), (0, 0), (7, 11)):
            roi = (x0, y0, x0 + w, y0 + h)
            _decode_both(ss, torch, wide["stack"], (13, 6), wide["plain"][y0:y0 + h, x0:x0 + w], roi=roi)
            _decode_both(ss, torch, wide["stack"], (13, 6), wide["decoded"][y0:y0 + h, x0:x0 + w], roi=roi, maps=wide["maps"])


@pytest.mark.parametrize("w,h", [(1023, 1), (341, 3), (32, 32), (1024, 1), (41, 25), (1025, 1), (241, 17)])
def test_region_sizes_around_a_block(ss, torch, wide, w, h):
    """flattened sizes of one block - 1, one block, one block + 1 and four blocks + 1, in one row and in several"""
    assert w * h in (BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK + 1)
    x0, y0 = 5, 3
    roi = (x0, y0, x0 + w, y0 + h)
    dec = wide["decoded"][y0:y0 + h, x0:x0 + w]
    _decode_both(ss, torch, wide["stack"], (13, 6), wide["plain"][y0:y0 + h, x0:x0 + w], roi=roi)
    _decode_both(ss, torch, wide["stack"], (13, 6), dec, roi=roi, maps=wide["maps"])
    assert 0 < (dec[..., 0] >= 0).sum() < w * h
    _cloud_all_routes(ss, torch, wide["gc"], wide["stack"], G.cloud_dense(wide["geom"], dec, x0, y0), dec, roi=roi)


# ------------------------------------------------------------------------------------------------ compaction
@pytest.fixture(scope="module")
def small(ss):
    r = G.rig((67, 37), (13, 6), "d5")
    yy, xx = np.mgrid[0:37, 0:67]
    return {"rig": r, "gc": ss.active.GrayCode(G.make_rig(ss, r)), "px": xx % 13, "py": yy % 6, "geom": G.geometry(r)}


@pytest.mark.parametrize("which", ["all", "none", "last", "first"])
def test_compaction_corner_cases(ss, torch, small, which):
    contrast = np.zeros((7, 37, 67), int)
    if which == "all":
        contrast[:] = 60
    elif which != "none":
        contrast[(slice(None),) + ((-1, -1) if which == "last" else (0, 0))] = 60
    stack = G.render(small["px"], small["py"], 13, 6, contrast)
    dec = G.decode(G.undistort_stack(stack, small["rig"]["intrinsic1"], small["rig"]["distCoeffs1"], (67, 37)), 13, 6, 5)
    n = {"all": 37 * 67, "none": 0, "last": 1, "first": 1}[which]
    assert (dec[..., 0] >= 0).sum() == n
    want = _cloud_all_routes(ss, torch, small["gc"], stack, G.cloud_dense(small["geom"], dec, 0, 0), dec)
    assert want.shape == (n, 1, 3) and np.isfinite(want).all()


def test_compaction_keeps_raster_order_over_many_blocks(ss, torch):
    r = G.rig((310, 305), (64, 32), "d5")
    stack = G.scene(27, (310, 305), (64, 32), noise=2, holes=0.45)
    roi = (5, 2, 305, 303)                                                      # 300 x 301 pixels, 89 blocks
    dec = G.decode(stack, 64, 32, 5)[2:303, 5:305]
    valid = dec[..., 0] >= 0
    assert dec.shape == (301, 300, 2) and 0.3 < valid.mean() < 0.8
    gc = ss.active.GrayCode(G.make_rig(ss, r))
    dense = G.cloud_dense(G.geometry(r), dec, 5, 2)
    want = _cloud_all_routes(ss, torch, gc, stack, dense, dec, roi=roi)
    assert np.array_equal(want, dense[valid].reshape(-1, 1, 3)) and want.shape[0] == valid.sum()


def test_scan_walks_more_than_one_round(ss, torch):
    """1400 x 1500 = 2 100 000 region pixels = 2051 blocks: three rounds of the one-workgroup scan (1024 + 1024 + 3).  A constant
    plane pair of a 2 x 1 projector, contrast washed out at every 7th pixel; the compacted cloud must be dense[valid]."""
    h, w = 1400, 1500
    assert h * w >= 2000001 and (h * w + BLOCK - 1) // BLOCK > 2 * BLOCK
    r = G.rig((w, h), (2, 1), "none")
    valid = (np.arange(h * w) % 7 != 0).reshape(h, w)
    stack = np.stack([np.where(valid, 90, 30), np.full((h, w), 30)]).astype(np.uint8)
    gc = ss.active.GrayCode(G.make_rig(ss, r))
    t = torch.from_numpy(stack).cuda()
    dec = ss.active.grayCodeDecode(t, (2, 1))
    assert bool((dec[..., 1][torch.from_numpy(valid).cuda()] == 0).all()) and bool((dec[..., 0] == torch.from_numpy(np.where(valid, 1, -1)).cuda()).all())
    pts = gc.getCloud(t)
    dense = gc.getCloud(t, dense=True)
    tv = torch.from_numpy(valid).cuda()
    assert tuple(pts.shape) == (int(valid.sum()), 1, 3) and tuple(dense.shape) == (h, w, 3)
    assert bool(torch.isnan(dense[~tv]).all()) and bool(torch.isfinite(dense[tv]).all())
    assert torch.equal(pts.reshape(-1, 3).view(torch.int64), dense[tv].view(torch.int64))
    # a few rows against the restatement, the first and the last block among them
    for y0 in (0, 701, h - 2):
        rows = G.cloud_dense(G.geometry(r), _np(dec[y0:y0 + 2]), 0, y0)
        assert G.same_points(_np(dense[y0:y0 + 2]), rows)


# ------------------------------------------------------------------------------------------------ bit depth
def test_sixteen_bits_per_axis(ss, torch):
    res = (65536, 65536)
    assert G.num_patterns(*res) == 64
    px = np.array([[65535, 65534, 32768, 32767, 0, 1, 43690, 21845, 49152]] * 3)
    py = np.array([[65535] * 9, [32768] * 9, [12345] * 9])
    stack = G.render(px, py, *res, 40)
    want = G.decode(stack, *res, 5)
    assert np.array_equal(want[..., 0], px) and np.array_equal(want[..., 1], py)
    _decode_both(ss, torch, stack, res, want)
    r = G.rig((9, 3), res, "d5")
    _cloud_all_routes(ss, torch, ss.active.GrayCode(G.make_rig(ss, r)), stack, G.cloud_dense(G.geometry(r), want, 0, 0), want)


def test_a_projector_of_one_pixel_has_no_patterns(ss, torch):
    empty = np.empty((0, 3, 9), np.uint8)
    want = np.zeros((3, 9, 2), np.int32)
    assert np.array_equal(G.decode(empty, 1, 1, 5, shape=(3, 9)), want)
    _decode_both(ss, torch, empty, (1, 1), want)
    _decode_both(ss, torch, G.random_stack(1, 2, 3, 9), (1, 1), want)           # extra images are ignored
    r = G.rig((9, 3), (1, 1), "none")
    gc = ss.active.GrayCode(G.make_rig(ss, r))
    assert gc.num_patterns == 0
    want_pts = _cloud_all_routes(ss, torch, gc, empty, G.cloud_dense(G.geometry(r), want, 0, 0), want)
    assert want_pts.shape == (27, 1, 3)


# ------------------------------------------------------------------------------------------------ cloud
@pytest.fixture(scope="module")
def scene_stack():
    return G.scene(28, (67, 37), (1280, 720), noise=2)


@pytest.mark.parametrize("dist", ["none", "d4", "d5", "d8", "d12", None])
def test_cloud_for_every_distortion_model(ss, torch, scene_stack, dist):
    r = G.rig((67, 37), (1280, 720), dist, dist1=[-0.2, 0.08, 0.001, -0.002, 0.01])
    und = G.undistort_stack(scene_stack, r["intrinsic1"], r["distCoeffs1"], r["res1"])
    dec = G.decode(und, 1280, 720, 5)
    assert 0.5 < (dec[..., 0] >= 0).mean() < 1
    dense = G.cloud_dense(G.geometry(r), dec, 0, 0)
    assert np.isfinite(dense[dec[..., 0] >= 0]).all()
    _cloud_all_routes(ss, torch, ss.active.GrayCode(G.make_rig(ss, r)), scene_stack, dense, dec)
    if dist is None:                                                            # no coefficients = none of them
        r0 = dict(r, distCoeffs2=[])
        assert G.same_points(ss.active.GrayCode(G.make_rig(ss, r0)).getCloud(scene_stack, dense=True), dense)


def test_baseline_along_x_and_a_disparity_of_exactly_zero(ss, torch):
    """T[2] == 0 (no finite epipole: ftpGeometry refuses such a rig, Gray code does not need one); camera and projector with the
    same intrinsics and orientation, so that a pixel that sees its own projector coordinates has a disparity of exactly 0"""
    K = [[1024.0, 0, 24.0], [0, 1024.0, 16.0], [0, 0, 1]]
    r = G.rig((48, 32), (64, 32), "none", T=(-200.0, 0.0, 0.0), R=np.eye(3), K1=K, K2=K)
    yy, xx = np.mgrid[0:32, 0:48]
    px = xx + 9
    px[5, 7], px[20, 40] = 7, 40
    stack = G.render(px, yy, 64, 32, 60)
    dec = G.decode(stack, 64, 32, 5)
    assert (dec[..., 0] >= 0).all()
    dense = G.cloud_dense(G.geometry(r), dec, 0, 0)
    assert not np.isfinite(dense[5, 7]).any() and not np.isfinite(dense[20, 40]).any()       # baseline * (pc / 0), rotated: inf and 0 * inf
    assert np.isfinite(np.delete(dense.reshape(-1, 3), [5 * 48 + 7, 20 * 48 + 40], axis=0)).all()
    with pytest.raises(ValueError, match="T\\[2\\] == 0"):
        ss.active.ftpGeometry(G.make_rig(ss, r), 1000.0, 12.0)
    _cloud_all_routes(ss, torch, ss.active.GrayCode(G.make_rig(ss, r)), stack, dense, dec)


# ------------------------------------------------------------------------------------------------ routes
def test_another_stream_and_a_roi(ss, torch, scene_stack):
    r = G.rig((67, 37), (1280, 720), "d5", dist1=[-0.2, 0.08, 0.001, -0.002, 0.01])
    gc = ss.active.GrayCode(G.make_rig(ss, r))
    roi = (3, 5, 60, 36)
    host = gc.getCloud(scene_stack, roi=roi)
    host_dense = gc.getCloud(scene_stack, roi=roi, dense=True)
    assert host_dense.shape == (31, 57, 3) and host.shape[0] == np.isfinite(host_dense[..., 0]).sum()
    assert G.same_points(host, host_dense[~np.isnan(host_dense[..., 0])].reshape(-1, 1, 3))      # dense against compacted
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t = torch.from_numpy(scene_stack).cuda()
        pts = gc.getCloud(t, roi=roi)
        dense = gc.getCloud(t, roi=roi, dense=True)
    stream.synchronize()
    assert G.same_points(_np(pts), host) and G.same_points(_np(dense), host_dense)


def test_paths_of_generated_pngs(ss, torch, tmp_path):
    pytest.importorskip("PIL.Image")
    target = str(tmp_path / "codes")
    n = ss.active.generateGrayCodeImgs(target, (64, 48))
    assert n == 24
    r = G.rig((64, 48), (64, 48), "d5", dist1=[-0.05, 0.01, 0.0, 0.0, 0.0])
    gc = ss.active.GrayCode(G.make_rig(ss, r))
    paths = [os.path.join(target, "%d.png" % i) for i in range(n)] + [os.path.join(target, "white.png")]
    pat = G.pattern(64, 48)
    got = gc.getCloud(paths)
    assert G.same_points(got, gc.getCloud(pat)) and got.shape[0] > 2000
    und = G.undistort_stack(pat, r["intrinsic1"], r["distCoeffs1"], r["res1"])
    dec = G.decode(und, 64, 48, 5)
    assert G.same_points(got, G.compact(G.cloud_dense(G.geometry(r), dec, 0, 0), dec))


def test_a_720p_frame(ss, torch):
    """a user's size: 1280 x 720 camera and projector (N = 42), a rendered scene with noise, compared in full.  The camera has no
    lens distortion here (the remap restatement of 42 such planes takes several seconds): its maps are the pixel grid, exactly, so
    cv2.undistort leaves every plane as it is."""
    r = G.rig((1280, 720), (1280, 720), "d5")
    stack = G.scene(29, (1280, 720), (1280, 720), noise=3)
    import _stereo_ftp_ref as S
    mx, my = S.undistort_maps(np.array(r["intrinsic1"]), r["distCoeffs1"], (1280, 720))
    yy, xx = np.mgrid[0:720, 0:1280]
    assert np.array_equal(mx, xx.astype(np.float32)) and np.array_equal(my, yy.astype(np.float32))
    dec = G.decode(stack, 1280, 720, 5)
    assert 0.5 < (dec[..., 0] >= 0).mean() < 0.95
    dense = G.cloud_dense(G.geometry(r), dec, 0, 0)
    gc = ss.active.GrayCode(G.make_rig(ss, r))
    t = torch.from_numpy(stack).cuda()
    assert np.array_equal(_np(ss.active.grayCodeDecode(t, (1280, 720), maps=(mx, my))), dec)
    pts = gc.getCloud(t)
    assert G.same_points(_np(pts), G.compact(dense, dec))
    assert G.same_points(_np(gc.getCloud(t, dense=True)), dense)
    assert G.same_points(gc.getCloud(stack), _np(pts))                          # the host-array route
