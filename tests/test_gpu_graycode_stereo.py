"""GPU tier of ss.active.GrayCodeStereo / grayCodeMatch / stereoTriangulate: the scatter, match and cloud kernels of
graycode_stereo_kernels.hip.h against the numpy restatement tests/_graycode_stereo_ref.py.  Every comparison is exact: integers by
value, float64 on bit patterns (NaN where the restatement has NaN).  Shapes are the smallest at which a path can go wrong: a block
is 1024 consecutive pixels or cells (256 threads x 4), so a 67 x 37 camera is three workgroups with a partial last one, its rows
are no multiple of 4, and a 64 x 32 projector is two blocks of cells."""
import functools

import numpy as np
import pytest

import _ftp_cloud_ref as C
import _graycode_ref as G
import _graycode_stereo_ref as S
import _phaseshift_ref as P

pytestmark = pytest.mark.gpu
RES1, RES2 = (67, 37), (53, 41)
REDUCES = ("last", "mean")


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


@functools.lru_cache(maxsize=None)
def _random_stacks(proj):
    n = G.num_patterns(*proj)
    stacks = (G.random_stack(41, n + 1, RES1[1], RES1[0]), G.random_stack(42, n, RES2[1], RES2[0]))      # (an extra image is ignored)
    for s in stacks:
        s.setflags(write=False)
    return stacks


@functools.lru_cache(maxsize=None)
def _want(proj, reduce, rois=(None, None), dist=False, stacks="random"):
    """(rig dict, stacks, dense cloud, compacted cloud, matches, decoded maps) of the restatement, computed once and shared"""
    r = S.two_camera_rig(RES1, RES2, dist1=C.DIST_MODELS["d5"], dist2=[0.11, -0.07, 0.002, -0.001, 0.02]) if dist else S.two_camera_rig(RES1, RES2)
    st = _random_stacks(proj) if stacks == "random" else stacks()
    dense, m, decoded = S.get_cloud(r, st, proj, 5, reduce, rois, dense=True)
    compact = S.cloud(S.geometry(r), m)
    for a in (dense, compact, m) + tuple(decoded):
        a.setflags(write=False)
    return r, st, dense, compact, m, decoded


def _all_routes(ss, torch, proj, reduce, rois=(None, None), dist=False, stacks="random"):
    """getCloud compacted and dense, on host arrays and on device tensors, twice, against the restatement"""
    r, st, dense, compact, m, decoded = _want(proj, reduce, rois, dist, stacks)
    gs = ss.active.GrayCodeStereo(G.make_rig(ss, r), proj, reduce=reduce)
    tensors = tuple(torch.from_numpy(np.array(s)).cuda() for s in st)
    for images in (st, tensors):
        on_dev = images is tensors
        for _ in range(2):                                                      # two consecutive calls: identical bytes
            pts = gs.getCloud(images, roi1=rois[0], roi2=rois[1])
            assert pts.is_cuda if on_dev else isinstance(pts, np.ndarray)
            assert tuple(pts.shape) == compact.shape and G.same_points(_np(pts), compact)
            full = gs.getCloud(images, roi1=rois[0], roi2=rois[1], dense=True)
            assert tuple(full.shape) == (proj[1], proj[0], 3) and G.same_points(_np(full), dense)
    return r, st, dense, compact, m, decoded


def _seen(decoded, proj):
    """bool [Hp, Wp]: the projector pixels some pixel of the map decodes to"""
    return S.table_last(decoded, (0, 0), proj)[..., 0] >= 0


# ------------------------------------------------------------------------------------------------ random stacks
@pytest.mark.parametrize("reduce", REDUCES)
@pytest.mark.parametrize("proj", [(13, 6), (64, 32)])
def test_random_stacks_all_routes(ss, torch, proj, reduce):
    r, st, dense, compact, m, decoded = _all_routes(ss, torch, proj, reduce)
    for d in decoded:
        assert 0.2 < float((d[..., 0] >= 0).mean()) < 0.8
    s1, s2 = _seen(decoded[0], proj), _seen(decoded[1], proj)
    assert (s1 & s2).any() and compact.shape[0] == int((s1 & s2).sum())
    if proj == (64, 32):        # (78 cells under 1000 valid pixels per camera are all seen by both: the small rois below thin them out)
        assert (s1 ^ s2).any() and (~s1 & ~s2).any()
    if reduce == "mean":
        assert (np.asarray(m)[s1 & s2] % 0.5 != 0).any()                         # a centroid that is no pixel centre


@pytest.mark.parametrize("reduce", REDUCES)
def test_rois_with_origins_give_absolute_coordinates(ss, torch, reduce):
    """non-zero origins, regions whose rows are not whole threads; small enough that a 13 x 6 projector has pixels seen by both
    cameras, by one only and by none"""
    proj, rois = (13, 6), ((5, 3, 18, 9), (7, 2, 16, 11))
    r, st, dense, compact, m, decoded = _all_routes(ss, torch, proj, reduce, rois)
    assert decoded[0].shape == (6, 13, 2) and decoded[1].shape == (9, 9, 2)
    s1, s2 = _seen(decoded[0], proj), _seen(decoded[1], proj)
    assert (s1 & s2).any() and (s1 ^ s2).any() and (~s1 & ~s2).any()
    both = np.asarray(m)[s1 & s2]
    assert both[:, 0].min() >= 5.5 and both[:, 0].max() <= 17.5 and both[:, 1].min() >= 3.5 and both[:, 3].min() >= 2.5 and both[:, 2].max() <= 15.5
    if reduce == "last":
        origin0 = S.match(decoded[0], decoded[1], proj, reduce)                  # the same maps without their origins
        assert np.array_equal(both - origin0[s1 & s2], np.broadcast_to([5.0, 3.0, 7.0, 2.0], both.shape))
    # larger regions with origins: several workgroups per camera
    _all_routes(ss, torch, (64, 32), reduce, ((5, 3, 60, 30), (0, 2, 50, 40)))


def test_empty_roi_and_no_match_give_no_points(ss, torch):
    proj = (13, 6)
    r = S.two_camera_rig(RES1, RES2)
    st = _random_stacks(proj)
    gs = ss.active.GrayCodeStereo(G.make_rig(ss, r), proj)
    tensors = tuple(torch.from_numpy(np.array(s)).cuda() for s in st)
    for images in (st, tensors):
        out = gs.getCloud(images, roi1=(3, 5, 3, 9))
        assert tuple(out.shape) == (0, 1, 3) and (out.is_cuda if images is tensors else True)
        assert np.isnan(_np(gs.getCloud(images, roi2=(0, 7, 9, 7), dense=True))).all()
    # camera 1 sees nothing (no contrast anywhere): the kernels run and match nothing
    dark = (np.zeros_like(st[0]), st[1])
    for reduce in REDUCES:
        gs = ss.active.GrayCodeStereo(G.make_rig(ss, r), proj, reduce=reduce)
        for images in (dark, tuple(torch.from_numpy(np.array(s)).cuda() for s in dark)):
            out = gs.getCloud(images)
            assert tuple(out.shape) == (0, 1, 3) and str(out.dtype).endswith("float64")
            full = _np(gs.getCloud(images, dense=True))
            assert full.shape == (6, 13, 3) and np.isnan(full).all()


# ------------------------------------------------------------------------------------------------ contention and the per-thread merge
def _no_planes():
    return (np.zeros((0, RES1[1], RES1[0]), np.uint8), np.zeros((0, RES2[1], RES2[0]), np.uint8))


@pytest.mark.parametrize("reduce", REDUCES)
def test_total_contention_on_a_one_pixel_projector(ss, torch, reduce):
    """a 1 x 1 projector has no planes and every pixel decodes to (0, 0): all 2479 + 2173 pixels of three workgroups per camera land
    on one cell"""
    r, st, dense, compact, m, decoded = _all_routes(ss, torch, (1, 1), reduce, stacks=_no_planes)
    assert all((d == 0).all() for d in decoded) and decoded[0].shape == (37, 67, 2) and decoded[1].shape == (41, 53, 2)
    want = [66.5, 36.5, 52.5, 40.5] if reduce == "last" else [33.5, 18.5, 26.5, 20.5]      # the last pixel / the exact centroid
    assert np.array_equal(np.asarray(m).reshape(4), want) and compact.shape == (1, 1, 3) and np.isfinite(compact).all()
    for images in (decoded, tuple(torch.from_numpy(np.array(d)).cuda() for d in decoded)):
        got = ss.active.grayCodeMatch(images[0], images[1], (1, 1), reduce=reduce)
        assert np.array_equal(_np(got).reshape(4), want)
    # a centroid that is not representable exactly: 5 pixels of a row of 7 -> x = (0 + 1 + 2 + 3 + 4 + ... ) / n, one division
    d = np.zeros((3, 7, 2), np.int32)
    d[1, 2:] = -1
    got = ss.active.grayCodeMatch(d, d[:, :5], (1, 1), reduce="mean")
    assert G.same_points(got, S.match(d, d[:, :5], (1, 1), "mean")) and got[0, 0, 0] == (21 + 1 + 21) / 16 + 0.5


def _run_stacks():
    proj = (64, 32)
    a, cell_a = S.render_runs(RES1, proj, (1, 2, 3, 4), start=0)
    b, cell_b = S.render_runs(RES2, proj, (4, 3, 2, 1, 2), start=3)
    return a, b


@pytest.mark.parametrize("reduce", REDUCES)
def test_runs_of_equal_codes_across_thread_and_wave_boundaries(ss, torch, reduce):
    """neighbouring pixels that share a code in runs of 1, 2, 3 and 4, which the scatter merges per thread: runs inside one thread,
    and runs cut by a thread's, a wave's and a workgroup's boundary"""
    proj = (64, 32)
    cut, inside = {4: set(), 256: set(), 1024: set()}, set()
    for res, runs, start in ((RES1, (1, 2, 3, 4), 0), (RES2, (4, 3, 2, 1, 2), 3)):
        cell = S.render_runs(res, proj, runs, start)[1].ravel()
        for every in cut:
            b = np.arange(every, cell.size, every)
            b = b[(cell[b] >= 0) & (cell[b] == cell[b - 1])]                     # boundaries inside a run
            cut[every] |= {int((cell == c).sum()) for c in cell[b]}               # the lengths of the runs they cut
        inside |= {int(n) for p in range(0, cell.size - 3, 4) for c, n in zip(*np.unique(cell[p:p + 4], return_counts=True)) if c >= 0}
    assert cut[4] == cut[256] == {2, 3, 4} and cut[1024] and inside == {1, 2, 3, 4}, (cut, inside)
    r, st, dense, compact, m, decoded = _all_routes(ss, torch, proj, reduce, stacks=_run_stacks)
    cell1 = S.render_runs(RES1, proj, (1, 2, 3, 4), 0)[1]
    assert np.array_equal(decoded[0][..., 1] * 64 + decoded[0][..., 0], cell1)    # the render decodes to what it was made from
    assert compact.shape[0] > 300
    if reduce == "mean":
        # a run of four pixels in one row has its centroid 1.5 pixels right of its first pixel's centre
        sx, sy, n = S.table_mean(decoded[0], (0, 0), proj)
        assert (n == 4).any() and (n == 1).any()


# ------------------------------------------------------------------------------------------------ undistortion of both cameras
@pytest.mark.parametrize("reduce", REDUCES)
def test_undistortion_maps_of_both_cameras(ss, torch, reduce):
    """rig d5 for camera 1 and a distorted camera 2: the decode through each camera's maps against remap-then-decode"""
    proj = (64, 32)
    r, st, dense, compact, m, decoded = _all_routes(ss, torch, proj, reduce, dist=True)
    plain = _want(proj, reduce)[5]
    assert not np.array_equal(plain[0], decoded[0]) and not np.array_equal(plain[1], decoded[1])      # the maps matter
    assert compact.shape[0] > 100


# ------------------------------------------------------------------------------------------------ the pieces
@pytest.mark.parametrize("reduce", REDUCES)
def test_match_then_triangulate_is_getcloud(ss, torch, reduce):
    from simplestereo_amd import _rigs
    proj = (64, 32)
    r, st, dense, compact, m, decoded = _want(proj, reduce, dist=True)
    rig = G.make_rig(ss, r)
    gs = ss.active.GrayCodeStereo(rig, proj, reduce=reduce)
    for dev in (False, True):
        up = (lambda a: torch.from_numpy(np.array(a)).cuda()) if dev else (lambda a: a)
        d = [ss.active.grayCodeDecode(up(st[i]), proj, maps=tuple(up(x) for x in _rigs._undistort_maps(rig, i + 1))) for i in range(2)]
        assert np.array_equal(_np(d[0]), decoded[0]) and np.array_equal(_np(d[1]), decoded[1])
        got = ss.active.grayCodeMatch(d[0], d[1], proj, reduce=reduce)
        assert (got.is_cuda if dev else isinstance(got, np.ndarray)) and tuple(got.shape) == (32, 64, 4) and G.same_points(_np(got), m)
        keep = ~np.isnan(_np(got)[..., 0])
        pairs = got[up(keep)] if dev else got[keep]
        pts = ss.active.stereoTriangulate(rig, pairs[:, :2], pairs[:, 2:])
        cloud = gs.getCloud(tuple(up(s) for s in st))
        assert tuple(pts.shape) == tuple(cloud.shape) == compact.shape
        assert G.same_points(_np(pts), _np(cloud)) and G.same_points(_np(pts), compact)
        # all cells at once: three NaN where a couple holds a NaN
        flat = got.reshape(-1, 4)
        assert G.same_points(_np(ss.active.stereoTriangulate(rig, flat[:, :2], flat[:, 2:])).reshape(32, 64, 3), dense)
        # origins, a map that is a misaligned view, float32 couples converted to float64
        part = ss.active.grayCodeMatch(d[0][1:], d[1][:, 2:], proj, reduce=reduce, origin1=(0, 1), origin2=(2, 0))
        assert G.same_points(_np(part), S.match(decoded[0][1:], decoded[1][:, 2:], proj, reduce, (0, 1), (2, 0)))
    p32 = pairs.float() if dev else pairs.astype(np.float32)
    assert G.same_points(_np(ss.active.stereoTriangulate(rig, p32[:, :2], p32[:, 2:])),
                         S.triangulate(S.geometry(r), _np(p32)[:, :2].astype(np.float64), _np(p32)[:, 2:].astype(np.float64)))


def test_codes_outside_the_projector_contribute_nothing(ss, torch):
    """maps decoded for a 16 x 8 projector matched on a 13 x 6 table: the scatter stays inside the table"""
    st = _random_stacks((13, 6))
    d = [G.decode(np.asarray(s), 16, 8, 5) for s in st]
    assert (d[0][..., 0] >= 13).any() and (d[1][..., 1] >= 6).any()
    d[0][0, 0] = (1 << 30, 1 << 30)
    d[1][0, 0] = (-7, 3)
    for reduce in REDUCES:
        want = S.match(d[0], d[1], (13, 6), reduce)
        assert G.same_points(ss.active.grayCodeMatch(d[0], d[1], (13, 6), reduce=reduce), want)
        got = ss.active.grayCodeMatch(torch.from_numpy(d[0]).cuda(), torch.from_numpy(d[1]).cuda(), (13, 6), reduce=reduce)
        assert G.same_points(_np(got), want)


def test_triangulation_against_the_references_recorded_points(ss, torch):
    """stereoTriangulate on the seeded correspondences of rig `none` of tests/golden/phaseshift_cases.*: bit for bit the restatement,
    and within that fixture's own tolerance of the points the reference's StructuredLightRig.triangulate recorded"""
    meta, arrays = P.load()
    c = meta["rigs"]["none"]
    sl = ss.StructuredLightRig(G.make_rig(ss, c["rig"]))
    cam, proj = P.correspondences(c["rig"], c["n"], c["seed"])
    want = S.triangulate(P.sl_rig(c["rig"])["geom"], cam, proj)
    ref = arrays["rig_none__points"]
    for up in (lambda a: a, lambda a: torch.from_numpy(a).cuda()):
        got = _np(ss.active.stereoTriangulate(sl, up(cam), up(proj)))
        assert G.same_points(got, want)
        err = float(C.rel_err(got, ref.astype(np.longdouble)).max())
        print("stereoTriangulate against the reference's points: %.3e (tolerance %.3e)" % (err, c["tol"]))
        assert err <= c["tol"]
    # the plain rig's own baseline (not the StructuredLightRig's) scales the same points
    plain = G.make_rig(ss, c["rig"])
    got = ss.active.stereoTriangulate(plain, cam, proj)
    assert np.allclose(got, want * (c["plain_baseline"] / c["baseline"]), rtol=1e-12, atol=0)


def test_a_projector_of_two_to_the_31_pixels_is_refused_before_anything_is_allocated(ss, torch):
    rig = G.make_rig(ss, S.two_camera_rig(RES1, RES2))
    d = torch.zeros((4, 8, 2), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="2\\^31"):
        ss.active.GrayCodeStereo(rig, (65536, 32768))
    with pytest.raises(ValueError, match="2\\^31"):
        ss.active.grayCodeMatch(d, d, (65536, 32768))
    assert torch.cuda.memory_allocated() == before
