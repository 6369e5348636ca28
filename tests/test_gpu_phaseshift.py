"""GPU tier of phase shifting and ss.StructuredLightRig: phaseshift_decode_kernel and sl_triangulate_kernel against the numpy
restatement tests/_phaseshift_ref.py and what the reference's own StructuredLightRig recorded (tests/golden/phaseshift_cases.*).
The decode is compared within the recorded tolerance (the device's atan2 is not numpy's) with an identical NaN mask; the
triangulation on its bit patterns.  Shapes are the smallest at which a path can go wrong: a block is 1024 consecutive region pixels
(256 threads x 4), so the 67 x 37 camera is three blocks with a ragged end, and the roi's origin breaks the four-pixel alignment."""
import numpy as np
import pytest

import _ftp_cloud_ref as C
import _graycode_ref as G
import _phaseshift_ref as P
import _stereo_ftp_ref as S

pytestmark = pytest.mark.gpu
META, ARRAYS = P.load()
PROJ = tuple(META["proj_res"])
MODULATIONS = (None, 0, 1.5, 50)


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


def _box(roi, res):
    return (0, 0, res[0], res[1]) if roi is None else tuple(roi)


_SCENES = {}


def _decode_case(name):
    """(stack, maps | None, what the decode sees of the stack, box) of a recorded decode case, built once"""
    if name not in _SCENES:
        c = META["decode"][name]
        stack = P.scene(c["seed"], c["res1"], PROJ, c["periods"])
        maps, seen = None, stack
        if c["maps_of_rig"] is not None:
            r = META["rigs"][c["maps_of_rig"]]["rig"]
            maps = S.undistort_maps(np.array(r["intrinsic1"]), r["distCoeffs1"], tuple(c["res1"]))
            seen = G.remap_stack(stack, *maps)
        x0, y0, w, h = _box(c["roi"], c["res1"])
        cut = np.ascontiguousarray(seen[:, y0:y0 + h, x0:x0 + w])
        cut.setflags(write=False)
        _SCENES[name] = (stack, maps, cut, (x0, y0, w, h))
    return _SCENES[name]


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("name", sorted(META["decode"]))
def test_decode_is_the_restatement_within_its_tolerance(ss, torch, name):
    c = META["decode"][name]
    stack, maps, cut, box = _decode_case(name)
    periods, roi = c["periods"], c["roi"]
    dmaps = None if maps is None else tuple(torch.from_numpy(m).cuda() for m in maps)
    t = torch.from_numpy(stack).cuda()
    masks = []
    for m in MODULATIONS:
        want, tie = P.decode(cut, periods, PROJ, thr2=P.mod_thr2(m), details=True)
        assert tie.max() <= META["tie_max"]                                     # no k of the input hangs on a rounding
        got = ss.active.phaseShiftDecode(stack, periods, PROJ, maps=maps, roi=roi, min_modulation=m)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.shape == want.shape == (box[3], box[2], 2)
        nan = np.isnan(want[..., 0])
        assert np.array_equal(np.isnan(got), np.isnan(want))                    # the mask, on both coordinates
        err = float(np.abs(got - want)[~nan].max()) if (~nan).any() else 0.0
        print("%s, min_modulation %s: %d of %d masked, worst |p - restatement| %.3e (numpy %.3e, tolerance %.3e)"
              % (name, m, int(nan.sum()), nan.size, err, c["numpy_err"], c["tol"]))
        assert err <= c["tol"]
        dev = ss.active.phaseShiftDecode(t, periods, PROJ, maps=dmaps, roi=roi, min_modulation=m)
        assert dev.is_cuda and dev.dtype == torch.float64 and P.same_bits(_np(dev), got)      # host route == device route, bit for bit
        masks.append(int(nan.sum()))
    assert masks[0] == masks[1] == 0                                            # None and 0 mask nothing
    if name == "full":                                                          # the weakly lit block (a^2 + b^2 = 10 there): whole at 50
        assert masks[2] == 0 and masks[3] == 35
    if maps is not None:                                                        # host maps with a device stack are uploaded
        mixed = ss.active.phaseShiftDecode(t, periods, PROJ, maps=maps, roi=roi)
        assert P.same_bits(_np(mixed), ss.active.phaseShiftDecode(stack, periods, PROJ, maps=maps, roi=roi))


def test_decode_ignores_extra_images_and_takes_a_list(ss, torch):
    c = META["decode"]["roi"]
    stack = _decode_case("roi")[0]
    assert stack.shape[0] == 4 * 5 + 1                                          # the image in normal light is in the stack
    want = ss.active.phaseShiftDecode(stack[:20], c["periods"], PROJ, roi=c["roi"])
    assert P.same_bits(ss.active.phaseShiftDecode(stack, c["periods"], PROJ, roi=c["roi"]), want)
    assert P.same_bits(ss.active.phaseShiftDecode(list(stack), c["periods"], PROJ, roi=c["roi"]), want)
    assert P.same_bits(ss.active.phaseShiftDecode(stack, tuple(tuple(p) for p in c["periods"]), PROJ, roi=tuple(c["roi"])), want)


def test_empty_roi_and_executed_limits(ss, torch):
    c = META["decode"]["full"]
    stack = _decode_case("full")[0]
    t = torch.from_numpy(stack).cuda()
    for images in (stack, t):
        out = ss.active.phaseShiftDecode(images, c["periods"], PROJ, roi=(3, 5, 0, 4))
        assert tuple(out.shape) == (4, 0, 2) and (out.is_cuda if images is t else isinstance(out, np.ndarray))
        assert tuple(ss.active.phaseShiftDecode(images, c["periods"], PROJ, roi=(66, 36, 1, 1)).shape) == (1, 1, 2)
        seventeen = [64.0 / (i + 1) for i in range(17)]
        for bad in ((seventeen, [32.0]), ([64.0], seventeen), ([], [32.0]), ([64.0], [])):      # 17 periods on an axis, and 0
            with pytest.raises(ValueError):
                ss.active.phaseShiftDecode(images, bad, PROJ)
        with pytest.raises(ValueError):
            ss.active.phaseShiftDecode(images[:19], c["periods"], PROJ)
    with pytest.raises(TypeError):                                              # device maps with a host stack
        ss.active.phaseShiftDecode(stack, c["periods"], PROJ, maps=tuple(torch.zeros((37, 67), dtype=torch.float32).cuda() for _ in range(2)))


# ------------------------------------------------------------------------------------------------ StructuredLightRig
@pytest.mark.parametrize("name", sorted(META["rigs"]))
def test_triangulate_is_the_restatement_and_near_the_reference(ss, torch, name):
    c = META["rigs"][name]
    sl = ss.StructuredLightRig(G.make_rig(ss, c["rig"]))
    cam, proj = P.correspondences(c["rig"], c["n"], c["seed"])
    want = P.triangulate(P.sl_rig(c["rig"])["geom"], cam, proj)
    got = sl.triangulate(cam, proj)
    assert isinstance(got, np.ndarray) and got.shape == (c["n"], 1, 3) and P.same_bits(got, want)
    dev = sl.triangulate(torch.from_numpy(cam).cuda(), torch.from_numpy(proj).cuda())
    assert dev.is_cuda and dev.dtype == torch.float64 and P.same_bits(_np(dev), want)
    err = float(C.rel_err(got, ARRAYS["rig_%s__points" % name].astype(np.longdouble)).max())
    print("%s: worst relative distance to the reference's points %.3e (numpy %.3e, tolerance %.3e)" % (name, err, c["numpy_err"], c["tol"]))
    assert err <= c["tol"]
    # a NaN correspondence is three NaN, in either coordinate; the other points are what they were
    holes = proj.copy()
    holes[3, 0] = holes[17, 1] = np.nan
    holes[25] = np.nan
    want_holes = want.copy()
    want_holes[[3, 17, 25]] = np.nan
    assert P.same_bits(P.triangulate(P.sl_rig(c["rig"])["geom"], cam, holes), want_holes)
    assert P.same_bits(sl.triangulate(cam, holes), want_holes)
    assert P.same_bits(_np(sl.triangulate(torch.from_numpy(cam).cuda(), torch.from_numpy(holes).cuda())), want_holes)


def test_triangulate_shapes_dtypes_and_sides(ss, torch):
    c = META["rigs"]["d8"]
    sl = ss.StructuredLightRig(G.make_rig(ss, c["rig"]))
    g = P.sl_rig(c["rig"])["geom"]
    cam, proj = P.correspondences(c["rig"], 1030, 7)                            # five workgroups of 256, a ragged last one
    want = P.triangulate(g, cam, proj)
    assert P.same_bits(sl.triangulate(cam.reshape(103, 10, 2), proj.reshape(-1, 1, 2)), want)        # any shape ending in 2
    assert P.same_bits(_np(sl.triangulate(torch.from_numpy(cam).cuda()[::1], torch.from_numpy(proj).cuda().reshape(10, 103, 2))), want)
    assert P.same_bits(sl.triangulate(cam[:1], proj[:1]), want[:1])
    cam32, proj32 = cam.astype(np.float32), proj.astype(np.float32)             # float32 in: converted, float64 out
    want32 = P.triangulate(g, cam32.astype(np.float64), proj32.astype(np.float64))
    assert P.same_bits(sl.triangulate(cam32, proj32), want32)
    assert P.same_bits(_np(sl.triangulate(torch.from_numpy(cam32).cuda(), torch.from_numpy(proj32).cuda())), want32)
    icam = np.rint(cam).astype(np.int32)                                        # integer pixels
    assert P.same_bits(sl.triangulate(icam, proj), P.triangulate(g, icam.astype(np.float64), proj))
    noncontig = np.ascontiguousarray(np.concatenate([cam, proj], axis=1))       # views: made contiguous
    assert P.same_bits(sl.triangulate(noncontig[:, :2], noncontig[:, 2:]), want)
    out = sl.triangulate(torch.zeros((0, 2)).cuda(), torch.zeros((0, 2), dtype=torch.float64).cuda())
    assert out.is_cuda and tuple(out.shape) == (0, 1, 3) and out.dtype == torch.float64
    for a, b in ((cam, torch.from_numpy(proj).cuda()), (torch.from_numpy(cam).cuda(), proj)):
        with pytest.raises(TypeError):
            sl.triangulate(a, b)


def test_undistort_camera_image_on_the_device_is_the_host_bytes(ss, torch):
    r = META["rigs"]["d12"]["rig"]
    sl = ss.StructuredLightRig(G.make_rig(ss, r))
    rng = np.random.default_rng(5)
    gray, bgr = rng.integers(0, 256, (37, 67), dtype=np.uint8), rng.integers(0, 256, (37, 67, 3), dtype=np.uint8)
    for img in (gray, bgr):
        want = sl.undistortCameraImage(img)
        got = sl.undistortCameraImage(torch.from_numpy(img).cuda())
        assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous() and np.array_equal(_np(got), want)
        assert not np.array_equal(want, img)
    with pytest.raises(ValueError):
        sl.undistortCameraImage(torch.zeros((37, 67, 4), dtype=torch.uint8).cuda())


# ------------------------------------------------------------------------------------------------ PhaseShift.getCloud
@pytest.mark.parametrize("name", sorted(META["cloud"]))
def test_get_cloud_is_decode_then_triangulate(ss, torch, name):
    c = META["cloud"][name]
    r = META["rigs"][c["rig"]]["rig"]
    rig = G.make_rig(ss, r)
    periods, roi = c["periods"], c["roi"]
    box = _box(roi, r["res1"])
    stack = P.scene(c["seed"], r["res1"], PROJ, periods)
    maps = S.undistort_maps(np.array(r["intrinsic1"]), r["distCoeffs1"], tuple(r["res1"]))
    seen = G.remap_stack(stack, *maps)[:, box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
    g = P.sl_rig(r)["geom"]
    t = torch.from_numpy(stack).cuda()
    for m in (None, 50):
        ps = ss.active.PhaseShift(rig, periods, min_modulation=m)
        want = P.triangulate(g, P.grid(box), P.decode(seen, periods, PROJ, thr2=P.mod_thr2(m))).reshape(box[3], box[2], 3)
        for images in (stack, t):
            cloud = ps.getCloud(images, roi=roi)
            assert (cloud.is_cuda if images is t else isinstance(cloud, np.ndarray)) and tuple(cloud.shape) == want.shape
            proj = ss.active.phaseShiftDecode(images, periods, PROJ, maps=maps, roi=roi, min_modulation=m)
            cam = torch.from_numpy(P.grid(box)).cuda() if images is t else P.grid(box)
            chain = ps.rig.triangulate(cam, proj)                               # bitwise the two public calls
            assert P.same_bits(_np(cloud).reshape(-1, 1, 3), _np(chain))
            cloud = _np(cloud)
            nan = np.isnan(want[..., 0])
            assert np.array_equal(np.isnan(cloud), np.isnan(want)) and nan.any() == (m is not None)
            err = float(C.rel_err(cloud, want.astype(np.longdouble))[~nan].max())
            print("%s, min_modulation %s: worst relative distance to the restatement chain %.3e (numpy %.3e, tolerance %.3e)"
                  % (name, m, err, c["numpy_err"], c["tol"]))
            assert err <= c["tol"]
    assert isinstance(ps.rig, ss.StructuredLightRig) and "host" in ps._cache    # the maps are built once per instance
