"""CPU tier of phase shifting and ss.StructuredLightRig: the fifth public header include/ssamd_structured_light.h against its ctypes
rows (the four older headers unchanged), its argument errors without a device, the Python exception tables, ``phaseShiftPattern``
against ``buildFringe``, and the numpy restatement tests/_phaseshift_ref.py -- and the package's host side -- against what the
reference's own StructuredLightRig recorded (tests/golden/phaseshift_cases.*).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _ftp_cloud_ref as C
import _graycode_ref as G
import _plane_stack as X
import _phaseshift_ref as P
from test_native_signatures_cpu import SCALARS, _is_pointer_class, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META, ARRAYS = P.load()
PERIODS = META["decode"]["full"]["periods"]
PROJ = tuple(META["proj_res"])


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


# ------------------------------------------------------------------------------------------------ the fifth header
def test_header_parses_and_matches_its_ctypes_rows():
    from simplestereo_amd import _native
    with open(os.path.join(ROOT, "include", "ssamd_structured_light.h")) as f:
        header = f.read()
    protos = _prototypes(header)
    assert sorted(protos) == ["ssamd_phaseshift_decode", "ssamd_phaseshift_decode_device", "ssamd_sl_triangulate", "ssamd_sl_triangulate_device"]
    assert set(protos) == set(re.findall(r"\b(ssamd_[a-z0-9_]+)\s*\(", header))
    assert int(re.search(r"#define SSAMD_SL_VERSION (\d+)", header).group(1)) == _native.SL_VERSION == 1
    assert int(re.search(r"#define SSAMD_SL_MAX_PERIODS (\d+)", header).group(1)) == 8
    assert protos["ssamd_phaseshift_decode"] == ("int", ["ptr", "int", "int", "int", "ptr", "ptr"] + ["int"] * 6 + ["ptr", "ptr"] + ["int"] * 3 + ["ptr", "int"])
    assert protos["ssamd_phaseshift_decode_device"][1] == protos["ssamd_phaseshift_decode"][1][:-1] + ["ptr"]
    assert protos["ssamd_sl_triangulate"] == ("int", ["ptr", "ptr", "long long", "int", "int", "int", "ptr", "ptr", "int"])
    assert protos["ssamd_sl_triangulate_device"][1] == protos["ssamd_sl_triangulate"][1][:-1] + ["ptr"]
    lib = _native.lib()
    for name, (ret, kinds) in protos.items():
        fn = getattr(lib, name)                                                 # exported from the same library
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(fn.argtypes, kinds)):
            assert _is_pointer_class(t) if kind == "ptr" else t is SCALARS[kind], (name, i, t, kind)


def test_the_older_headers_are_as_they_were():
    from simplestereo_amd import _native
    for name, count in (("ssamd.h", 54), ("ssamd_active.h", 4), ("ssamd_graycode.h", 6), ("ssamd_ftp_mapping.h", 4)):
        with open(os.path.join(ROOT, "include", name)) as f:
            header = f.read()
        assert "phaseshift" not in header.lower() and "sl_triangulate" not in header.lower(), name
        assert len(_prototypes(header)) == count, name
    assert (_native.ABI_VERSION, _native.ACTIVE_VERSION, _native.GRAYCODE_VERSION, _native.FTP_MAPPING_VERSION, _native.K_COUNT) == (8, 1, 1, 1, 12)
    assert _native.lib().ssamd_abi_version() == 8


def test_abi_argument_errors_need_no_device():
    """SSAMD_EINVAL for what include/ssamd_structured_light.h lists, decided before any device is looked for"""
    from simplestereo_amd import _native
    lib = _native.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    planes = np.zeros((20, 4, 8), np.uint8)
    out = np.zeros((4, 8, 3), np.float64)
    maps = np.zeros((4, 8), np.float32)
    tx, ty = np.array([64.0, 16.0, 5.0]), np.array([32.0, 8.0])

    def decode(planes=planes.ctypes.data, n=20, hc=4, wc=8, mx=None, my=None, x0=0, y0=0, h=4, w=8, nx=3, ny=2, tx=tx, ty=ty, pw=64, ph=32, thr2=0,
               out=out.ctypes.data, device=False):
        args = (planes, n, hc, wc, mx, my, x0, y0, h, w, nx, ny, None if tx is None else tx.ctypes.data_as(dp), None if ty is None else ty.ctypes.data_as(dp),
                pw, ph, thr2, out)
        return lib.ssamd_phaseshift_decode_device(*args, None) if device else lib.ssamd_phaseshift_decode(*args, -1)

    bad = X.phase_bad(maps)
    for kw in bad:
        for device in (False, True):
            assert decode(device=device, **kw) == _native.EINVAL, (kw, device)
            assert lib.ssamd_last_error()
    assert decode(out=out.ctypes.data + 8, device=True) == _native.EINVAL                # a misaligned output
    assert decode(h=0) == 0 and decode(w=0, planes=None, out=None) == 0                  # an empty region does nothing
    assert decode(h=0, device=True) == 0
    assert decode(h=0, nx=0, ny=5) == _native.EINVAL                                     # ... but its arguments are checked

    geom = np.ones(68)
    pts = np.zeros((5, 2))

    def tri(cam=pts.ctypes.data, proj=pts.ctypes.data, n=5, w=1, x0=0, y0=0, geom=geom, out=out.ctypes.data, device=False):
        args = (cam, proj, n, w, x0, y0, None if geom is None else geom.ctypes.data_as(dp), out)
        return lib.ssamd_sl_triangulate_device(*args, None) if device else lib.ssamd_sl_triangulate(*args, -1)

    bad = [dict(proj=None), dict(out=None), dict(geom=None), dict(n=-1), dict(n=(1 << 38) + 1), dict(cam=None, w=0), dict(cam=None, x0=-1), dict(cam=None, y0=-1)]
    for i in (12, 27, 36, 40, 58, 67):
        g = geom.copy()
        g[i] = np.nan if i % 2 else np.inf
        bad.append(dict(geom=g))
    for kw in bad:
        for device in (False, True):
            assert tri(device=device, **kw) == _native.EINVAL, (kw, device)
    assert tri(out=out.ctypes.data + 4, device=True) == _native.EINVAL and tri(proj=pts.ctypes.data + 4, device=True) == _native.EINVAL
    assert tri(n=0) == 0 and tri(n=0, proj=None, out=None, device=True) == 0             # no point: nothing is done
    for i in (0, 11, 37, 39):                                                            # entries the triangulation does not read
        g = geom.copy()
        g[i] = np.nan
        assert tri(n=0, geom=g) == 0
    assert tri(w=0, x0=-5) != _native.EINVAL                                             # with cam the grid arguments are not read


# ------------------------------------------------------------------------------------------------ patterns
@pytest.mark.parametrize("periods, res", [(PERIODS, PROJ), ([[13.0], [7.5, 3.0]], (13, 6)), ([[1920.0, 240.0, 30.0], [1080.0]], (40, 24))])
def test_pattern_is_the_buildfringe_stack(ss, periods, res):
    a = ss.active
    got = a.phaseShiftPattern(periods, res)
    n = 4 * (len(periods[0]) + len(periods[1]))
    assert got.dtype == np.uint8 and got.shape == (n, res[1], res[0])
    want = [a.buildFringe(T, shift=i * T / 4, dims=res) for T in periods[0] for i in range(4)]
    want += [a.buildFringe(T, shift=i * T / 4, dims=res, vertical=True) for T in periods[1] for i in range(4)]
    assert np.array_equal(got, np.stack(want)) and np.array_equal(got, P.pattern(periods, res))
    assert (got[:4 * len(periods[0])] == got[:4 * len(periods[0]), :1]).all() and (got[4 * len(periods[0]):] == got[4 * len(periods[0]):, :, :1]).all()


def test_the_restatement_decodes_its_own_pattern():
    """a camera that sees the projector pixel for pixel: px = x, py = y up to the 8-bit quantisation of the fringes"""
    periods = [[64.0, 16.0], [32.0, 8.0]]
    got, tie = P.decode(P.pattern(periods, PROJ), periods, PROJ, details=True)
    yy, xx = np.mgrid[0:PROJ[1], 0:PROJ[0]]
    assert np.abs(got[..., 0] - xx).max() < 0.1 and np.abs(got[..., 1] - yy).max() < 0.1 and tie.max() < 0.1


# ------------------------------------------------------------------------------------------------ the goldens
@pytest.mark.parametrize("name", sorted(META["rigs"]))
def test_restatement_and_package_hold_what_the_reference_holds(ss, name):
    c = META["rigs"][name]
    want = P.sl_rig(c["rig"])
    sl = ss.StructuredLightRig(G.make_rig(ss, c["rig"]))
    for f in ("R1", "R2", "R", "R_inv"):
        ref = ARRAYS["rig_%s__%s" % (name, f)]
        assert ref.dtype == np.float64 and np.array_equal(want[f].view(np.uint64), ref.view(np.uint64)), f
        assert np.array_equal(np.ascontiguousarray(getattr(sl, f), dtype=np.float64).view(np.uint64), ref.view(np.uint64)), f
    assert want["baseline"] == c["baseline"] == sl.getBaseline() and c["baseline"] != c["plain_baseline"]      # the reference's quirk
    assert G.make_rig(ss, c["rig"]).getBaseline() == c["plain_baseline"]
    assert np.array_equal(sl._geometry().view(np.uint64), want["geom"].view(np.uint64)) and sl._geometry()[67] == c["baseline"]
    cam, proj = P.correspondences(c["rig"], c["n"], c["seed"])
    pts = P.triangulate(want["geom"], cam, proj)
    ref = ARRAYS["rig_%s__points" % name]
    assert pts.shape == ref.shape == (c["n"], 1, 3)
    err = float(C.rel_err(pts, ref.astype(np.longdouble)).max())
    print("%s: restatement against the reference's points %.3e (tolerance %.3e)" % (name, err, c["tol"]))
    assert err <= c["tol"]
    assert c["tol"] == META["tol_factor"] * max(c["numpy_err"], META["floor"]) and "reference's points" in c["numpy_err_of"]


def test_recorded_tolerances_follow_their_rule():
    for name, c in META["decode"].items():
        assert c["tol"] == META["tol_factor"] * max(c["numpy_err"], max(PROJ) * META["floor"]) and c["worst_tie"] <= META["tie_max"] == 0.25, name
    for name, c in META["cloud"].items():
        assert c["tol"] == META["tol_factor"] * max(c["numpy_err"], META["floor"]) and c["worst_tie"] <= 0.25, name
    assert sorted(META["rigs"]) == ["d12", "d5", "d8", "none", "t2_zero"] and META["rigs"]["t2_zero"]["rig"]["T"][2] == 0


# ------------------------------------------------------------------------------------------------ the Python side
def test_rig_constructor_classmethod_and_export(ss, tmp_path):
    assert "StructuredLightRig" in ss.__all__ and issubclass(ss.StructuredLightRig, ss.StereoRig)
    r = META["rigs"]["d5"]["rig"]
    for bad in (r, None, 5, "rig.json"):
        with pytest.raises(ValueError, match=re.escape(META["bad_rig"]["message"])):
            ss.StructuredLightRig(bad)
    assert META["bad_rig"]["message"] == "Invalid argument!"
    path = str(tmp_path / "rig.json")
    G.make_rig(ss, r).save(path)
    sl = ss.StructuredLightRig.fromFile(path)
    assert isinstance(sl, ss.StructuredLightRig) and np.array_equal(sl.R1, ARRAYS["rig_d5__R1"]) and sl.res2 == tuple(r["res2"])
    again = ss.StructuredLightRig(sl)                                # a StructuredLightRig is a StereoRig: its R is the common one now
    assert again.R_inv.shape == (4, 4)


def test_exceptions_are_raised_before_any_native_call(ss, monkeypatch):
    a = ss.active
    assert {"phaseShiftPattern", "phaseShiftDecode", "PhaseShift", "MAX_PERIODS"} <= set(a.__all__) and a.MAX_PERIODS == 8
    for text in ("``StereoFTPAnaglyph`` stays out", "ssamd_structured_light.h", "``phaseShiftDecode``", "calibration.py:656-687", "half-pixel"):
        assert text in a.__doc__, text

    def no_native(*args, **kw):
        raise AssertionError("a native call")
    monkeypatch.setattr(a._native, "lib", no_native)
    r = META["rigs"]["d5"]["rig"]
    rig = G.make_rig(ss, r)
    stack = P.scene(1, (67, 37), PROJ, PERIODS)
    assert stack.shape == (21, 37, 67)
    # periods: the limits are executed, 0 and 17 (and 9) on an axis
    seventeen = [64.0 / (i + 1) for i in range(17)]
    for bad in (([], [32.0]), ([64.0], []), (seventeen, [32.0]), ([64.0], seventeen[:9]), ([64.0],), ([64.0], [32.0], [1.0]), 7, None, (64.0, 32.0),
                ([64.0, 0.0], [32.0]), ([64.0], [-32.0]), ([np.inf], [32.0]), ([64.0], [np.nan]), (["64"], [32.0]), ([True], [32.0])):
        with pytest.raises(ValueError):
            a.phaseShiftPattern(bad, PROJ)
        with pytest.raises(ValueError):
            a.phaseShiftDecode(stack, bad, PROJ)
        with pytest.raises(ValueError):
            a.PhaseShift(rig, bad)
    assert a.phaseShiftPattern((seventeen[:8], seventeen[:8]), (5, 3)).shape == (64, 3, 5)
    # resolutions
    for bad in ((0, 5), (5, 65537), (5,), (5.0, 3), 7):
        with pytest.raises(ValueError):
            a.phaseShiftPattern(PERIODS, bad)
        with pytest.raises(ValueError):
            a.phaseShiftDecode(stack, PERIODS, bad)
    with pytest.raises(ValueError):
        a.PhaseShift(G.make_rig(ss, dict(r, res2=[65537, 6])), PERIODS)
    # images
    ps = a.PhaseShift(rig, PERIODS)
    for bad in (stack.astype(np.float32), [stack[0].astype(np.uint16)], "name.png", 5):
        with pytest.raises(TypeError):
            a.phaseShiftDecode(bad, PERIODS, PROJ)
        with pytest.raises(TypeError):
            ps.getCloud(bad)
    for bad in (stack[0], stack[None], [stack[0], stack[1][:, :-1]]):
        with pytest.raises(ValueError):
            a.phaseShiftDecode(bad, PERIODS, PROJ)
    with pytest.raises(ValueError, match="need 20 images, got 19"):
        a.phaseShiftDecode(stack[:19], PERIODS, PROJ)
    with pytest.raises(ValueError, match="need 20 images, got 2"):
        ps.getCloud(list(stack[:2]))
    with pytest.raises(ValueError, match="Image size of 0 is mismatch!"):
        ps.getCloud(stack[:, :-1])
    # min_modulation
    for bad in (-1, -0.5, "5", True, np.nan, [1]):
        with pytest.raises(ValueError, match="min_modulation"):
            a.phaseShiftDecode(stack, PERIODS, PROJ, min_modulation=bad)
        with pytest.raises(ValueError, match="min_modulation"):
            a.PhaseShift(rig, PERIODS, min_modulation=bad)
    assert [a._mod_thr2(m) for m in (None, 0, 0.5, 1.5, 50, 1e200, np.inf)] == [0, 0, 1, 9, 10000, 130051, 130051]
    assert [P.mod_thr2(m) for m in (None, 0, 0.5, 1.5, 50, 1e200)] == [0, 0, 1, 9, 10000, 130051]
    # maps
    m = np.zeros((37, 67), np.float32)
    for bad in (m, (m,), (m, m[:-1])):
        with pytest.raises(ValueError):
            a.phaseShiftDecode(stack, PERIODS, PROJ, maps=bad)
    for bad in ((m, m.astype(np.float64)), (m, None)):
        with pytest.raises(TypeError):
            a.phaseShiftDecode(stack, PERIODS, PROJ, maps=bad)
    # roi: (x, y, width, height)
    for bad in ((0, 0, 68, 37), (1, 0, 67, 37), (0, 30, 5, 8), (-1, 0, 5, 5), (0, 0, -5, 5), (0, 0, 5), (0, 0, 5.5, 5), (0, 0, True, 5), 7):
        with pytest.raises(ValueError):
            a.phaseShiftDecode(stack, PERIODS, PROJ, roi=bad)
        with pytest.raises(ValueError):
            ps.getCloud(stack, roi=bad)
    # the rig
    for bad in (r, None):
        with pytest.raises(ValueError, match="Invalid argument!"):
            a.PhaseShift(bad, PERIODS)
    with pytest.raises(NotImplementedError):
        a.PhaseShift(G.make_rig(ss, dict(r, distCoeffs2=[0.0] * 12 + [0.01, 0.0])), PERIODS).getCloud(stack)
    with pytest.raises(ValueError, match="not finite"):
        a.PhaseShift(G.make_rig(ss, dict(r, distCoeffs2=[np.inf, 0, 0, 0, 0])), PERIODS).getCloud(stack)
    # empty regions and no points need no device
    assert ps.getCloud(stack, roi=(3, 5, 0, 4)).shape == (4, 0, 3) and a.phaseShiftDecode(stack, PERIODS, PROJ, roi=(0, 0, 5, 0)).shape == (0, 5, 2)
    assert isinstance(ps.rig, ss.StructuredLightRig) and a.PhaseShift(ps.rig, PERIODS).rig is ps.rig
    # StructuredLightRig.triangulate
    sl = ps.rig
    pts = np.zeros((6, 2))
    out = sl.triangulate(pts[:0], pts[:0].astype(np.float32))
    assert out.shape == (0, 1, 3) and out.dtype == np.float64
    for cam, proj in ((np.zeros((6, 3)), pts), (pts, np.zeros((4, 3))), (pts, pts[:5]), (np.zeros((3, 4, 2)), pts), (np.zeros(()), pts)):
        with pytest.raises(ValueError):
            sl.triangulate(cam, proj)
    for cam, proj in ((pts.tolist(), pts), (pts, None), (pts.astype(np.complex128), pts), (pts, pts.astype(bool))):
        with pytest.raises(TypeError):
            sl.triangulate(cam, proj)
    with pytest.raises(NotImplementedError):
        ss.StructuredLightRig(G.make_rig(ss, dict(r, distCoeffs2=[0.0] * 12 + [0.01, 0.0]))).triangulate(pts, pts)
    with pytest.raises(ValueError, match="not finite"):
        ss.StructuredLightRig(G.make_rig(ss, dict(r, distCoeffs2=[np.nan, 0, 0, 0, 0]))).triangulate(pts, pts)


def test_undistort_camera_image_on_the_host_is_the_remap_of_stereo_ftp(ss):
    import _stereo_ftp_ref as S
    r = META["rigs"]["d12"]["rig"]
    sl = ss.StructuredLightRig(G.make_rig(ss, r))
    rng = np.random.default_rng(5)
    gray, bgr = rng.integers(0, 256, (37, 67), dtype=np.uint8), rng.integers(0, 256, (37, 67, 3), dtype=np.uint8)
    mx, my = S.undistort_maps(np.array(r["intrinsic1"]), r["distCoeffs1"], tuple(r["res1"]))
    assert np.array_equal(sl.undistortCameraImage(gray), G.remap_stack(gray[None], mx, my)[0])
    assert np.array_equal(sl.undistortCameraImage(bgr), S.remap_linear(bgr, mx, my))
    assert not np.array_equal(sl.undistortCameraImage(gray), gray)
