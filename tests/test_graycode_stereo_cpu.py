"""CPU tier of two-camera Gray code (ss.active.GrayCodeStereo, grayCodeMatch, stereoTriangulate): the sixth public header
include/ssamd_graycode_stereo.h against its ctypes rows (the five older headers unchanged), its argument errors without a device,
the Python exception table, and the numpy restatement tests/_graycode_stereo_ref.py -- its `last` table against the literal
double loop, its triangulation against the points the reference's own StructuredLightRig recorded
(tests/golden/phaseshift_cases.*, rig `none`, where undistortPoints is the identity up to rounding).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _ftp_cloud_ref as C
import _graycode_ref as G
import _graycode_stereo_ref as S
import _phaseshift_ref as P
from test_native_signatures_cpu import SCALARS, _is_pointer_class, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
META, ARRAYS = P.load()


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


# ------------------------------------------------------------------------------------------------ the sixth header
NAMES = ["ssamd_graycode_stereo_cloud", "ssamd_graycode_stereo_cloud_device", "ssamd_graycode_stereo_match", "ssamd_graycode_stereo_match_device",
         "ssamd_graycode_stereo_points", "ssamd_stereo_triangulate", "ssamd_stereo_triangulate_device"]


def test_header_parses_and_matches_its_ctypes_rows():
    from simplestereo_amd import _native
    with open(os.path.join(ROOT, "include", "ssamd_graycode_stereo.h")) as f:
        header = f.read()
    protos = _prototypes(header)
    assert sorted(protos) == NAMES
    assert set(protos) == set(re.findall(r"\b(ssamd_[a-z0-9_]+)\s*\(", header))
    assert int(re.search(r"#define SSAMD_GRAYCODE_STEREO_VERSION (\d+)", header).group(1)) == _native.GRAYCODE_STEREO_VERSION == 1
    assert int(re.search(r"#define SSAMD_STEREO_LAST (\d+)", header).group(1)) == _native.STEREO_LAST == 0
    assert int(re.search(r"#define SSAMD_STEREO_MEAN (\d+)", header).group(1)) == _native.STEREO_MEAN == 1
    side = ["ptr"] + ["int"] * 4
    assert protos["ssamd_graycode_stereo_match"] == ("int", side + side + ["int"] * 3 + ["ptr", "ptr", "int"])
    assert protos["ssamd_graycode_stereo_match_device"][1] == protos["ssamd_graycode_stereo_match"][1][:-1] + ["ptr", "ptr"]      # scratch, stream
    assert protos["ssamd_graycode_stereo_cloud"] == ("int", ["ptr", "int", "int", "ptr", "ptr", "ptr", "int"])
    assert protos["ssamd_graycode_stereo_cloud_device"][1] == protos["ssamd_graycode_stereo_cloud"][1][:-1] + ["ptr"]
    assert protos["ssamd_stereo_triangulate"] == ("int", ["ptr", "ptr", "long long", "ptr", "ptr", "int"])
    assert protos["ssamd_stereo_triangulate_device"][1] == protos["ssamd_stereo_triangulate"][1][:-1] + ["ptr"]
    stack = ["ptr", "int", "int", "ptr", "ptr"] + ["int"] * 4
    assert protos["ssamd_graycode_stereo_points"] == ("int", stack + stack + ["int"] * 7 + ["ptr", "int", "ptr", "ptr", "int"])
    lib = _native.lib()
    for name, (ret, kinds) in protos.items():
        fn = getattr(lib, name)                                                 # exported from the same library
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(fn.argtypes, kinds)):
            assert _is_pointer_class(t) if kind == "ptr" else t is SCALARS[kind], (name, i, t, kind)


def test_the_older_headers_are_as_they_were():
    from simplestereo_amd import _native
    for name, count in (("ssamd.h", 54), ("ssamd_active.h", 4), ("ssamd_graycode.h", 6), ("ssamd_ftp_mapping.h", 4), ("ssamd_structured_light.h", 4)):
        with open(os.path.join(ROOT, "include", name)) as f:
            header = f.read()
        assert "graycode_stereo" not in header.lower() and "stereo_triangulate" not in header.lower(), name
        assert len(_prototypes(header)) == count, name
    assert (_native.ABI_VERSION, _native.ACTIVE_VERSION, _native.GRAYCODE_VERSION, _native.FTP_MAPPING_VERSION, _native.SL_VERSION, _native.K_COUNT) == (8, 1, 1, 1, 1, 12)
    assert _native.lib().ssamd_abi_version() == 8


def test_abi_argument_errors_need_no_device():
    """SSAMD_EINVAL for what include/ssamd_graycode_stereo.h lists, decided before any device is looked for"""
    from simplestereo_amd import _native
    lib = _native.lib()
    dp = ctypes.POINTER(ctypes.c_double)
    dec = np.zeros((4, 8, 2), np.int32)
    matches = np.zeros((6, 13, 4), np.float64)
    counts = np.zeros((1,), np.int32)
    scratch = np.zeros((2 * 20 * 78 // 8 + 2,), np.int64)

    def match(d1=dec.ctypes.data, h1=4, w1=8, x1=0, y1=0, d2=dec.ctypes.data, h2=4, w2=8, x2=0, y2=0, pw=13, ph=6, reduce=0,
              out=matches.ctypes.data, counts=counts.ctypes.data, scratch=scratch.ctypes.data, device=False):
        args = (d1, h1, w1, x1, y1, d2, h2, w2, x2, y2, pw, ph, reduce, out, counts)
        return lib.ssamd_graycode_stereo_match_device(*args, scratch, None) if device else lib.ssamd_graycode_stereo_match(*args, -1)

    bad = [dict(d1=None), dict(d2=None), dict(out=None), dict(h1=-1), dict(w2=-1), dict(x1=-1), dict(y2=-1), dict(pw=0), dict(ph=0), dict(pw=65537),
           dict(pw=65536, ph=32768), dict(reduce=2), dict(reduce=-1), dict(h1=65536, w1=32768), dict(x2=1 << 30, y2=4), dict(h2=46341, w2=46341)]
    for kw in bad:
        for device in (False, True):
            assert match(device=device, **kw) == _native.EINVAL, (kw, device)
            assert lib.ssamd_last_error()
    assert match(scratch=None, device=True) == _native.EINVAL
    assert match(out=matches.ctypes.data + 8, device=True) == _native.EINVAL and match(d1=dec.ctypes.data + 8, device=True) == _native.EINVAL
    assert match(scratch=scratch.ctypes.data + 4, device=True) == _native.EINVAL

    geom = np.ones(68)
    out = np.zeros((6, 13, 3), np.float64)
    offsets = np.zeros((2,), np.int32)

    def cloud(m=matches.ctypes.data, pw=13, ph=6, geom=geom, offsets=None, out=out.ctypes.data, device=False):
        args = (m, pw, ph, None if geom is None else geom.ctypes.data_as(dp), offsets, out)
        return lib.ssamd_graycode_stereo_cloud_device(*args, None) if device else lib.ssamd_graycode_stereo_cloud(*args, -1)

    pts = np.zeros((5, 2))

    def tri(p1=pts.ctypes.data, p2=pts.ctypes.data, n=5, geom=geom, out=out.ctypes.data, device=False):
        args = (p1, p2, n, None if geom is None else geom.ctypes.data_as(dp), out)
        return lib.ssamd_stereo_triangulate_device(*args, None) if device else lib.ssamd_stereo_triangulate(*args, -1)

    bad_geom = []
    for i in (40, 49, 58, 66, 67):
        g = geom.copy()
        g[i] = np.nan if i % 2 else np.inf
        bad_geom.append(dict(geom=g))
    for kw in [dict(m=None), dict(out=None), dict(geom=None), dict(pw=0), dict(ph=65537), dict(pw=65536, ph=32768)] + bad_geom:
        for device in (False, True):
            assert cloud(device=device, **kw) == _native.EINVAL, (kw, device)
    bad_total = np.array([0, 79], np.int32)                                              # more points than cells (host form reads it)
    assert cloud(offsets=bad_total.ctypes.data) == _native.EINVAL
    assert cloud(m=matches.ctypes.data + 8, device=True) == _native.EINVAL and cloud(out=out.ctypes.data + 4, device=True) == _native.EINVAL
    assert cloud(offsets=offsets.ctypes.data + 2, device=True) == _native.EINVAL
    for kw in [dict(p1=None), dict(p2=None), dict(out=None), dict(geom=None), dict(n=-1), dict(n=(1 << 38) + 1)] + bad_geom:
        for device in (False, True):
            assert tri(device=device, **kw) == _native.EINVAL, (kw, device)
    assert tri(p1=pts.ctypes.data + 4, device=True) == _native.EINVAL and tri(out=out.ctypes.data + 4, device=True) == _native.EINVAL
    assert tri(n=0) == 0 and tri(n=0, p1=None, p2=None, out=None, device=True) == 0      # no point: nothing is done
    for i in (0, 12, 27, 36, 39):                                                        # entries this triangulation does not read
        g = geom.copy()
        g[i] = np.nan
        assert tri(n=0, geom=g) == 0

    planes = np.zeros((14, 4, 8), np.uint8)
    n = ctypes.c_int(7)

    def points(p1=planes.ctypes.data, p2=planes.ctypes.data, hc=4, wc=8, h1=4, w2=8, nimg=14, ncol=4, nrow=3, pw=13, ph=6, thr=5, reduce=1, geom=geom,
               out=out.ctypes.data, npoints=ctypes.byref(n)):
        return lib.ssamd_graycode_stereo_points(p1, hc, wc, None, None, 0, 0, h1, 8, p2, hc, wc, None, None, 0, 0, 4, w2, nimg, ncol, nrow, pw, ph, thr,
                                                reduce, None if geom is None else geom.ctypes.data_as(dp), 0, out, npoints, -1)

    for kw in [dict(p1=None), dict(p2=None), dict(h1=5), dict(w2=9), dict(nimg=12), dict(ncol=17, nimg=40), dict(pw=0), dict(thr=257), dict(reduce=3),
               dict(geom=None), dict(out=None), dict(npoints=None)] + bad_geom:
        assert points(**kw) == _native.EINVAL, kw


# ------------------------------------------------------------------------------------------------ the restatement
def test_last_table_is_the_literal_double_loop():
    """np.maximum.at on the raster key against the reference's loop with the indices the right way round: 67 x 37 / 13 x 6"""
    proj = (13, 6)
    stack = G.random_stack(3, G.num_patterns(*proj), 37, 67)
    dec = G.decode(stack, proj[0], proj[1], 5)
    valid = float((dec[..., 0] >= 0).mean())
    assert 0.2 < valid < 0.8
    for origin in ((0, 0), (5, 9)):
        want = S.table_last_literal(dec, origin, proj)
        assert np.array_equal(S.table_last(dec, origin, proj), want)
        assert (want[..., 0] >= 0).all() and want[..., 1].max() == 36 + origin[1]        # 2479 pixels on 78 cells: every cell is hit
    # a sparse map: cells nobody decodes to stay (-1, -1); a value outside the projector contributes nothing
    sparse = np.full((37, 67, 2), -1, np.int32)
    sparse[3, 5] = (2, 1); sparse[30, 1] = (2, 1); sparse[30, 0] = (12, 5); sparse[7, 7] = (13, 0); sparse[8, 8] = (0, 6)
    t = S.table_last(sparse, (0, 0), proj)
    assert np.array_equal(t, S.table_last_literal(sparse, (0, 0), proj))
    assert tuple(t[1, 2]) == (1, 30) and tuple(t[5, 12]) == (0, 30) and int((t[..., 0] >= 0).sum()) == 2
    sx, sy, n = S.table_mean(sparse, (4, 2), proj)
    assert (int(sx[1, 2]), int(sy[1, 2]), int(n[1, 2])) == (5 + 1 + 8, 3 + 30 + 4, 2) and int(n.sum()) == 3
    m = S.match(sparse, sparse, proj, "mean", (4, 2), (0, 0))
    assert np.array_equal(m[1, 2], [7.5, 19.0, 3.5, 17.0]) and int(np.isnan(m[..., 0]).sum()) == 76


def test_triangulation_against_the_references_recorded_points():
    """The two-camera triangulation on the seeded correspondences of rig `none` against the reference's own
    StructuredLightRig.triangulate (rig_none__points): without distortion its undistortPoints is the identity up to the rounding
    of a normalise / denormalise, which the fixture's tolerance (16 x the reference's own error) covers."""
    c = META["rigs"]["none"]
    assert not any(c["rig"]["distCoeffs2"] or [0.0])
    g = P.sl_rig(c["rig"])["geom"]
    cam, proj = P.correspondences(c["rig"], c["n"], c["seed"])
    pts = S.triangulate(g, cam, proj)
    ref = ARRAYS["rig_none__points"]
    assert pts.shape == ref.shape == (c["n"], 1, 3)
    err = float(C.rel_err(pts, ref.astype(np.longdouble)).max())
    print("two-camera restatement against the reference's points: %.3e (tolerance %.3e)" % (err, c["tol"]))
    assert err <= c["tol"]
    # (profiles/graycode_stereo_parity.txt records the measured distance)
    # three NaN where a couple holds a NaN; zero disparity is inf / NaN, not an exception
    holes = proj.copy()
    holes[3, 1] = np.nan
    out = S.triangulate(g, cam, holes)
    assert np.isnan(out[3]).all() and G.same_points(np.delete(out, 3, axis=0), np.delete(pts, 3, axis=0))
    eye = np.zeros(68)
    eye[40:49] = eye[49:58] = eye[58:67] = np.eye(3).ravel()
    eye[67] = 1.0
    assert not np.isfinite(S.triangulate(eye, [[1.0, 2.0]], [[1.0, 5.0]])).any()


def test_cloud_of_a_match_is_compacted_in_projector_raster_order():
    g = S.geometry(S.two_camera_rig((67, 37), (53, 41)))
    assert not g[:40].any() and np.isfinite(g[40:]).all()
    rng = np.random.default_rng(2)
    m = rng.uniform(1, 30, (6, 13, 4))
    m[rng.random((6, 13)) < 0.4] = np.nan
    dense, compact = S.cloud(g, m, dense=True), S.cloud(g, m)
    keep = ~np.isnan(m[..., 0])
    assert dense.shape == (6, 13, 3) and compact.shape == (int(keep.sum()), 1, 3) and 0 < keep.sum() < 78
    assert G.same_points(compact, dense[keep].reshape(-1, 1, 3)) and np.isnan(dense[~keep]).all()


# ------------------------------------------------------------------------------------------------ the Python side
def test_names_and_docstring(ss):
    a = ss.active
    assert hasattr(a, "GrayCodeStereo") and "GrayCodeDouble" in a.__doc__ and not hasattr(a, "GrayCodeDouble")
    assert {"GrayCodeStereo", "grayCodeMatch", "stereoTriangulate"} <= set(a.__all__)
    for text in ("``GrayCodeStereo``", "ssamd_graycode_stereo.h", "active.py:1463-1608", "active.py:1594-1606", "``GrayCodeDouble`` stays out",
                 "``StereoFTPAnaglyph`` stays out"):
        assert text in a.__doc__, text
    assert "zero disparity" in a.GrayCodeStereo.getCloud.__doc__ and "undistortPoints" in a.stereoTriangulate.__doc__


def test_exceptions_are_raised_before_any_native_call(ss, monkeypatch, tmp_path):
    a = ss.active

    def no_native(*args, **kw):
        raise AssertionError("a native call")
    monkeypatch.setattr(a._native, "lib", no_native)
    proj = (13, 6)
    r = S.two_camera_rig((67, 37), (53, 41))
    rig = G.make_rig(ss, r)
    n = G.num_patterns(*proj)
    s1, s2 = G.random_stack(1, n + 1, 37, 67), G.random_stack(2, n, 41, 53)
    # the constructor
    gs = a.GrayCodeStereo(rig, proj)
    assert gs.rig is rig and gs.projRes == proj and gs.num_patterns == n == 14 and gs.reduce == "last"
    assert gs.Rectify1.shape == gs.Rectify2.shape == (3, 3) and gs.R_inv.shape == (4, 4)
    want = S.geometry(r)
    assert np.array_equal(gs._geometry().view(np.uint64), want.view(np.uint64))
    for bad in (r, None, 5):
        with pytest.raises(ValueError, match="Invalid argument!"):
            a.GrayCodeStereo(bad, proj)
        with pytest.raises(ValueError, match="Invalid argument!"):
            a.stereoTriangulate(bad, np.zeros((3, 2)), np.zeros((3, 2)))
    for bad in ((0, 5), (5, 65537), (5,), (5.0, 3), 7, (65536, 32768), (65536, 65536)):
        with pytest.raises(ValueError):
            a.GrayCodeStereo(rig, bad)
        with pytest.raises(ValueError):
            a.grayCodeMatch(np.zeros((2, 2, 2), np.int32), np.zeros((2, 2, 2), np.int32), bad)
    assert a.GrayCodeStereo(rig, (65536, 32767)).num_patterns == 62
    for bad in ("first", None, 0, "LAST"):
        with pytest.raises(ValueError, match="reduce"):
            a.GrayCodeStereo(rig, proj, reduce=bad)
        with pytest.raises(ValueError, match="reduce"):
            a.grayCodeMatch(np.zeros((2, 2, 2), np.int32), np.zeros((2, 2, 2), np.int32), proj, reduce=bad)
    for bad in (-1, 257, 5.0, True):
        with pytest.raises(ValueError, match="white_thr"):
            a.GrayCodeStereo(rig, proj, white_thr=bad)
    # images
    for bad in (s1, 5, "name.png", [], (s1,), (s1, s2, s2), [("a.png",), ("b.png",)]):
        with pytest.raises(TypeError):
            gs.getCloud(bad)
    for bad in ((s1.astype(np.float32), s2), (s1, [s2[0].astype(np.uint16)]), (s1, "name.png")):
        with pytest.raises(TypeError):
            gs.getCloud(bad)
    for bad in ((s1[0], s2), (s1, s2[None])):
        with pytest.raises(ValueError):
            gs.getCloud(bad)
    with pytest.raises(ValueError, match="needs 14 pattern images, got 13"):
        gs.getCloud((s1, s2[:13]))
    with pytest.raises(ValueError, match="Image size of 0 is mismatch!"):
        gs.getCloud((s1[:, :-1], s2))
    with pytest.raises(ValueError, match="Image size of 0 is mismatch!"):
        gs.getCloud((s1, s1))                                                # camera 2's stack must be of res2
    with pytest.raises(ValueError, match="Image size of 3 is mismatch!"):
        gs.getCloud((s1, list(s2[:3]) + [s2[3][:, :-1]] + list(s2[4:])))
    # files: the reference's list of couples
    from PIL import Image
    couples = []
    for i in range(n):
        couples.append((str(tmp_path / ("%dL.png" % i)), str(tmp_path / ("%dR.png" % i))))
        Image.fromarray(s1[i]).save(couples[-1][0])
        Image.fromarray(s2[i] if i != 5 else s2[i][:-1]).save(couples[-1][1])
    with pytest.raises(ValueError, match=re.escape("Image size of %s is mismatch!" % couples[5][1])):
        gs.getCloud(couples)
    Image.fromarray(np.zeros((41, 53, 3), np.uint8)).save(couples[5][1])
    with pytest.raises(ValueError, match="not an 8-bit single-channel image"):
        gs.getCloud(couples)
    # roi1 / roi2: (x, y, x_end, y_end)
    for bad in ((0, 0, 68, 37), (-1, 0, 5, 5), (0, 0, 5), (0, 0, 5.5, 5), 7):
        with pytest.raises(ValueError):
            gs.getCloud((s1, s2), roi1=bad)
    for bad in ((0, 0, 54, 41), (0, 0, 53, 42), (0, -1, 5, 5)):
        with pytest.raises(ValueError):
            gs.getCloud((s1, s2), roi2=bad)
    # an empty roi of either camera: no projector pixel is seen by both, and no device is needed
    for kw in (dict(roi1=(3, 5, 3, 9)), dict(roi2=(0, 7, 9, 7)), dict(roi1=(9, 9, 2, 2), roi2=(1, 1, 1, 1))):
        out = gs.getCloud((s1, s2), **kw)
        assert out.shape == (0, 1, 3) and out.dtype == np.float64
        out = gs.getCloud((s1, s2), dense=True, **kw)
        assert out.shape == (6, 13, 3) and np.isnan(out).all()
    # a rig whose geometry is not finite
    with pytest.raises(ValueError, match="not finite"):
        a.GrayCodeStereo(G.make_rig(ss, dict(r, T=[np.inf, 0.0, 0.0])), proj).getCloud((s1, s2))
    # grayCodeMatch
    d1, d2 = np.zeros((37, 67, 2), np.int32), np.zeros((41, 53, 2), np.int32)
    for bad in (d1.astype(np.int64), d1.tolist(), None, d1.astype(np.float64)):
        with pytest.raises(TypeError):
            a.grayCodeMatch(bad, d2, proj)
        with pytest.raises(TypeError):
            a.grayCodeMatch(d1, bad, proj)
    for bad in (d1[0], d1[..., :1], np.zeros((37, 67, 3), np.int32), d1[None]):
        with pytest.raises(ValueError):
            a.grayCodeMatch(bad, d2, proj)
    for bad in ((-1, 0), (0,), (0.0, 0), 5, None, (True, 0)):
        with pytest.raises(ValueError, match="origin1"):
            a.grayCodeMatch(d1, d2, proj, origin1=bad)
        with pytest.raises(ValueError, match="origin2"):
            a.grayCodeMatch(d1, d2, proj, origin2=bad)
    with pytest.raises(ValueError, match="2\\^31"):
        a.grayCodeMatch(d1, d2, proj, origin2=(1 << 30, 0))
    # stereoTriangulate: the checks of StructuredLightRig.triangulate
    pts = np.zeros((6, 2))
    out = a.stereoTriangulate(rig, pts[:0], pts[:0].astype(np.float32))
    assert out.shape == (0, 1, 3) and out.dtype == np.float64
    for p1, p2 in ((np.zeros((6, 3)), pts), (pts, np.zeros((4, 3))), (pts, pts[:5]), (np.zeros((3, 4, 2)), pts), (np.zeros(()), pts)):
        with pytest.raises(ValueError):
            a.stereoTriangulate(rig, p1, p2)
    for p1, p2 in ((pts.tolist(), pts), (pts, None), (pts.astype(np.complex128), pts), (pts, pts.astype(bool))):
        with pytest.raises(TypeError):
            a.stereoTriangulate(rig, p1, p2)
    with pytest.raises(ValueError, match="not finite"):
        a.stereoTriangulate(G.make_rig(ss, dict(r, T=[np.nan, 0.0, 0.0])), pts, pts)
    assert a.stereoTriangulate(ss.StructuredLightRig(rig), pts[:0], pts[:0]).shape == (0, 1, 3)


def test_private_map_helpers_take_the_camera(ss):
    """_undistort_maps / _cached_maps(which=2): initUndistortRectifyMap(K2, D2, I, K2, res2), cached apart from camera 1's"""
    import _stereo_ftp_ref as F
    from simplestereo_amd import _rigs
    r = S.two_camera_rig((67, 37), (53, 41), dist1=C.DIST_MODELS["d5"], dist2=[0.11, -0.07, 0.002, -0.001, 0.02])
    rig = G.make_rig(ss, r)
    cache = {}
    m1, m2 = _rigs._cached_maps(cache, rig), _rigs._cached_maps(cache, rig, which=2)
    assert m1[0].shape == (37, 67) and m2[0].shape == (41, 53) and m2[0].dtype == np.float32
    for got, (K, d, res) in ((m1, (r["intrinsic1"], r["distCoeffs1"], r["res1"])), (m2, (r["intrinsic2"], r["distCoeffs2"], r["res2"]))):
        want = F.undistort_maps(np.array(K), d, tuple(res))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert _rigs._cached_maps(cache, rig, which=2) is m2 and _rigs._cached_maps(cache, rig) is m1
    assert np.array_equal(_rigs._undistort_maps(rig)[0], m1[0]) and np.array_equal(_rigs._undistort_maps(rig, 2)[1], m2[1])
