"""RectifiedStereoRig plumbing (reference _rigs.py:341-628), numpy-only restatement.
JSON layout is pinned by the reference's own example rig files (copied as DATA fixtures:
tests/golden/rig_example2_rigRect.json = examples/res/2/rigRect.json,
tests/golden/rig_example1_rig.json = examples/res/1/rig.json).  Pixel values of rectifyImages
cannot be pinned against OpenCV here (cv2 is absent): self-consistency checks instead."""
import json
import os

import numpy as np
import pytest

import simplestereo_amd as ss
from simplestereo_amd import _rigs

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RIGRECT = os.path.join(G, "rig_example2_rigRect.json")
RIG = os.path.join(G, "rig_example1_rig.json")


def test_stereo_rig_json_round_trip(tmp_path):
    rig = ss.StereoRig.fromFile(RIG)
    data = json.load(open(RIG))
    assert tuple(rig.res1) == tuple(data["res1"]) and rig.intrinsic1.shape == (3, 3) and rig.T.shape == (3, 1)
    out = tmp_path / "rig.json"
    rig.save(str(out))
    back = json.load(open(out))
    for k in ("res1", "res2", "intrinsic1", "intrinsic2", "R", "distCoeffs1", "distCoeffs2"):
        assert np.allclose(np.asarray(back[k], float).ravel(), np.asarray(data[k], float).ravel())
    assert np.allclose(np.asarray(back["T"], float).ravel(), np.asarray(data["T"], float).ravel())
    assert np.isclose(ss.StereoRig.fromFile(str(out)).getBaseline(), rig.getBaseline())


def test_rectified_rig_json_round_trip_and_ctor_forms(tmp_path):
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    data = json.load(open(RIGRECT))
    out = tmp_path / "rr.json"
    rig.save(str(out))
    back = json.load(open(out))
    assert set(back) == set(data)
    for k in data:
        assert np.allclose(np.asarray(back[k], float).ravel(), np.asarray(data[k], float).ravel()), k
    # second constructor form: (Rcommon, H1, H2, StereoRig)
    base = ss.StereoRig(rig.res1, rig.res2, rig.intrinsic1, rig.intrinsic2, rig.distCoeffs1, rig.distCoeffs2, rig.R, rig.T)
    rig2 = ss.RectifiedStereoRig(rig.Rcommon, rig.rectHomography1, rig.rectHomography2, base)
    assert np.allclose(rig2.K1, rig.K1) and np.allclose(rig2.mapx2, rig.mapx2)
    assert rig.mapx1.dtype == np.float32 and rig.mapx1.shape == (rig.res1[1], rig.res1[0])


def test_rectified_projections_share_rows():
    """after rectification a 3D point projects to the same image row in both cameras"""
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    P1, P2 = rig.getRectifiedProjectionMatrices()
    rng = np.random.default_rng(0)
    X = np.c_[rng.uniform(-500, 500, 50), rng.uniform(-300, 300, 50), rng.uniform(800, 3000, 50), np.ones(50)]
    a, b = X.dot(P1.T), X.dot(P2.T)
    y1, y2 = a[:, 1] / a[:, 2], b[:, 1] / b[:, 2]
    # the example rig comes from a real calibration: its homographies rectify to ~0.1 px
    assert np.abs(y1 - y2).max() < 0.25
    x1, x2 = a[:, 0] / a[:, 2], b[:, 0] / b[:, 2]
    assert np.all((x1 - x2) * np.sign((x1 - x2)[0]) > 0)        # one-signed disparity


def test_maps_agree_with_forward_camera_model():
    """mapx/mapy (initUndistortRectifyMap restatement) == forward projection of the rectified ray
    through rotation, distortion and intrinsics; undistortPoints inverts the distortion model"""
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    h, w = rig.mapx1.shape
    for (K, dist, Rr, Knew, mx, my) in ((rig.intrinsic1, rig.distCoeffs1, rig.Rcommon, rig.K1, rig.mapx1, rig.mapy1),
                                        (rig.intrinsic2, rig.distCoeffs2, rig.Rcommon.dot(rig.R.T), rig.K2, rig.mapx2, rig.mapy2)):
        for (u, v) in ((10, 20), (w // 2, h // 2), (w - 7, h - 3)):
            ray = np.linalg.inv(Knew.dot(Rr)).dot([u, v, 1.0])
            x, y = ray[0] / ray[2], ray[1] / ray[2]
            xd, yd = _rigs._distort(np.array([x]), np.array([y]), _rigs._dist_vector(dist))
            assert np.isclose(K[0, 0] * xd[0] + K[0, 2], mx[v, u], atol=1e-2)
            assert np.isclose(K[1, 1] * yd[0] + K[1, 2], my[v, u], atol=1e-2)
            back = _rigs._undistort_points([[mx[v, u], my[v, u]]], K, dist)
            assert np.allclose(back[0], [x, y], atol=1e-5)


def test_remap_bilinear_on_linear_ramp_and_borders():
    ys, xs = np.mgrid[0:40, 0:60]
    img = (2 * xs + 3 * ys).astype(np.float32)
    mapx = (xs * 0.5 + 3.25).astype(np.float32)
    mapy = (ys * 0.75 + 1.5).astype(np.float32)
    out = _rigs._remap(img, mapx, mapy)
    inside = (mapx < 59) & (mapy < 39)
    assert np.allclose(out[inside], (2 * mapx + 3 * mapy)[inside], atol=1e-3)      # bilinear is exact on ramps
    u8 = np.clip(img, 0, 255).astype(np.uint8)
    far = _rigs._remap(np.dstack([u8] * 3), mapx + 1000, mapy)
    assert far.shape == (40, 60, 3) and far.dtype == np.uint8 and not far.any()    # constant border
    assert far.flags["C_CONTIGUOUS"]
    near = _rigs._remap(u8, np.rint(mapx), np.rint(mapy), interpolation=0)
    assert near[5, 7] == u8[int(np.rint(mapy[5, 7])), int(np.rint(mapx[5, 7]))]


def test_remap_uint8_ties_round_up_like_opencv_fixed_point():
    """cv2.remap's 8-bit bilinear path ends in FixedPtCast: (sum + (1 << 14)) >> 15 with integer weights summing to
    32768 (imgwarp.cpp), so a tie rounds UP: fx = 16/32 between pixels 2 and 3 gives 3 (half-to-even would give 2).
    Host numpy path and the per-pixel oracle restatement must agree on every tie."""
    from oracle import rig_oracle
    img = np.zeros((4, 6, 3), np.uint8)
    img[:, :, 0] = [0, 2, 3, 7, 8, 255]
    img[:, :, 1] = np.arange(6)[None, :] * 40
    img[:, :, 2] = 255 - img[:, :, 0]
    img[2:] //= 2
    mapx = np.array([[1.5, 2.5, 3.5, 0.5, 4.5, 5.5, -0.5]], np.float32)
    mapy = np.zeros_like(mapx)
    out = _rigs._remap(img, mapx, mapy)
    assert out[0, 0, 0] == 3            # (2 + 3) / 2 = 2.5 -> 3
    assert out[0, 1, 0] == 5            # (3 + 7) / 2 = 5
    assert out[0, 2, 0] == 8            # (7 + 8) / 2 = 7.5 -> 8
    assert out[0, 3, 0] == 1            # (0 + 2) / 2 = 1
    assert out[0, 4, 0] == 132          # (8 + 255) / 2 = 131.5 -> 132
    assert out[0, 5, 0] == 128          # (255 + border 0) / 2 = 127.5 -> 128
    assert out[0, 6, 0] == 0            # (border 0 + 0) / 2
    assert np.array_equal(out, rig_oracle.remap_bilinear(img, mapx, mapy))
    # every 1/32 fraction in both directions, including all quarter-way ties
    fy, fx = np.mgrid[0:32, 0:32]
    mx = (1 + fx / 32.0).astype(np.float32)
    my = (1 + fy / 32.0).astype(np.float32)
    got = _rigs._remap(img, mx, my)
    assert np.array_equal(got, rig_oracle.remap_bilinear(img, mx, my))
    a, b, c, d = (int(img[1, 1, 0]), int(img[1, 2, 0]), int(img[2, 1, 0]), int(img[2, 2, 0]))
    want = ((32 - fy) * (32 - fx) * a + (32 - fy) * fx * b + fy * (32 - fx) * c + fy * fx * d + 512) >> 10
    assert np.array_equal(got[:, :, 0], want)


def test_undistort_points_follows_opencv_default_iteration_count():
    """cv2.undistortPoints stops after 5 fixed-point iterations by default; the corner positions that feed the
    fitting matrix (reference rectification.py:125-156) are those of the 5th iterate"""
    K = np.array([[800.0, 0, 320], [0, 800, 240], [0, 0, 1]])
    dist = np.array([-0.3, 0.12, 0.001, -0.002, 0.0])
    pts = np.array([[0.0, 0.0], [639, 0], [639, 479], [0, 479]])
    five = _rigs._undistort_points(pts, K, dist)
    assert np.array_equal(five, _rigs._undistort_points(pts, K, dist, iterations=5))
    conv = _rigs._undistort_points(pts, K, dist, iterations=200)
    assert not np.array_equal(five, conv)                    # the default is not the converged solution ...
    assert np.abs(five - conv).max() < 5e-3                  # ... but within 5e-3 (normalised units) of it here


def test_rectify_images_feeds_matcher_shapes():
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=(160, 90))
    w, h = rig.res1
    rng = np.random.default_rng(1)
    a = rng.integers(0, 255, (h, w, 3)).astype(np.uint8)
    r1, r2 = rig.rectifyImages(a, a[:, ::-1].copy())
    assert r1.shape == (90, 160, 3) and r2.shape == (90, 160, 3) and r1.dtype == np.uint8
    assert r1.flags["C_CONTIGUOUS"] and r2.flags["C_CONTIGUOUS"]


def test_get3dpoints_matches_q_algebra():
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=(64, 36))
    d = np.full((36, 64), 7, np.int16)
    pts = rig.get3DPoints(d)
    assert pts.shape == (36, 64, 3) and pts.dtype == np.float32
    Q = rig.getQ()
    v = Q.dot([10.0, 20.0, 7.0, 1.0])
    assert np.allclose(pts[20, 10], v[:3] / v[3], rtol=1e-5)
    ys, xs = np.mgrid[0:36, 0:64]
    allp = np.stack([xs, ys, np.full_like(xs, 7), np.ones_like(xs)], -1).astype(np.float64).dot(Q.T)
    assert np.allclose(pts, (allp[..., :3] / allp[..., 3:]).astype(np.float32), rtol=1e-5)


def test_ply_round_trip_and_reference_header(tmp_path):
    """points.exportPLY / importPLY (reference points.py:10-121): header lines and column order"""
    rng = np.random.default_rng(0)
    pts = rng.normal(size=(4, 5, 3))
    img = rng.integers(0, 255, (4, 5, 3)).astype(np.uint8)
    f = tmp_path / "c.ply"
    ss.points.exportPLY(pts, str(f), img, precision=4)
    lines = open(f).read().splitlines()
    assert lines[:3] == ["ply", "format ascii 1.0", "comment SimpleStereo point cloud export"]
    assert lines[3] == "comment Original array shape 4x5x3" and lines[4] == "element vertex 20"
    assert lines[5:11] == ["property double x", "property double y", "property double z",
                           "property uchar red", "property uchar green", "property uchar blue"]
    assert lines[11] == "end_header" and len(lines) == 12 + 20
    back = ss.points.importPLY(str(f))
    assert back.shape == (20, 3) and np.allclose(back, pts.reshape(-1, 3), atol=1e-4)
    rgb = ss.points.importPLY(str(f), 3, 4, 5)
    assert np.array_equal(rgb.astype(np.uint8), img.reshape(-1, 3)[:, ::-1])          # BGR stored as RGB
    g = tmp_path / "g.ply"
    ss.points.exportPLY(pts, str(g), img[..., 0].astype(np.int64))
    assert "property int intensity" in open(g).read()
    h = tmp_path / "h.ply"
    ss.points.exportPLY(pts, str(h))
    assert ss.points.importPLY(str(h)).shape == (20, 3)


@pytest.mark.parametrize("name,key,prec", [("ply_none_p6.ply", None, 6), ("ply_bgr_p4.ply", "bgr", 4),
                                           ("ply_gray_i64_p3.ply", "gray_i64", 3), ("ply_gray_u8_p6.ply", "gray_u8", 6),
                                           ("ply_gray_f32_p2.ply", "gray_f32", 2)])
def test_export_ply_equals_the_files_the_reference_writes(tmp_path, name, key, prec):
    """pinned: tests/golden/ply_*.ply were written by the unmodified reference exportPLY (points.py:10-80, via
    tests/golden/make_golden_ply.py) from the inputs in ply_cases.npz -- our writer must produce the same bytes
    (header, column order, int64-only `int intensity`, the `{:{p}f}` float field), and our reader the same values"""
    G = os.path.dirname(RIGRECT)
    z = np.load(os.path.join(G, "ply_cases.npz"))
    flat = z["pts"].reshape(-1, 3)
    img = None if key is None else z[key]
    out = tmp_path / name
    ss.points.exportPLY(flat, str(out), img, precision=prec)
    assert open(out, "rb").read() == open(os.path.join(G, name), "rb").read()
    back = ss.points.importPLY(os.path.join(G, name))
    assert back.shape == (12, 3) and np.allclose(back, flat, atol=0.5 * 10.0 ** -prec)
    if key == "bgr":
        rgb = ss.points.importPLY(os.path.join(G, name), 3, 4, 5)
        assert np.array_equal(rgb.astype(np.uint8), z["bgr"].reshape(-1, 3)[:, ::-1])


def test_import_ply_of_an_empty_cloud_has_the_reference_shape(tmp_path):
    f = tmp_path / "e.ply"
    ss.points.exportPLY(np.zeros((0, 3)), str(f))
    assert ss.points.importPLY(str(f)).shape == (0,)        # np.asarray([], dtype=float), reference points.py:121


def test_adimensional_points_geometry():
    d = np.full((6, 8), 2, np.int16)
    p = ss.points.getAdimensional3DPoints(d)
    assert p.shape == (6, 8, 3) and p.dtype == np.float32
    # centre pixel maps to x = y = 0; depth = -f*b/d with f = width, b = 1
    assert np.allclose(p[3, 4], [0.0, 0.0, -8 / 2.0])
    assert np.allclose(p[..., 2], -4.0)


# ---- the test references of oracle/rig_oracle.py themselves (what tests/test_gpu_rigs_limits.py holds the kernels to)
def _fp64_reproject(d, Q):
    """plain fp64 evaluation in the kernel's order of operations (no contraction), one division per component"""
    H, W = d.shape
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    v = [x, y, d.astype(np.float64), np.ones_like(x)]
    p = [Q[r, 0] * v[0] + Q[r, 1] * v[1] + Q[r, 2] * v[2] + Q[r, 3] for r in range(4)]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.stack([p[0] / p[3], p[1] / p[3], p[2] / p[3]], -1).astype(np.float32)


def test_reprojection_references_agree_and_bound_has_teeth():
    """exact rational and longdouble references agree; plain fp64 evaluation lies within the derived bound
    0.5 ulp32(t) + |t| 8 2^-53 (kX + kW); a value two float32 ulps away does not; W = 0 demands the class"""
    from oracle import rig_oracle
    rig = ss.RectifiedStereoRig.fromFile(RIGRECT)
    rig.computeRectificationMaps(destDims=(640, 360))
    rng = np.random.default_rng(12)
    dense = rng.uniform(0.25, 2.0, (4, 4)) * rng.choice([-1.0, 1.0], (4, 4))
    wzero = np.array([[1, 0, 0, -5.0], [0, 1, 0, -1.0], [0, 0, 0, 1000.0], [0, 0, 8.0, -8.0 * 37]])
    for Q in (rig.getQ(), dense, wzero):
        d = rng.integers(-32768, 32768, (3, 200)).astype(np.int16)
        d[:, ::9] = 37
        d[:, 5] = 37
        d[0, :4] = (0, -1, -32768, 32767)
        g = _fp64_reproject(d, Q)
        assert rig_oracle.reproject_check_longdouble(g, d, Q)[0] == 0
        t, tol, cls = rig_oracle.reproject_longdouble(d, Q)
        for y in range(3):
            for x in range(0, 200, 3):
                assert rig_oracle.reproject_check_exact(g[y, x], Q, x, y, int(d[y, x])) is None
                for r, e in enumerate(rig_oracle.reproject_exact(Q, x, y, int(d[y, x]))):
                    if e[0] == "value":
                        assert cls[y, x, r] == 0 and abs(float(t[y, x, r]) - float(e[1])) <= 1e-15 * abs(float(e[1])) + 1e-300
                        # (the longdouble bound adds that evaluation's own error: 2^-11 of the second term)
                        assert float(e[2]) * (1 - 1e-12) <= float(tol[y, x, r]) <= float(e[2]) * (1 + 2.0 ** -11 + 1e-12)
                    else:
                        assert cls[y, x, r] == (2 if e[0] == "nan" else e[1])
        # teeth: two float32 ulps off is outside the bound (well-conditioned pixels), in both references
        fin = np.argwhere(np.isfinite(g).all(-1) & (cls == 0).all(-1) & (tol[..., 0] <= np.spacing(np.abs(g[..., 0])) * 0.75))
        assert len(fin) > 50
        y, x = fin[7]
        bad = g.copy()
        bad[y, x, 0] = np.nextafter(np.nextafter(bad[y, x, 0], np.float32(np.inf)), np.float32(np.inf))
        assert rig_oracle.reproject_check_longdouble(bad, d, Q)[0] == 1
        assert rig_oracle.reproject_check_exact(bad[y, x], Q, x, y, int(d[y, x])) is not None
    # W = 0 exactly (last matrix): +inf / -inf by the numerator's sign, NaN where that is 0 as well; a finite value or the wrong sign fails
    assert [e[0] for e in rig_oracle.reproject_exact(wzero, 5, 1, 37)] == ["nan", "nan", "inf"]
    assert rig_oracle.reproject_exact(wzero, 3, 2, 37) == [("inf", -1), ("inf", 1), ("inf", 1)]
    assert rig_oracle.reproject_check_exact(np.float32([-np.inf, np.inf, np.inf]), wzero, 3, 2, 37) is None
    assert rig_oracle.reproject_check_exact(np.float32([np.inf, np.inf, np.inf]), wzero, 3, 2, 37) is not None
    assert rig_oracle.reproject_check_exact(np.float32([-3e38, np.inf, np.inf]), wzero, 3, 2, 37) is not None
    assert rig_oracle.reproject_check_exact(np.float32([np.nan, np.inf, np.inf]), wzero, 3, 2, 37) is not None
    # beyond the float32 range: infinity of the right sign
    huge = np.array([[1e30, 0, 0, 1e30], [0, 1, 0, 0], [0, 0, 0, 1], [0, 0, 0, 1e-10]])
    assert rig_oracle.reproject_exact(huge, 3, 2, 1)[0] == ("inf", 1)


def test_remap_coordinates_outside_every_range_give_the_border_value():
    """NaN, +-inf and coordinates whose product with 32 leaves int32: cvRound gives INT_MIN, the pixel is the border value 0 --
    in the oracle's definition and in the numpy host path, bilinear and nearest"""
    from oracle import rig_oracle
    assert rig_oracle.cv_round(float("nan")) == rig_oracle.cv_round(float("inf")) == rig_oracle.cv_round(2.0 ** 31) == -2 ** 31
    assert rig_oracle.cv_round(-2.0 ** 31) == -2 ** 31 and rig_oracle.cv_round(2.0 ** 31 - 1) == 2 ** 31 - 1
    assert [rig_oracle.cv_round(v) for v in (0.5, 1.5, 2.5, -0.5, -1.5, -2.5)] == [0, 2, 2, 0, -2, -2]
    rng = np.random.default_rng(4)
    img = rng.integers(1, 256, (7, 8, 3)).astype(np.uint8)
    out = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 2.0 ** 26, -2.0 ** 26]
    mx = np.array([out + [2.25] * len(out) + out + [0.0] * len(out) + out], np.float32)
    my = np.array([[3.5] * len(out) + out + out + out + [0.0] * len(out)], np.float32)
    for interp in (_rigs.INTER_LINEAR, _rigs.INTER_NEAREST):
        with np.errstate(invalid="ignore"):
            host = _rigs._remap(img, mx, my, interp)
        assert (host == 0).all()
        assert np.array_equal(host, rig_oracle.remap_bilinear(img, mx, my, nearest=(interp == _rigs.INTER_NEAREST)))


def test_remap_coordinates_on_the_64th_pixel_grid_oracle_equals_host_path():
    """-1/64 -> cell 0, fraction 0; -3/64 -> cell -1, fraction 30/32 (half to even), and the whole grid around a small image"""
    from oracle import rig_oracle
    rng = np.random.default_rng(6)
    img = rng.integers(1, 256, (4, 5, 3)).astype(np.uint8)
    k = np.arange(-3 * 64, 7 * 64 + 1, dtype=np.float32) / np.float32(64)
    mx, my = np.meshgrid(k[::3], k[::5])
    mx, my = np.ascontiguousarray(mx, np.float32), np.ascontiguousarray(my, np.float32)
    for interp in (_rigs.INTER_LINEAR, _rigs.INTER_NEAREST):
        assert np.array_equal(_rigs._remap(img, mx, my, interp), rig_oracle.remap_bilinear(img, mx, my, nearest=(interp == 0)))
    two = _rigs._remap(img, np.array([[-1 / 64, -3 / 64]], np.float32), np.zeros((1, 2), np.float32))
    assert np.array_equal(two[0, 0], img[0, 0])
    assert np.array_equal(two[0, 1], (30 * 32 * img[0, 0].astype(np.int64) + 512) >> 10)
