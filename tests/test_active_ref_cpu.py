"""The numpy restatements (tests/_stereo_ftp_ref.py, _ftp_mapping_ref.py, _graycode_ref.py) and the host-side code of ss.active
against what the reference's OWN simplestereo/active.py computed: tests/golden/active_ref_cases.{npz,json}, recorded by
tests/golden/make_golden_active_ref.py with the reference loaded from where it lies and a cv2 stand-in.  No GPU, no cv2, no
reference here: only tests/golden is read.

Integer and byte results are compared exactly; float results within the tolerance recorded per case, 16 * max(numpy_err,
2^-52) with numpy_err the reference's own distance to itself run on the np.longdouble phase.  Measured here, restatement
against the reference, worst relative distance of a point: StereoFTP 7.9e-16 .. 1.3e-15 (tolerances 5.4e-15 .. 1.6e-14),
StereoFTP_Mapping 6.3e-16 .. 8.0e-16 (1.3e-14 .. 1.4e-14), GrayCode 4.5e-16 .. 1.0e-15, 4.2e-15 for the ill-conditioned 1 x 1
projector (1.4e-14 and up); with the fundamental matrix built in float64 throughout, as before the reference's float32
cross-product matrix was followed, StereoFTP 1.22e-10 .. 1.26e-10 and StereoFTP_Mapping 1.27e-10 .. 1.30e-10."""
import os
import sys

import numpy as np
import pytest

import _active_ref as AR
import _ftp_cloud_ref as C
import _ftp_mapping_ref as M
import _ftp_ref as P
import _graycode_ref as G
import _stereo_ftp_ref as S

META, DATA = AR.load()
PERIOD = META["period"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _rel(a, b):
    """worst |a - b| / |b| of two float arrays"""
    return float((np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)).max())


def _rows(a, b):
    """worst relative distance of the points (rows) of a to those of b"""
    return float(C.rel_err(np.asarray(a), np.asarray(b).astype(np.longdouble)).max())


def _undistorted(c, d):
    x0, y0, w, h = AR.box(c["rig"], c["roi"])
    return AR.frame(c["rig"], PERIOD)[y0:y0 + h, x0:x0 + w] if c["undistorted_is_the_frame"] else d["undistorted"]


def test_no_stand_in_cv2_in_this_process():
    """the loader's fake cv2 belongs to the golden maker's process: here cv2 is absent, or the real one"""
    assert "simplestereo" not in sys.modules
    assert "cv2" not in sys.modules or getattr(sys.modules["cv2"], "__file__", None)


# ------------------------------------------------------------------------------------------------ what __init__ derives
@pytest.mark.parametrize("name", sorted(META["ftp"]))
def test_fundamental_matrix_and_rectification_are_the_references_bits(name):
    import simplestereo_amd as ss
    c, d = META["ftp"][name], AR.fields(DATA, "ftp_" + name)
    rig = C.make_rig(ss, c["rig"])
    assert _bits(rig.getFundamentalMatrix(), d["F"]) and rig.getFundamentalMatrix().dtype == np.float64
    rg = S.Rig(c["rig"], PERIOD, AR.fringe(PERIOD).shape[1])
    assert _bits(rg.F, d["F"])
    assert _bits(M.mapping_geometry(c["rig"], PERIOD)[1], d["F"].reshape(9))
    sf = ss.active.StereoFTP(C.make_rig(ss, c["rig"]), AR.fringe(PERIOD), PERIOD)
    assert _bits(sf.F, d["F"]) and _bits(sf.Rectify1, d["Rectify1"]) and _bits(sf.Rectify2, d["Rectify2"]) and _bits(sf.R_inv, d["R_inv"])
    assert _bits(rg.Rectify1, d["Rectify1"]) and _bits(rg.Rectify2, d["Rectify2"]) and _bits(rg.R_inv, d["R_inv"][:3, :3])
    assert not d["R_inv"][:3, 3].any() and np.array_equal(d["R_inv"][3], [0, 0, 0, 1])
    assert rig.getBaseline() == c["baseline"] and rg.baseline == c["baseline"]
    assert sf.stripeCentralPeak == c["peak"] and rg.peak == c["peak"]
    # E = K2^T F K1 inherits the rounding
    assert _bits(C.make_rig(ss, c["rig"]).getEssentialMatrix(), np.array(c["rig"]["intrinsic2"]).T.dot(d["F"]).dot(np.array(c["rig"]["intrinsic1"])))


def test_float64_cross_matrix_would_be_noticed():
    """F of the scene's rig with the cross-product matrix left in float64 is 1e-7 away: the rounding is observable"""
    c, d = META["ftp"]["full"], AR.fields(DATA, "ftp_full")
    K1, K2, R, T = (np.array(c["rig"][k], dtype=np.float64) for k in ("intrinsic1", "intrinsic2", "R", "T"))
    v = K1.dot(R.T).dot(T.reshape(3, 1)).ravel()
    F64 = np.linalg.inv(K2).T.dot(R).dot(K1.T).dot(np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]))
    assert 1e-9 < np.abs(F64 - d["F"]).max() / np.abs(d["F"]).max() < 1e-6


# ------------------------------------------------------------------------------------------------ StereoFTP.getCloud
@pytest.mark.parametrize("name", sorted(META["ftp"]))
def test_stereo_ftp_restatement_against_the_reference(name):
    import simplestereo_amd as ss
    c, d = META["ftp"][name], AR.fields(DATA, "ftp_" + name)
    roi = None if c["roi"] is None else tuple(c["roi"])
    x0, y0, w, h = AR.box(c["rig"], roi)
    mine = S.pipeline(c["rig"], AR.fringe(PERIOD), PERIOD, AR.frame(c["rig"], PERIOD), roi, c["radius_factor"],
                      unwrap=None if c["unwrap"] is None else AR.UNWRAPPERS[c["unwrap"]])
    assert np.array_equal(mine["undistorted"], _undistorted(c, d)) and mine["undistorted"].dtype == np.uint8
    assert _bits(mine["stripe"], d["stripe_cam"])
    assert np.array_equal(mine["ref"], d["ref"]) and mine["ref"].dtype == np.uint8
    tol = c["tol"]
    errs = {"stripe_world": _rows(mine["world"], d["stripe_world"]), "z_plane": abs(mine["z_plane"] - c["z_plane"]) / c["z_plane"],
            "fc": _rel(mine["fc"], d["fc"])}
    keep = np.unpackbits(d["keep"])[:h * w].reshape(h, w).astype(bool)
    assert mine["cloud"].shape == d["cloud"].shape == (h, w, 3) and np.isfinite(mine["cloud"]).all()
    errs["cloud"] = float(C.rel_err(mine["cloud"], d["cloud"].astype(np.longdouble))[keep].max())
    # the host-side product code on the reference's own intermediate values
    sf = ss.active.StereoFTP(C.make_rig(ss, c["rig"]), AR.fringe(PERIOD), PERIOD)
    world = sf._triangulate(d["stripe_cam"], sf.stripeCentralPeak, (x0, y0, w, h))
    errs["ss._triangulate"] = _rows(world, d["stripe_world"])
    errs["ss._calculateCameraFrequency"] = _rel(sf._calculateCameraFrequency(d["stripe_world"]), d["fc"])
    print("ftp %-16s numpy_err %.3e tol %.3e  restatement vs reference: %s" % (name, c["numpy_err"], tol, {k: "%.2e" % v for k, v in errs.items()}))
    assert all(v <= tol for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------ StereoFTP_Mapping.getCloud
@pytest.mark.parametrize("name", sorted(META["mapping"]))
def test_mapping_restatement_against_the_reference(name):
    c, d = META["mapping"][name], AR.fields(DATA, "mapping_" + name)
    roi = None if c["roi"] is None else tuple(c["roi"])
    x0, y0, w, h = AR.box(c["rig"], roi)
    args = (c["rig"], AR.fringe(PERIOD), PERIOD, AR.frame(c["rig"], PERIOD), roi, c["radius_factor"])
    shifted = (x0, y0) != (0, 0)
    mine = AR.mapping_with_inplace_shift(*args) if shifted else M.pipeline_mapping(*args)
    assert np.array_equal(mine["undistorted"], _undistorted(c, d)) and _bits(mine["stripe"], d["stripe_cam"])
    errs = {"stripe_world": _rows(mine["world"], d["stripe_world"]), "fc": _rel(mine["fc"], d["fc"])}
    assert mine["cloud"].shape == d["cloud"].shape == (h, w, 3) and np.isfinite(mine["cloud"]).all()
    errs["cloud"] = _rows(mine["cloud"], d["cloud"])
    print("mapping %-24s numpy_err %.3e tol %.3e  restatement vs reference: %s" % (name, c["numpy_err"], c["tol"], {k: "%.2e" % v for k, v in errs.items()}))
    assert all(v <= c["tol"] for v in errs.values()), errs
    if shifted:
        # the README row: sampled where the stripe is, the cloud is per cent away from the reference's
        plain = _rows(M.pipeline_mapping(*args)["cloud"], d["cloud"])
        print("   without the in-place shift: %.3e" % plain)
        assert 1e-3 < plain < 1e-1


# ------------------------------------------------------------------------------------------------ StereoFTP_PhaseOnly.getPhase
def test_phase_only_restatement_against_the_reference():
    c, d = META["phase_only"]["roi"], AR.fields(DATA, "phase_only_roi")
    roi = tuple(c["roi"])
    mine = M.pipeline_phase_only(c["rig"], AR.fringe(PERIOD), PERIOD, AR.frame(c["rig"], PERIOD), roi, c["radius_factor"])
    assert np.array_equal(mine["ref"], d["ref"])
    tol = min(c["tol"])
    assert _rows(mine["world"], d["stripe_world"]) <= tol and _rel(mine["fc"], d["fc"]) <= tol and abs(mine["z_plane"] - c["z_plane"]) <= tol * c["z_plane"]
    for i, key in enumerate(("phase", "phase_obj", "phase_ref")):
        keep = np.unpackbits(d["keep%d" % i])[:roi[2] * roi[3]].reshape(roi[3], roi[2]).astype(bool)
        assert mine[key].shape == d["out%d" % i].shape == (roi[3], roi[2])
        err = float(P.wrap_err(mine[key], d["out%d" % i])[keep].max())
        print("phase_only out%d: numpy_err %.3e tol %.3e  restatement vs reference %.3e" % (i, c["numpy_err"][i], c["tol"][i], err))
        assert err <= c["tol"][i]


def test_phase_only_without_roi_is_an_error_in_the_reference_as_the_readme_says():
    rec = META["phase_only"]["roi_none"]
    assert rec["exception"] == "UnboundLocalError" and "roi_y" in rec["message"]
    with open(os.path.join(ROOT, "README.md")) as f:
        rows = [line for line in f if "getPhase(roi=None)" in line]
    assert len(rows) == 1 and "UnboundLocalError" in rows[0] and "whole frame" in rows[0]


# ------------------------------------------------------------------------------------------------ GrayCode.getCloud
@pytest.mark.parametrize("name", sorted(META["graycode"]))
def test_graycode_restatement_against_the_reference(name):
    c, d = META["graycode"][name], AR.fields(DATA, "gray_" + name)
    r = c["rig"]
    (w1, h1), (w2, h2) = r["res1"], r["res2"]
    stack = AR.graycode_stack(c)
    assert stack.shape[0] == c["num_patterns"] == G.num_patterns(w2, h2)
    und = G.undistort_stack(stack, r["intrinsic1"], r["distCoeffs1"], (w1, h1))
    x0, y0, xe, ye = c["roi"] or (0, 0, w1, h1)
    decoded = G.decode(und, w2, h2, c["white_thr"], shape=(h1, w1))[y0:ye, x0:xe]
    g = G.geometry(r)
    assert _bits(g[40:49].reshape(3, 3), d["Rectify1"]) and _bits(g[49:58].reshape(3, 3), d["Rectify2"]) and _bits(g[58:67].reshape(3, 3), d["R_inv"][:3, :3])
    assert g[67] == c["baseline"]
    mine = G.compact(G.cloud_dense(g, decoded, x0, y0), decoded)
    assert mine.shape == d["cloud"].shape == (c["n"], 1, 3) and 0 < c["n"] <= c["pixels"]          # the same count ...
    err = _rows(mine, d["cloud"])                                                                # ... and order: point by point
    print("graycode %-18s %d points  tol %.3e  restatement vs reference %.3e" % (name, c["n"], c["tol"], err))
    assert err <= c["tol"]


def test_generate_gray_code_imgs(tmp_path):
    import simplestereo_amd as ss
    from PIL import Image
    c = META["gray_imgs"]
    target = str(tmp_path / "patterns")
    assert ss.active.generateGrayCodeImgs(target, tuple(c["resolution"])) == c["count"]
    assert sorted(os.listdir(target)) == c["names"] and len(c["names"]) == c["count"] + 2
    pattern = G.pattern(*c["resolution"])
    for f in c["names"]:
        with Image.open(os.path.join(target, f)) as im:
            assert im.mode == "L" and np.array_equal(np.array(im), DATA["gray_imgs__" + f[:-4]]), f
        if f[:-4].isdigit():
            assert np.array_equal(pattern[int(f[:-4])], DATA["gray_imgs__" + f[:-4]])


# ------------------------------------------------------------------------------------------------ functions
@pytest.mark.parametrize("name", sorted(n for n, c in META["stripe"]["cases"].items() if c["interpolation"] == "linear"))
def test_find_central_stripe_restatement(name):
    c = META["stripe"]["cases"][name]
    out = S.find_central_stripe(AR.stripe_image(c, META["stripe"]["rig"], PERIOD), c["color"], c["sensitivity"])
    if c["found"]:
        assert _bits(out, DATA["stripe_" + name + "__out"])
        assert not c["blank"] or np.isfinite(out).all()
    else:
        assert out is None


@pytest.mark.parametrize("name", sorted(META["fringe"]))
def test_build_fringe(name):
    import simplestereo_amd as ss
    kw = dict(META["fringe"][name])
    want = DATA["fringe_" + name + "__out"]
    if "dims" in kw:
        kw["dims"] = tuple(kw["dims"])
    if "dtype" in kw:
        kw["dtype"] = np.dtype(kw["dtype"]).type
    got = ss.active.buildFringe(**kw)
    if name == "scene_red":
        assert got.shape == (720, 1280, 3) and (got == got[:1]).all() and _bits(got[:1], want)
        assert _bits(AR.fringe(PERIOD)[:1], want)
    else:
        assert _bits(got, want)
    if not kw.get("vertical") and "dtype" not in kw and name != "scene_red":
        color = kw.get("stripeColor")
        assert _bits(S.build_fringe(kw["period"], kw.get("shift", 0), kw["dims"], color), want)


def test_build_fringe_bad_colour_and_central_peak():
    import simplestereo_amd as ss
    with pytest.raises(ValueError) as e:
        ss.active.buildFringe(12.0, dims=(64, 24), stripeColor="yellow")
    assert META["fringe_bad_color"] == {"exception": "ValueError", "message": str(e.value)}
    for args, want in zip(META["peak"], DATA["peak__out"]):
        assert ss.active._getCentralPeak(*args) == want and S.central_peak(*args) == want
