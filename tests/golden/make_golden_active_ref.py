"""Writes tests/golden/active_ref_cases.{npz,json}: what the reference's OWN simplestereo/active.py computes on the small cases
of the active tests.  Run from the repository root, where the reference lies and cv2 need not exist:

    python tests/golden/make_golden_active_ref.py

The reference's modules are loaded from where they lie by oracle/ref_active.py, with a cv2 stand-in built from the numpy
restatements of tests/_stereo_ftp_ref.py and tests/_graycode_ref.py: the fixtures pin the reference's own numpy, scipy and
control flow; the cv2 calls stay unpinned against cv2.  Nothing here imports simplestereo_amd or runs a kernel, and no input
is stored that a seeded helper regenerates (S.render, S.build_fringe, G.scene, G.rig; the rigs are in the json).

Per cloud case of StereoFTP and StereoFTP_Mapping the reference runs twice: as it is, and with the np.angle of its demodulation
answered by the np.longdouble phase of the same images and band (_ftp_ref.truth_longdouble, _ftp_mapping_ref.
carrier_truth_longdouble) -- the module's `np` is wrapped for that one run, its text is untouched.
  numpy_err : the worst relative distance of a point between the two runs (StereoFTP: over the pixels with
              |ghat conj(g0hat)| >= 0.01 of its row maximum, at least 90 % of them; Mapping: everywhere), so the reference's own
  tol       : 16 * max(numpy_err, 2^-52)
Both runs are asserted to unwrap identically (the unwrapped maps differ by less than 1e-9).  The three maps of
StereoFTP_PhaseOnly.getPhase get the rule of make_golden_ftp.py: numpy_err the worst angle to the np.longdouble phase over
the well-conditioned pixels, tol = 16 * max(numpy_err, pi 2^-52).  GrayCode demodulates nothing, so there is no second run of
the reference to take: its numpy_err is the distance of the reference's cloud to the restatement's per-pixel triangulation
evaluated in np.longdouble on the same fp64 geometry (_graycode_ref.cloud_dense) -- not the reference's own, and the json
says so.
The intermediate values are read through wrappers around the instance's methods."""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _active_ref as AR            # noqa: E402
import _ftp_cloud_ref as C          # noqa: E402
import _ftp_mapping_ref as M        # noqa: E402
import _ftp_ref as P                # noqa: E402
import _graycode_ref as G           # noqa: E402
from make_golden_stereo_ftp import CAMERA_DIST, PERIOD, scene_rig      # noqa: E402
from oracle import ref_active       # noqa: E402

TOL_FACTOR, CLOUD_FLOOR, ANGLE_FLOOR, KEEP_RATIO, MIN_KEPT = 16.0, 2.0 ** -52, float(np.pi * 2.0 ** -52), 0.01, 0.90
ROI0, ROI17, ROI_SMALL = (0, 0, 110, 34), (17, 5, 110, 34), (50, 10, 60, 20)
NO_DIST = [0.0] * 5


def rig_with(dist1=NO_DIST, dist2=None):
    rig = scene_rig(dist1)
    if dist2 is not None:
        rig["distCoeffs2"] = list(C.DIST_MODELS[dist2])
    return rig


# name: (rig, roi, radius_factor, unwrappingMethod)
FTP = {
    "full": (rig_with(), None, 0.5, None),
    "roi_origin": (rig_with(), ROI0, 0.5, None),
    "roi_17_5": (rig_with(), ROI17, 0.5, None),
    "roi_camera_dist": (rig_with(CAMERA_DIST), ROI17, 0.5, None),
    "proj_none": (rig_with(dist2="none"), ROI_SMALL, 0.5, None),
    "proj_d8": (rig_with(dist2="d8"), ROI_SMALL, 0.5, None),
    "proj_d12": (rig_with(dist2="d12"), ROI_SMALL, 0.5, None),
    "radius_0.3": (rig_with(), ROI_SMALL, 0.3, None),
    "callable": (rig_with(), ROI_SMALL, 0.5, "columns_first"),
}
MAPPING = {
    "full": (rig_with(), None, 0.5, None),
    "roi_origin": (rig_with(), ROI0, 0.5, None),
    "roi_17_5_inplace_shift": (rig_with(), ROI17, 0.5, None),
}
GRAY_RES1, GRAY_RES2, GRAY_ROI, GRAY_ROI_SMALL = (67, 37), (64, 32), (3, 5, 60, 36), (3, 5, 33, 20)
# name: (G.rig arguments, white_thr, roi, seed)
GRAY = {
    "d5_full": (dict(res2=GRAY_RES2, dist2="d5", dist1=CAMERA_DIST), 5, None, 1),
    "d8_full": (dict(res2=GRAY_RES2, dist2="d8", dist1=CAMERA_DIST), 5, None, 2),
    "d5_roi": (dict(res2=GRAY_RES2, dist2="d5", dist1=CAMERA_DIST), 5, GRAY_ROI, 3),
    "d8_roi_thr0": (dict(res2=GRAY_RES2, dist2="d8", dist1=CAMERA_DIST), 0, GRAY_ROI, 4),
    "t2_zero_roi": (dict(res2=GRAY_RES2, dist2="d5", T=(-250.0, 10.0, 0.0)), 5, GRAY_ROI_SMALL, 5),
    "projector_1x1_roi": (dict(res2=(1, 1), dist2="d5"), 5, GRAY_ROI_SMALL, 6),
}
# name: (channel holding the stripe, color argument, sensitivity, interpolation, blanked rows | "all")
STRIPE = {
    "r_0.5_linear": (2, "r", 0.5, "linear", []),
    "red_0.3_linear": (2, "red", 0.3, "linear", []),
    "g_0.5_linear_gaps": (1, "g", 0.5, "linear", [0, 1, 10, 11, 12, 13, 30, 47]),
    "green_0.3_cubic_gaps": (1, "green", 0.3, "cubic", [0, 1, 10, 11, 12, 13, 30, 47]),
    "b_0.5_cubic": (0, "b", 0.5, "cubic", []),
    "blue_0.5_linear_gaps": (0, "blue", 0.5, "linear", [5, 6, 7, 46, 47]),
    "no_stripe": (2, "r", 0.5, "linear", "all"),
}
FRINGE = {
    "plain": dict(period=12.0, dims=(64, 24)),
    "shift": dict(period=12.0, shift=2.5, dims=(64, 24)),
    "vertical": dict(period=10.5, dims=(64, 24), vertical=True),
    "vertical_red_shift": dict(period=10.5, shift=-3.0, dims=(64, 24), vertical=True, stripeColor="red"),
    "r": dict(period=12.0, dims=(64, 24), stripeColor="r"),
    "g": dict(period=12.0, dims=(64, 24), stripeColor="g"),
    "b": dict(period=12.0, dims=(64, 24), stripeColor="b"),
    "blue_shift": dict(period=7.25, shift=1.5, dims=(61, 9), stripeColor="blue"),
    "green_uint16": dict(period=12.0, dims=(64, 24), stripeColor="green", dtype="uint16"),
    "float64": dict(period=12.0, shift=0.5, dims=(64, 24), dtype="float64"),
    "scene_red": dict(period=PERIOD, stripeColor="red"),                # the fringe of every scene here; its first row is stored
}
PEAK = [(1280, 12.0, 0), (1280, 12.0, 2.5), (64, 10.5, -3.0), (61, 7.25, 1.5), (160, 12.0, 0.0), (7, 12.0, 1.0), (1, 1.0, 0)]
GRAY_IMGS = (64, 48)


class NumpyFor:
    """`np` of the reference's active module for one run: numpy, except that np.angle answers `phase` when one is given,
    and the result of the last np.unwrap is kept"""

    def __init__(self, phase=None):
        self._phase, self.unwrapped = phase, None

    def __getattr__(self, name):
        return getattr(np, name)

    def angle(self, z):
        return np.angle(z) if self._phase is None else np.array(self._phase)

    def unwrap(self, *a, **kw):
        self.unwrapped = np.unwrap(*a, **kw)
        return self.unwrapped


def make_rig(ref, r):
    return ref.StereoRig(tuple(r["res1"]), tuple(r["res2"]), r["intrinsic1"], r["intrinsic2"], r["distCoeffs1"], r["distCoeffs2"], r["R"], r["T"])


def run_class(ref, kind, rig, roi, radius_factor, method, phase=None, call="getCloud"):
    """One call of the reference's class -> (result, what the wrappers saw).  Wrappers only: the instance's methods, the
    module's findCentralStripe, the stand-in's undistort and the module's `np` are wrapped for the call and put back."""
    A, cv2 = ref.active, ref.cv2
    inst = getattr(A, kind)(make_rig(ref, rig), AR.fringe(PERIOD), PERIOD)
    rec, proxy = {}, NumpyFor(phase)
    keep = (inst._triangulate, inst._calculateCameraFrequency, inst._getProjectorMapping, A.findCentralStripe, cv2.undistort, A.np)

    def tri(camPoints, p_x, r):
        out = keep[0](camPoints, p_x, r)
        rec.setdefault("stripe_world", np.array(out))
        return out

    def freq(objPoints):
        out = keep[1](objPoints)
        rec.setdefault("fc", np.array(out))
        return out

    def mapping(z, *a, **kw):
        out = keep[2](z, *a, **kw)
        rec["z_plane"], rec["ref_full"] = float(z), np.array(out[1])
        return out

    def stripe(*a, **kw):
        out = keep[3](*a, **kw)
        rec.setdefault("stripe_cam", None if out is None else np.array(out))
        return out

    def undistort(*a, **kw):
        out = keep[4](*a, **kw)
        rec["undistorted_full"] = np.array(out)
        return out

    def unwrapper(ph):
        proxy.unwrapped = AR.UNWRAPPERS[method](ph)
        return proxy.unwrapped
    inst._triangulate, inst._calculateCameraFrequency, inst._getProjectorMapping = tri, freq, mapping
    A.findCentralStripe, cv2.undistort, A.np = stripe, undistort, proxy
    try:
        img = np.array(AR.frame(rig, PERIOD))
        if call == "getCloud":
            out = inst.getCloud(img, radius_factor=radius_factor, roi=roi, unwrappingMethod=None if method is None else unwrapper)
        else:
            out = inst.getPhase(img, radius_factor=radius_factor, roi=roi)
    finally:
        A.findCentralStripe, cv2.undistort, A.np = keep[3:]
    rec.update(F=np.array(inst.F), Rectify1=np.array(inst.Rectify1), Rectify2=np.array(inst.Rectify2), R_inv=np.array(inst.R_inv),
               baseline=float(inst.stereoRig.getBaseline()), unwrapped=proxy.unwrapped, peak=float(inst.stripeCentralPeak))
    x0, y0, w, h = AR.box(rig, roi)
    rec["undistorted"] = np.ascontiguousarray(rec["undistorted_full"][y0:y0 + h, x0:x0 + w])
    if "ref_full" in rec:
        rec["ref"] = np.ascontiguousarray(rec["ref_full"][y0:y0 + h, x0:x0 + w])
    return out, rec


def cloud_case(ref, kind, name, rig, roi, rf, method, arrays):
    cloud, rec = run_class(ref, kind, rig, roi, rf, method)
    if kind == "StereoFTP":
        truth_phase, ratio = P.truth_longdouble(rec["undistorted"], rec["ref"], rec["fc"], rf)
        keep = ratio >= KEEP_RATIO
        assert keep.mean() >= MIN_KEPT, (name, float(keep.mean()))
    else:
        truth_phase = M.carrier_truth_longdouble(rec["undistorted"], rec["fc"], rf)[0]
        keep = np.ones(truth_phase.shape, bool)
    truth, trec = run_class(ref, kind, rig, roi, rf, method, phase=truth_phase)
    unwrap_diff = float(np.abs(rec["unwrapped"] - trec["unwrapped"]).max())
    assert unwrap_diff < 1e-9, (kind, name, unwrap_diff)
    assert np.isfinite(cloud).all() and np.isfinite(truth).all() and cloud.dtype == np.float64
    numpy_err = float(C.rel_err(cloud, truth.astype(np.longdouble))[keep].max())
    assert numpy_err < 1e-9, (kind, name, numpy_err)
    tol = TOL_FACTOR * max(numpy_err, CLOUD_FLOOR)
    key = ("ftp_" if kind == "StereoFTP" else "mapping_") + name
    frame_cut = AR.frame(rig, PERIOD)[AR.box(rig, roi)[1]:, AR.box(rig, roi)[0]:][:rec["undistorted"].shape[0], :rec["undistorted"].shape[1]]
    same_as_frame = bool(np.array_equal(rec["undistorted"], frame_cut))
    for f in ("stripe_cam", "stripe_world", "fc", "F", "Rectify1", "Rectify2", "R_inv") + (("ref",) if "ref" in rec else ()):
        arrays[key + "__" + f] = rec[f]
    arrays[key + "__cloud"] = cloud
    if not same_as_frame:
        arrays[key + "__undistorted"] = rec["undistorted"]
    if kind == "StereoFTP":
        arrays[key + "__keep"] = np.packbits(keep)
    entry = {"rig": rig, "roi": None if roi is None else list(roi), "radius_factor": rf, "unwrap": method, "numpy_err": numpy_err, "tol": tol,
             "numpy_err_of": "the reference's own two runs", "unwrap_diff": unwrap_diff, "kept": float(keep.mean()),
             "baseline": rec["baseline"], "peak": rec["peak"], "undistorted_is_the_frame": same_as_frame}
    if "z_plane" in rec:
        entry["z_plane"] = rec["z_plane"]
    print("%-10s %-24s numpy_err %.3e  tol %.3e  unwrapped maps differ by %.1e  kept %.3f" % (kind[6:] or "FTP", name, numpy_err, tol, unwrap_diff, keep.mean()))
    return entry


def phase_only(ref, arrays):
    rig, roi, rf = rig_with(CAMERA_DIST), ROI17, 0.5
    out, rec = run_class(ref, "StereoFTP_PhaseOnly", rig, roi, rf, None, call="getPhase")
    assert isinstance(out, tuple) and len(out) == 3
    truths = (P.truth_longdouble(rec["undistorted"], rec["ref"], rec["fc"], rf), M.carrier_truth_longdouble(rec["undistorted"], rec["fc"], rf),
              M.carrier_truth_longdouble(rec["ref"], rec["fc"], rf))
    errs, tols = [], []
    for i, (got, (truth, ratio)) in enumerate(zip(out, truths)):
        keep = ratio >= KEEP_RATIO
        assert keep.mean() >= MIN_KEPT and got.shape == (roi[3], roi[2]) and got.dtype == np.float64
        errs.append(float(P.wrap_err(got, truth)[keep].max()))
        tols.append(TOL_FACTOR * max(errs[-1], ANGLE_FLOOR))
        arrays["phase_only_roi__out%d" % i] = got
        arrays["phase_only_roi__keep%d" % i] = np.packbits(keep)
    for f in ("stripe_world", "fc", "ref"):
        arrays["phase_only_roi__" + f] = rec[f]
    print("PhaseOnly  roi                      numpy_err %s  tol %s" % (["%.2e" % e for e in errs], ["%.2e" % t for t in tols]))
    entry = {"roi": {"rig": rig, "roi": list(roi), "radius_factor": rf, "numpy_err": errs, "tol": tols, "z_plane": rec["z_plane"]}}
    try:
        run_class(ref, "StereoFTP_PhaseOnly", rig, None, rf, None, call="getPhase")
        raise AssertionError("the reference's getPhase(roi=None) returned")
    except UnboundLocalError as e:
        entry["roi_none"] = {"rig": rig, "exception": type(e).__name__, "message": str(e)}
        print("PhaseOnly  roi=None                 %s: %s" % (type(e).__name__, e))
    return entry


def graycode_case(ref, name, args, thr, roi, seed, arrays):
    rig = G.rig(GRAY_RES1, **args)
    c = {"rig": rig, "seed": seed, "noise": 2, "holes": 0.1, "white_thr": thr, "roi": None if roi is None else list(roi)}
    stack = AR.graycode_stack(c)
    names = ["%s/%d.png" % (name, i) for i in range(stack.shape[0])] + [name + "/white.png"]      # a following extra image is ignored
    ref.cv2.files.clear()
    ref.cv2.files.update({n: stack[i] for i, n in enumerate(names[:-1])})
    ref.cv2.files[names[-1]] = np.full(stack.shape[1:] if stack.shape[0] else GRAY_RES1[::-1], 255, np.uint8)
    gc = ref.active.GrayCode(make_rig(ref, rig), white_thr=thr)
    cloud = gc.getCloud(names, roi=roi)
    ref.cv2.files.clear()
    assert gc.num_patterns == stack.shape[0] and cloud.ndim == 3 and cloud.shape[1:] == (1, 3) and cloud.dtype == np.float64
    arrays["gray_" + name + "__cloud"] = cloud
    arrays["gray_" + name + "__Rectify1"], arrays["gray_" + name + "__Rectify2"], arrays["gray_" + name + "__R_inv"] = gc.Rectify1, gc.Rectify2, gc.R_inv
    x0, y0, xe, ye = roi or (0, 0) + GRAY_RES1
    und = G.undistort_stack(stack, rig["intrinsic1"], rig["distCoeffs1"], GRAY_RES1)
    decoded = G.decode(und, rig["res2"][0], rig["res2"][1], thr, shape=GRAY_RES1[::-1])[y0:ye, x0:xe]
    truth = G.compact(G.cloud_dense(G.geometry(rig), decoded, x0, y0, dtype=np.longdouble), decoded)
    assert truth.shape == cloud.shape and np.isfinite(cloud).all()
    numpy_err = float(C.rel_err(cloud, truth).max())
    c.update(n=int(cloud.shape[0]), pixels=(xe - x0) * (ye - y0), num_patterns=int(gc.num_patterns), numpy_err=numpy_err,
             tol=TOL_FACTOR * max(numpy_err, CLOUD_FLOOR), baseline=float(gc.rig.getBaseline()),
             numpy_err_of="the reference's cloud against the restatement's triangulation in np.longdouble on the fp64 geometry")
    print("GrayCode   %-24s numpy_err %.3e  tol %.3e  %d of %d pixels, %d patterns" % (name, numpy_err, c["tol"], c["n"], c["pixels"], c["num_patterns"]))
    return c


def main():
    ref = ref_active.load()
    if ref is None:
        raise SystemExit("the reference is not here: nothing written")
    A = ref.active
    arrays, meta = {}, {"period": PERIOD, "tol_factor": TOL_FACTOR, "cloud_floor": CLOUD_FLOOR, "angle_floor": ANGLE_FLOOR, "keep_ratio": KEEP_RATIO,
                        "packed": {}, "cv2": "a stand-in made of the numpy restatements (oracle/ref_active.py): unpinned against cv2"}
    meta["ftp"] = {n: cloud_case(ref, "StereoFTP", n, *a, arrays) for n, a in FTP.items()}
    meta["mapping"] = {n: cloud_case(ref, "StereoFTP_Mapping", n, *a, arrays) for n, a in MAPPING.items()}
    meta["phase_only"] = phase_only(ref, arrays)
    meta["graycode"] = {n: graycode_case(ref, n, *a, arrays) for n, a in GRAY.items()}

    with tempfile.TemporaryDirectory() as tmp:
        from PIL import Image
        target = os.path.join(tmp, "patterns")                       # created by the function
        n = A.generateGrayCodeImgs(target, GRAY_IMGS)
        names = sorted(os.listdir(target))
        for f in names:
            with Image.open(os.path.join(target, f)) as im:
                assert im.mode == "L"
                arrays["gray_imgs__" + f[:-4]] = np.array(im, dtype=np.uint8)
        meta["gray_imgs"] = {"resolution": list(GRAY_IMGS), "count": int(n), "names": names, "bytes": "the decoded pixels of every file"}

    stripe_rig = rig_with()
    meta["stripe"] = {"rig": stripe_rig, "cases": {}}
    for name, (channel, color, sens, kind, blank) in STRIPE.items():
        recipe = {"channel": channel, "color": color, "sensitivity": sens, "interpolation": kind, "blank": blank}
        out = A.findCentralStripe(AR.stripe_image(recipe, stripe_rig, PERIOD), color, sens, kind)
        recipe["found"] = out is not None
        if out is not None:
            arrays["stripe_" + name + "__out"] = out
        meta["stripe"]["cases"][name] = recipe

    meta["fringe"] = {}
    for name, kw in FRINGE.items():
        call = dict(kw)
        if "dtype" in call:
            call["dtype"] = np.dtype(call["dtype"]).type
        out = A.buildFringe(**call)
        if name == "scene_red":                                      # 1280 x 720: every row is the first
            assert (out == out[:1]).all()
            out = out[:1]
        arrays["fringe_" + name + "__out"] = out
        meta["fringe"][name] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items()}
    bad = {}
    try:
        A.buildFringe(12.0, dims=(64, 24), stripeColor="yellow")
    except ValueError as e:
        bad = {"exception": "ValueError", "message": str(e)}
    meta["fringe_bad_color"] = bad
    meta["peak"] = [list(p) for p in PEAK]
    arrays["peak__out"] = np.array([A._getCentralPeak(*p) for p in PEAK], dtype=np.float64)
    bgr = np.array(AR.frame(stripe_rig, PERIOD)[:4, 70:90])
    assert np.array_equal(A.StereoFTP.convertGrayscale(bgr), np.max(bgr, axis=2))
    assert "cv2" in sys.modules and "simplestereo_amd" not in sys.modules
    AR.save(arrays, meta)
    print("wrote %s (%d bytes) and the json" % (os.path.relpath(AR.NPZ), os.path.getsize(AR.NPZ)))


if __name__ == "__main__":
    main()
