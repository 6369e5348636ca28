"""Writes tests/golden/phaseshift_cases.{npz,json}: what the reference's OWN StructuredLightRig (simplestereo/_rigs.py) holds and
triangulates on the small rigs of the phase-shift tests, and the tolerances of the decode and cloud cases.  Run from the
repository root, where the reference lies and cv2 need not exist:

    python tests/golden/make_golden_phaseshift.py

The reference's modules are loaded from where they lie by oracle/ref_active.py, with its cv2 stand-in made of the numpy
restatements: the fixtures pin the reference's own numpy and control flow; the cv2 calls stay unpinned against cv2.  Nothing here
imports simplestereo_amd or runs a kernel, and no input is stored that a seeded helper regenerates (P.scene, P.correspondences,
G.rig; the rigs and the recipes are in the json).

Tolerances, by the Gray-code rule of make_golden_active_ref.py (the reference demodulates nothing here, so there is no second run
of it to take):
  rigs    numpy_err : the worst relative distance of the reference's points to the restatement's triangulation evaluated in
                      np.longdouble on the same fp64 geometry;  tol = 16 * max(numpy_err, 2^-52)
  decode  numpy_err : the worst |p - p_longdouble| of the fp64 restatement of the three closures over the unmasked pixels (both
                      coordinates);  tol = 16 * max(numpy_err, proj_extent * 2^-52), proj_extent the larger projector side
  cloud   numpy_err : the worst relative distance of the fp64 restatement chain (decode, then triangulation on the pixel grid) to
                      the same chain in np.longdouble;  tol = 16 * max(numpy_err, 2^-52)
The decode and cloud errors are the restatement's, not the reference's own, and the json says so.
Asserted, not measured: in every heterodyne step of every pixel of every decode and cloud case |kk - rint(kk)| <= 0.25, in the fp64
and in the np.longdouble chain, so that no k hangs on a rounding."""
import io
import json
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _ftp_cloud_ref as C          # noqa: E402
import _graycode_ref as G           # noqa: E402
import _phaseshift_ref as P         # noqa: E402
from make_golden_stereo_ftp import CAMERA_DIST      # noqa: E402
from oracle import ref_active       # noqa: E402

TOL_FACTOR, FLOOR, TIE_MAX, NPOINTS = 16.0, 2.0 ** -52, 0.25, 40
RES1, RES2, SMALL = (67, 37), (64, 32), (9, 5)
PERIODS = [[64.0, 16.0, 5.0], [32.0, 8.0]]                          # nx != ny, a ratio that does not divide
PERIODS_8 = [[64.0, 48.0, 32.0, 24.0, 16.0, 12.0, 8.0, 6.0], [32.0, 24.0, 16.0, 12.0, 8.0, 6.0, 4.0, 3.0]]
PERIODS_1 = [[64.0], [32.0]]
ROI = [3, 5, 33, 20]                                                # (x, y, width, height): breaks the four-pixel alignment
# name: G.rig arguments
RIGS = {
    "none": dict(res2=RES2, dist2="none"),
    "d5": dict(res2=RES2, dist2="d5", dist1=CAMERA_DIST),
    "d8": dict(res2=RES2, dist2="d8"),
    "d12": dict(res2=RES2, dist2="d12", dist1=CAMERA_DIST),
    "t2_zero": dict(res2=RES2, dist2="d5", T=(-250.0, 10.0, 0.0)),
}
# name: (camera size, periods, roi, the rig whose camera maps are used | None, seed)
DECODE = {
    "full": (RES1, PERIODS, None, None, 11),
    "full_maps": (RES1, PERIODS, None, "d5", 12),
    "roi": (RES1, PERIODS, ROI, None, 13),
    "roi_maps": (RES1, PERIODS, ROI, "d12", 14),
    "periods_8": (SMALL, PERIODS_8, None, None, 15),
    "periods_1": (RES1, PERIODS_1, None, None, 16),
}
# name: (rig, roi, seed)
CLOUD = {"d5_full": ("d5", None, 21), "d12_roi": ("d12", ROI, 22), "t2_zero_roi": ("t2_zero", ROI, 23)}


def box_of(roi, res):
    return (0, 0, res[0], res[1]) if roi is None else tuple(roi)


def decode_both(stack, periods, roi, res):
    x0, y0, w, h = box_of(roi, res)
    cut = stack[:, y0:y0 + h, x0:x0 + w]
    d64, tie64 = P.decode(cut, periods, RES2, details=True)
    dld, tield = P.decode(cut, periods, RES2, dtype=np.longdouble, details=True)
    assert max(tie64.max(), tield.max()) <= TIE_MAX, (float(tie64.max()), float(tield.max()))
    assert np.isfinite(d64).all()
    return d64, dld, float(max(tie64.max(), tield.max()))


def save(arrays, meta):
    """An npz whose bytes depend on the arrays alone (fixed member dates, sorted names)"""
    with zipfile.ZipFile(P.NPZ, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.ascontiguousarray(arrays[key]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    with open(P.JSON, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ref = ref_active.load()
    if ref is None:
        raise SystemExit("the reference is not here: nothing written")
    arrays = {}
    meta = {"tol_factor": TOL_FACTOR, "floor": FLOOR, "tie_max": TIE_MAX, "proj_res": list(RES2), "rigs": {}, "decode": {}, "cloud": {},
            "cv2": "a stand-in made of the numpy restatements (oracle/ref_active.py): unpinned against cv2"}
    rigs = {name: G.rig(RES1, **args) for name, args in RIGS.items()}
    for i, (name, rig) in enumerate(rigs.items()):
        plain = ref.StereoRig(tuple(rig["res1"]), tuple(rig["res2"]), rig["intrinsic1"], rig["intrinsic2"], rig["distCoeffs1"], rig["distCoeffs2"],
                              rig["R"], rig["T"])
        sl = ref._rigs.StructuredLightRig(plain)
        cam, proj = P.correspondences(rig, NPOINTS, 100 + i)
        pts = sl.triangulate(cam, proj)
        assert pts.shape == (NPOINTS, 1, 3) and pts.dtype == np.float64 and np.isfinite(pts).all()
        truth = P.triangulate(P.sl_rig(rig)["geom"], cam, proj, dtype=np.longdouble)
        numpy_err = float(C.rel_err(pts, truth).max())
        assert numpy_err < 1e-9, (name, numpy_err)
        for f in ("R1", "R2", "R", "R_inv"):
            arrays["rig_%s__%s" % (name, f)] = np.array(getattr(sl, f), dtype=np.float64)
        arrays["rig_%s__points" % name] = pts
        meta["rigs"][name] = {"rig": rig, "seed": 100 + i, "n": NPOINTS, "baseline": float(sl.getBaseline()), "plain_baseline": float(plain.getBaseline()),
                              "numpy_err": numpy_err, "tol": TOL_FACTOR * max(numpy_err, FLOOR),
                              "numpy_err_of": "the reference's points against the restatement's triangulation in np.longdouble on the fp64 geometry"}
        print("rig    %-12s numpy_err %.3e  tol %.3e  baseline %r (plain rig %r)" % (name, numpy_err, meta["rigs"][name]["tol"], meta["rigs"][name]["baseline"],
                                                                                   meta["rigs"][name]["plain_baseline"]))
    try:
        ref._rigs.StructuredLightRig(rigs["d5"])
        raise AssertionError("the reference took a dict for a rig")
    except ValueError as e:
        meta["bad_rig"] = {"exception": "ValueError", "message": str(e)}

    for name, (res, periods, roi, maps, seed) in DECODE.items():
        stack = P.scene(seed, res, RES2, periods)
        if maps is not None:
            stack = G.undistort_stack(stack, rigs[maps]["intrinsic1"], rigs[maps]["distCoeffs1"], res)
        d64, dld, tie = decode_both(stack, periods, roi, res)
        numpy_err = float(np.abs(d64.astype(np.longdouble) - dld).max())
        meta["decode"][name] = {"res1": list(res), "periods": periods, "roi": roi, "maps_of_rig": maps, "seed": seed, "worst_tie": tie,
                                "numpy_err": numpy_err, "tol": TOL_FACTOR * max(numpy_err, max(RES2) * FLOOR),
                                "numpy_err_of": "the fp64 restatement against the same chain in np.longdouble"}
        print("decode %-12s numpy_err %.3e  tol %.3e  worst |kk - rint(kk)| %.3f" % (name, numpy_err, meta["decode"][name]["tol"], tie))

    for name, (rig_name, roi, seed) in CLOUD.items():
        rig = rigs[rig_name]
        stack = G.undistort_stack(P.scene(seed, RES1, RES2, PERIODS), rig["intrinsic1"], rig["distCoeffs1"], RES1)
        d64, dld, tie = decode_both(stack, PERIODS, roi, RES1)
        g, cam = P.sl_rig(rig)["geom"], P.grid(box_of(roi, RES1))
        c64 = P.triangulate(g, cam, d64)
        cld = P.triangulate(g, cam, dld, dtype=np.longdouble)
        assert np.isfinite(c64).all()
        numpy_err = float(C.rel_err(c64, cld).max())
        assert numpy_err < 1e-9, (name, numpy_err)
        meta["cloud"][name] = {"rig": rig_name, "periods": PERIODS, "roi": roi, "seed": seed, "worst_tie": tie, "numpy_err": numpy_err,
                               "tol": TOL_FACTOR * max(numpy_err, FLOOR),
                               "numpy_err_of": "the fp64 restatement chain against the same chain in np.longdouble"}
        print("cloud  %-12s numpy_err %.3e  tol %.3e" % (name, numpy_err, meta["cloud"][name]["tol"]))
    assert "cv2" in sys.modules and "simplestereo_amd" not in sys.modules
    save(arrays, meta)
    print("wrote %s (%d bytes) and the json" % (os.path.relpath(P.NPZ), os.path.getsize(P.NPZ)))


if __name__ == "__main__":
    main()
