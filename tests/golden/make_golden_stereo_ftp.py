"""Writes tests/golden/stereo_ftp_cases.{json,npz}: the small cases of tests/test_gpu_stereo_ftp.py and test_stereo_ftp_cpu.py.

    python tests/golden/make_golden_stereo_ftp.py

Everything comes from the numpy restatements of tests/_stereo_ftp_ref.py, _ftp_ref.py and _ftp_cloud_ref.py; nothing here
imports simplestereo_amd or runs a kernel.

"reference" cases (ss.active.ftpReference): a rig, an roi, a fringe and a z_plane; the expected image is the restatement's,
computed by the test.  The case "nonfinite" holds a z_plane found here for which the fp64 depth Z' in front of the projector
is exactly 0 at one pixel, and the geometry packed for it (the input that zero belongs to, bit for bit).

"cloud" cases (ss.active.StereoFTP.getCloud): a rendered 48 x 160 frame (a plane at 1000 with a smooth bump, lit by
buildFringe(12, stripeColor='r') through a projector 160 to the camera's side), with and without roi, one with lens distortion
on the camera.  Per case the generator measures, on numpy alone,
  numpy_err : the distance (worst relative error of a point over the kept pixels) between the numpy pipeline -- np.fft
              demodulation, np.unwrap, cloud_from_geometry -- and the same pipeline fed the np.longdouble phase of _ftp_ref.py
  tol       : 16 * max(numpy_err, 2^-52)
  keep      : the pixels where |ghat * conj(g0hat)| >= 0.01 of its row maximum (at least 90 % of them, asserted here)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ftp_cloud_ref as C      # noqa: E402
import _ftp_ref as P            # noqa: E402
import _stereo_ftp_ref as S     # noqa: E402

PERIOD = 12.0
TOL_FACTOR, TOL_FLOOR, KEEP_RATIO, MIN_KEPT = 16.0, 2.0 ** -52, 0.01, 0.90
CAMERA_DIST = [-0.08, 0.03, 0.0005, -0.0004, 0.0]


def small_rig():
    """a 96 x 24 camera whose view covers a 64 x 7 projector image and a margin of several pixels around it"""
    return {"res1": [96, 24], "res2": [64, 7], "intrinsic1": [[100.0, 0, 48.0], [0, 100.0, 12.0], [0, 0, 1]],
            "intrinsic2": [[85.0, 0, 32.0], [0, 85.0, 3.5], [0, 0, 1]], "distCoeffs1": [0.0] * 5,
            "distCoeffs2": list(C.DIST_MODELS["d5"]), "R": C.rotation(1.0, -2.0, 3.0).tolist(), "T": [5.0, 2.0, 10.0]}


def scene_rig(dist1):
    rig = C.rig_params(res1=(160, 48), dist="d5")
    rig["T"] = [150.0, 10.0, 60.0]          # the central stripe (projector columns 630 .. 641) falls in the middle of the frame
    rig["distCoeffs1"] = list(dist1)
    return rig


def tall_rig():
    return C.rig_params(res1=(2, 65537), dist="d8", k1_fy=150000.0)


# name: (rig, roi, fringe: "cos" = the gray of build_fringe | (wp, hp) of random bytes, z_plane)
REFERENCE = {
    "r3x130": (C.rig_params(dist="d8"), (575, 300, 130, 3), "cos", 1000.0),
    "r5x257_roi": (C.rig_params(dist="d8"), (501, 333, 257, 5), "cos", 1000.0),
    "dist_none": (C.rig_params(dist="none"), (560, 320, 66, 4), "cos", 950.0),
    "dist_d5": (C.rig_params(dist="d5"), (560, 320, 66, 4), "cos", 950.0),
    "dist_d8": (C.rig_params(dist="d8"), (560, 320, 66, 4), "cos", 950.0),
    "dist_d12": (C.rig_params(dist="d12"), (560, 320, 66, 4), "cos", 950.0),
    "fringe_7x64": (small_rig(), (0, 0, 96, 24), (64, 7), 1000.0),
    "fringe_1x1": (small_rig(), (0, 0, 96, 24), (1, 1), 1000.0),
    "tall_65537x2": (tall_rig(), (0, 0, 2, 65537), "cos", 1000.0),
    "nonfinite": (C.rig_params(dist="d5"), (600, 300, 66, 5), "cos", None),
}
NONFINITE_PIXEL = (2, 31)                                    # (y, x) inside the roi of "nonfinite"


def zero_depth_plane(rig, u, v):
    """a z_plane for which the restatement's Z' = ((M6 u + M7 v) + M8) + T2 is exactly 0.0 at the camera pixel (u, v)"""
    K1, R = np.array(rig["intrinsic1"]), np.array(rig["R"])
    c = R.dot(np.linalg.inv(K1)).dot([u, v, 1.0])[2]
    z = -rig["T"][2] / c
    cands = [z]
    lo = hi = z
    for _ in range(4096):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cands += [lo, hi]
    for cand in cands:
        g, _ = C.geometry(rig, float(cand), PERIOD)
        with np.errstate(all="ignore"):
            if C.project_points(g, float(u), float(v))[2] == 0.0:
                return float(cand), g
    raise AssertionError("no z_plane with Z' == 0 found")


def main():
    arrays, meta = {}, {"period": PERIOD, "reference": {}, "cloud": {}}
    for name, (rig, roi, fringe, z_plane) in REFERENCE.items():
        entry = {"rig": rig, "roi": list(roi), "fringe": fringe if isinstance(fringe, str) else list(fringe), "z_plane": z_plane}
        if name == "nonfinite":
            y, x = NONFINITE_PIXEL
            z_plane, g = zero_depth_plane(rig, roi[0] + x, roi[1] + y)
            entry.update(z_plane=z_plane, pixel=[y, x])
            arrays[name + "__geom"] = g
            gray = np.max(S.build_fringe(PERIOD, stripeColor="r"), axis=2)
            mx, my = S.projector_map(g, *roi)
            assert not np.isfinite(mx[y, x]) or not np.isfinite(my[y, x])
            assert S.reference_image(gray, g, *roi)[y, x] == 0
        meta["reference"][name] = entry

    fringe = S.build_fringe(PERIOD, stripeColor="r")
    for name, (dist1, roi) in {"full": ([0.0] * 5, None), "roi": ([0.0] * 5, (17, 5, 127, 39)), "roi_camera_dist": (CAMERA_DIST, (17, 5, 127, 39))}.items():
        rig = scene_rig(dist1)
        frame = S.render(rig, PERIOD)
        mine = S.pipeline(rig, fringe, PERIOD, frame, roi)
        truth = S.pipeline(rig, fringe, PERIOD, frame, roi, phase_of=lambda *a: P.truth_longdouble(*a)[0])
        _, ratio = P.truth_longdouble(mine["undistorted"], mine["ref"], mine["fc"], 0.5)
        keep = ratio >= KEEP_RATIO
        assert keep.mean() >= MIN_KEPT, (name, float(keep.mean()))
        assert mine["k"] == truth["k"] and np.isfinite(mine["cloud"]).all() and np.isfinite(truth["cloud"]).all()
        numpy_err = float(C.rel_err(mine["cloud"], truth["cloud"])[keep].max())
        tol = TOL_FACTOR * max(numpy_err, TOL_FLOOR)
        arrays[name + "__frame"] = frame
        arrays[name + "__keep"] = np.packbits(keep)
        meta["cloud"][name] = {"rig": rig, "roi": None if roi is None else list(roi), "radius_factor": 0.5, "numpy_err": numpy_err, "tol": tol,
                               "kept": float(keep.mean()), "k": mine["k"], "z_plane": float(mine["z_plane"])}
        print("%-16s kept %.3f  numpy_err %.3e  tol %.3e  k %g  z_plane %.3f  z %.1f .. %.1f" %
              (name, keep.mean(), numpy_err, tol, mine["k"], mine["z_plane"], mine["cloud"][..., 2].min(), mine["cloud"][..., 2].max()))
    np.savez_compressed(os.path.join(HERE, "stereo_ftp_cases.npz"), **arrays)
    with open(os.path.join(HERE, "stereo_ftp_cases.json"), "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
