"""Writes tests/golden/ftp_mapping_cases.{npz,json}: the cases of tests/test_gpu_ftp_mapping.py.  Run from the repository root:
    python tests/golden/make_golden_ftp_mapping.py

Everything comes from the numpy restatements (tests/_ftp_mapping_ref.py and the files it imports); nothing here imports
simplestereo_amd or runs a kernel.

"carrier" cases (ss.active.ftpCarrierPhase): one seeded fringe image each, the extended-precision truth of its phase
(carrier_truth_longdouble; for the wide cases the test computes it, it is too large to store), numpy's own worst angle error
against that truth and the tolerance 16 * max(numpy_err, pi * 2**-52) -- the rule of make_golden_ftp.py.  Every case is asserted
to be well conditioned: |ghat| of the truth is at least 0.01 of its row's maximum at every pixel.

"cloud" cases (ss.active.StereoFTP_Mapping.getCloud, StereoFTP_PhaseOnly.getPhase): the rendered 48 x 160 frames of
make_golden_stereo_ftp.py's scene -- whole frame, an roi at a non-zero origin, lens distortion on the camera.  Per case, on numpy
alone: numpy_err, the worst relative error of a point between pipeline_mapping and the same pipeline fed the np.longdouble
phase, and tol = 16 * max(numpy_err, 2**-52).  Both pipelines are asserted to unwrap identically (the unwrapped maps differ by
less than 1e-9 everywhere: no 2 pi decision flips)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ftp_cloud_ref as C          # noqa: E402
import _ftp_mapping_ref as M        # noqa: E402
import _ftp_ref as P                # noqa: E402
import _stereo_ftp_ref as S         # noqa: E402
from make_golden_stereo_ftp import CAMERA_DIST, PERIOD, scene_rig      # noqa: E402
from make_golden_ftp import to_bgr  # noqa: E402

MAX_WIDTH = 8192
MIN_RATIO = 0.01
TOL_FACTOR = 16.0
TOL_FLOOR = float(np.pi * 2.0 ** -52)
CLOUD_FLOOR = 2.0 ** -52
STORE_TRUTH_UP_TO = 1024            # columns


def fringe(h, w, fc, seed, amp=70.0, noise=3):
    """One fringe image (uint8 [h, w]): 128 + amp cos(2 pi fc x + bump) +- noise; bump is a smooth hill of 1.5 rad."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    bump = 1.5 * np.exp(-(((x - w / 2) / (w / 4 + 1)) ** 2 + ((y - h / 2) / (h / 2 + 1)) ** 2))
    f = np.broadcast_to(np.asarray(fc, dtype=np.float64).reshape(-1, 1), (h, 1))
    img = 128 + amp * np.cos(2 * np.pi * f * x + bump) + rng.integers(-noise, noise + 1, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# name: (h, w, fc, radius_factor, channels[, the number of bins every row must keep])
CARRIER = {
    "w1": (1, 1, 0.0, 0.5, 1),                               # the only bin is s = 0
    "w2_both_bins": (1, 2, 0.25, 3.0, 1),                    # fmin = -0.5 is the Nyquist bin s = -1 itself
    "w3": (2, 3, 0.3, 0.5, 1),
    "w63_fc_per_row": (5, 63, [0.09, 0.1, 0.11, 0.1, 0.12], 0.5, 1),
    "w64_edges_on_bins": (4, 64, 0.125, 0.5, 1, 9),          # fmin = 4/64 and fmax = 12/64 exactly
    "w65": (3, 65, 0.1, 0.5, 1),
    "w257": (3, 257, 0.08, 0.5, 1),
    "w257_all_bins": (2, 257, 0.1, 10.0, 1, 257),            # [-0.9, 1.1]: negative bins and DC included
    "bgr": (3, 100, 0.1, 0.5, 3),
    "empty_middle_row": (3, 256, [0.125, 0.0019, 0.125], 0.04, 1),
    "bins_128": (2, 700, 83.5 / 700, 64 / 83.5, 1, 128),     # bins 20 .. 147: one chunk exactly
    "bins_129": (2, 700, 84.0 / 700, 64.25 / 84.0, 1, 129),  # bins 20 .. 148: a chunk and one bin
    "cpt2_w1025": (2, 1025, 0.05, 0.1, 1),
    "cpt4_w2049": (2, 2049, 0.05, 0.05, 1),
    "cpt8_w4097": (2, 4097, 0.05, 0.03, 1),
    "cpt8_w8192": (2, MAX_WIDTH, 0.05, 0.02, 1),
}


def make_carrier(name):
    h, w, fc, rf, ch = CARRIER[name][:5]
    seed = sorted(CARRIER).index(name) + 1
    img = fringe(h, w, fc, seed)
    if ch == 3:
        img = to_bgr(img, 100 + seed)
    return img, np.broadcast_to(np.asarray(fc, dtype=np.float64), (h,)).copy(), float(rf)


SCENES = {"full": ([0.0] * 5, None), "roi": ([0.0] * 5, (17, 5, 127, 39)), "roi_camera_dist": (CAMERA_DIST, (17, 5, 127, 39))}


def main():
    arrays, meta = {}, {}
    for name in CARRIER:
        img, fc, rf = make_carrier(name)
        truth, ratio = M.carrier_truth_longdouble(img, fc, rf)
        assert ratio.min() >= MIN_RATIO, (name, float(ratio.min()))
        h, w = truth.shape
        lo, hi = P.band_ranges(w, *P.band(fc, rf, h))
        if len(CARRIER[name]) > 5:
            assert (hi - lo + 1 == CARRIER[name][5]).all(), (name, lo, hi)
        numpy_err = float(P.wrap_err(M.carrier_phase_numpy(img, fc, rf), truth).max())
        stored = w <= STORE_TRUTH_UP_TO
        arrays[name + "__img"], arrays[name + "__fc"] = img, fc
        if stored:
            arrays[name + "__truth"] = truth
        meta[name] = {"shape": [h, w], "radius_factor": rf, "channels": CARRIER[name][4], "stored": stored,
                      "slo": [int(v) for v in lo], "shi": [int(v) for v in hi], "min_ratio": float(ratio.min()),
                      "numpy_err": numpy_err, "tol": TOL_FACTOR * max(numpy_err, TOL_FLOOR)}
        print("%-20s %4d x %4d  bins %s  min|ghat|/rowmax %.3f  numpy_err %.2e  tol %.2e" %
              (name, h, w, [int(b - a + 1) for a, b in zip(lo, hi)][:3], ratio.min(), numpy_err, meta[name]["tol"]))

    clouds = {}
    fr = S.build_fringe(PERIOD, stripeColor="r")
    for name, (dist1, roi) in SCENES.items():
        rig = scene_rig(dist1)
        frame = S.render(rig, PERIOD)
        mine = M.pipeline_mapping(rig, fr, PERIOD, frame, roi)
        truth = M.pipeline_mapping(rig, fr, PERIOD, frame, roi, phase_of=lambda *a: M.carrier_truth_longdouble(*a)[0])
        unwrap_diff = float(np.abs(mine["phase"] - truth["phase"]).max())
        assert unwrap_diff < 1e-9, (name, unwrap_diff)
        assert np.isfinite(mine["cloud"]).all() and np.isfinite(truth["cloud"]).all()
        numpy_err = float(C.rel_err(mine["cloud"], truth["cloud"].astype(np.longdouble)).max())
        tol = TOL_FACTOR * max(numpy_err, CLOUD_FLOOR)
        arrays["cloud_" + name + "__frame"] = frame
        clouds[name] = {"rig": rig, "roi": None if roi is None else list(roi), "radius_factor": 0.5, "numpy_err": numpy_err, "tol": tol,
                        "unwrap_diff": unwrap_diff, "theta_shift": mine["theta_shift"]}
        z = mine["cloud"][..., 2]
        print("%-16s numpy_err %.3e  tol %.3e  unwrapped maps differ by %.2e  theta %.4f  z %.1f .. %.1f" %
              (name, numpy_err, tol, unwrap_diff, mine["theta_shift"], z.min(), z.max()))
    np.savez_compressed(os.path.join(HERE, "ftp_mapping_cases.npz"), **arrays)
    with open(os.path.join(HERE, "ftp_mapping_cases.json"), "w") as f:
        json.dump({"tol_factor": TOL_FACTOR, "tol_floor": TOL_FLOOR, "cloud_floor": CLOUD_FLOOR, "min_ratio": MIN_RATIO,
                   "max_width": MAX_WIDTH, "period": PERIOD, "carrier": meta, "cloud": clouds}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
