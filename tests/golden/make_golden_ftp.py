"""Writes tests/golden/ftp_cases.npz / ftp_cases.json: fringe image pairs, the extended-precision truth of their
Fourier-profilometry phase (tests/_ftp_ref.truth_longdouble), numpy's own worst angle error against that truth and the
tolerance derived from it.  Run from the repository root:  python tests/golden/make_golden_ftp.py

Tolerance of a case: 16 * max(numpy_err, pi * 2**-52).  numpy's error is what the reference's own arithmetic allows itself;
the floor is one ulp of pi, the scale of an angle; 16 is headroom for another summation order and another atan2.  A wrong
bin, a wrong twiddle index or a missing conjugate is off by more than 1e-3.

Every case is asserted to be well conditioned: |ghat * conj(g0hat)| of the truth is at least 0.01 of its row's maximum at
every pixel, so the angle does not amplify rounding."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ftp_ref                                      # noqa: E402

MAX_WIDTH = 8192                                     # SSAMD_FTP_MAX_W
MIN_RATIO = 0.01
TOL_FACTOR = 16.0
TOL_FLOOR = float(np.pi * 2.0 ** -52)


def fringes(h, w, fc, seed, amp=70.0, noise=3):
    """Object and reference fringe images (uint8 [h, w]): 128 + amp cos(2 pi fc x + bump) +- noise against
    128 + amp cos(2 pi fc x); bump is a smooth hill of 1.5 rad."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    bump = 1.5 * np.exp(-(((x - w / 2) / (w / 4)) ** 2 + ((y - h / 2) / (h / 2 + 1)) ** 2))
    f = np.broadcast_to(np.asarray(fc, dtype=np.float64).reshape(-1, 1), (h, 1))
    obj = 128 + amp * np.cos(2 * np.pi * f * x + bump) + rng.integers(-noise, noise + 1, (h, w))
    ref = 128 + amp * np.cos(2 * np.pi * f * x)
    to_u8 = lambda a: np.clip(np.rint(a), 0, 255).astype(np.uint8)      # noqa: E731
    return to_u8(obj), to_u8(ref)


def to_bgr(gray, seed):
    """[h, w, 3] whose channel maximum is `gray`, the maximum sitting in a channel that changes from pixel to pixel."""
    rng = np.random.default_rng(seed)
    h, w = gray.shape
    img = (gray[..., None].astype(np.int64) - rng.integers(1, 60, (h, w, 3))).clip(0, 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    where = (x + 2 * y + 1) % 3
    np.put_along_axis(img, where[..., None], gray[..., None], axis=2)
    assert np.array_equal(img.max(axis=2), gray) and (where != 0).any()
    return img


# name: (h, w, fc, radius_factor, channels of obj, channels of ref)
CASES = {
    "w1": (1, 1, 0.0, 0.5, 1, 1),                            # the only bin is s = 0
    "w2_both_bins": (1, 2, 0.25, 3.0, 1, 1),                 # fmin = -0.5 is the Nyquist bin s = -1 itself
    "w3": (2, 3, 0.3, 0.5, 1, 1),
    "w16": (3, 16, 0.25, 0.5, 1, 1),
    "w63_fc_per_row": (5, 63, [0.09, 0.1, 0.11, 0.1, 0.12], 0.5, 1, 1),
    "w64_edges_on_bins": (4, 64, 0.125, 0.5, 1, 1),          # fmin = 4/64 and fmax = 12/64 exactly
    "w97": (3, 97, 0.1, 0.5, 1, 1),
    "w257": (3, 257, 0.08, 0.5, 1, 1),
    "w1000": (4, 1000, 0.05, 0.5, 1, 1),
    "w256_wide_band": (3, 256, 0.0625, 0.9, 1, 1),
    "w257_all_bins": (2, 257, 0.1, 10.0, 1, 1),              # [-0.9, 1.1]: negative bins and DC included
    "bgr": (3, 100, 0.1, 0.5, 3, 3),
    "gray_vs_bgr": (2, 80, 0.1, 0.5, 1, 3),
    "empty_middle_row": (3, 256, [0.125, 0.0019, 0.125], 0.04, 1, 1),
    "max_width": (2, MAX_WIDTH, 0.05, 0.02, 1, 1),
}


def make_case(name):
    h, w, fc, rf, ch_obj, ch_ref = CASES[name]
    seed = sorted(CASES).index(name) + 1
    obj, ref = fringes(h, w, fc, seed)
    if ch_obj == 3:
        obj = to_bgr(obj, 100 + seed)
    if ch_ref == 3:
        ref = to_bgr(ref, 200 + seed)
    return obj, ref, np.broadcast_to(np.asarray(fc, dtype=np.float64), (h,)).copy(), float(rf)


def main():
    arrays, meta = {}, {}
    for name in CASES:
        obj, ref, fc, rf = make_case(name)
        truth, ratio = _ftp_ref.truth_longdouble(obj, ref, fc, rf)
        assert ratio.min() >= MIN_RATIO, (name, float(ratio.min()))
        h, w = truth.shape
        lo, hi = _ftp_ref.band_ranges(w, *_ftp_ref.band(fc, rf, h))
        numpy_err = float(_ftp_ref.wrap_err(_ftp_ref.ftp_phase_numpy(obj, ref, fc, rf), truth).max())
        arrays[name + "__obj"], arrays[name + "__ref"], arrays[name + "__fc"], arrays[name + "__truth"] = obj, ref, fc, truth
        meta[name] = {"shape": [h, w], "radius_factor": rf, "channels": [CASES[name][4], CASES[name][5]],
                      "slo": [int(v) for v in lo], "shi": [int(v) for v in hi], "min_ratio": float(ratio.min()),
                      "numpy_err": numpy_err, "tol": TOL_FACTOR * max(numpy_err, TOL_FLOOR)}
        print("%-20s %4d x %4d  bins %s  min|z|/rowmax %.3f  numpy_err %.2e  tol %.2e" %
              (name, h, w, [int(b - a + 1) for a, b in zip(lo, hi)][:3], ratio.min(), numpy_err, meta[name]["tol"]))
    np.savez_compressed(os.path.join(HERE, "ftp_cases.npz"), **arrays)
    with open(os.path.join(HERE, "ftp_cases.json"), "w") as f:
        json.dump({"tol_factor": TOL_FACTOR, "tol_floor": TOL_FLOOR, "min_ratio": MIN_RATIO, "max_width": MAX_WIDTH,
                   "cases": meta}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
