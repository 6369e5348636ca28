"""Writes tests/golden/ftp_cloud_cases.npz / ftp_cloud_cases.json: rigs, their packed geometry, unwrapped phase maps, the extended-precision truth of
their point clouds (tests/_ftp_cloud_ref.cloud_from_geometry in np.longdouble), the fp64 numpy restatement's own worst relative
error against that truth and the tolerance derived from it.  Run from the repository root:
    python tests/golden/make_golden_ftp_cloud.py

Tolerance of a case: 16 * max(numpy_err, 2**-52), numpy_err = max over the pixels of ||p - truth|| / ||truth||: what the
reference's own fp64 arithmetic allows itself, times the project's headroom for another operation order; the floor is one ulp.

Every case is asserted to be well conditioned, so that rounding is not amplified: the truth's disparity is at least 0.05 of the
case's maximum at every pixel, the projector column is at least 100 px from the epipole, and the reference plane is in front of
the projector (Z' > 0).  A wrong matrix, a missing +0.5 or four iterations instead of five is then off by many orders more
than the tolerance (main() measures the last two and asserts it).

The 65537-row case is not stored (4.7 MB of points): its phase is _ftp_cloud_ref.tall_phase and the test computes the truth;
its numpy_err and tolerance are measured here like the others.

The `special` pixels of the case "nonfinite" are excluded from the conditioning and the error: one holds NaN, the other a
phase found here by bisection for which the fp64 restatement's disparity is exactly 0."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _ftp_cloud_ref as R                                   # noqa: E402

TOL_FACTOR = 16.0
TOL_FLOOR = 2.0 ** -52
MIN_DISPARITY_RATIO = 0.05
MIN_EPIPOLE_DISTANCE = 100.0
Z_PLANE = 1000.0
PERIOD = 12.0

# name: (h, w, roi origin (x, y), distortion, k, phase, rig keywords)
CASES = {
    "p1x1": (1, 1, (640, 360), "d5", 0, "smooth", {}),
    "p1x5": (1, 5, (0, 0), "d5", 0, "smooth", {}),                           # odd width: the tail of two pixels per thread
    "p3x64": (3, 64, (0, 0), "d5", 0, "smooth", {}),                         # 192 pixels: whole waves
    "p3x130": (3, 130, (0, 0), "d5", 0, "smooth", {}),                       # a wave and a ragged tail
    "p5x257_roi": (5, 257, (37, 11), "d5", 1, "smooth", {}),                 # 1285 pixels: several workgroups, odd count
    "tall_65537x3": (65537, 3, (0, 0), "none", 0, "tall", {"res1": (3, 65537), "k1_fy": 150000.0, "cy1": 32768.0}),
    "dist_none": (6, 33, (2, 1), "none", 0, "smooth", {}),                   # the camera corner farthest from the projector axis
    "dist_d4": (6, 33, (2, 1), "d4", 0, "smooth", {}),
    "dist_d5": (6, 33, (2, 1), "d5", 0, "smooth", {}),
    "dist_d8": (6, 33, (2, 1), "d8", 0, "smooth", {}),
    "dist_d12": (6, 33, (2, 1), "d12", 0, "smooth", {}),
    "k_minus3": (4, 70, (300, 200), "d8", -3, "smooth", {}),
    "steep_ramp": (4, 200, (500, 100), "d12", 0, "ramp", {}),
    "nonfinite": (5, 66, (600, 300), "d5", 0, "smooth", {}),
}
NAN_PIXEL = (1, 7)                                           # (y, x) of the case "nonfinite"
ZERO_PIXEL = (3, 40)


def zero_disparity_phase(g, k, x, y):
    """A phase for which the fp64 restatement's disparity at camera pixel (x, y) is exactly 0."""
    def signed(ph):
        return float(R.cloud_from_geometry(g, np.array([[ph]]), k, x, y, details=True)[1]["signed"][0, 0])
    lo, hi = -2000.0, 2000.0
    flo, fhi = signed(lo), signed(hi)
    assert flo * fhi < 0, (flo, fhi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        fm = signed(mid)
        if fm == 0.0:
            return mid
        if (fm < 0) == (flo < 0):
            lo, flo = mid, fm
        else:
            hi, fhi = mid, fm
        if np.nextafter(lo, hi) >= hi:
            break
    ph = lo
    for _ in range(100000):                                   # neighbouring doubles of the crossing
        if signed(ph) == 0.0:
            return ph
        ph = np.nextafter(ph, np.inf)
    raise AssertionError("no phase with a disparity of exactly 0 near %r" % lo)


def make_case(name):
    h, w, (x0, y0), dist, k, kind, rig_kw = CASES[name]
    seed = sorted(CASES).index(name) + 1
    rig = R.rig_params(dist=dist, **rig_kw)
    g, _ = R.geometry(rig, Z_PLANE, PERIOD)
    phase = {"smooth": lambda: R.smooth_phase(h, w, seed=seed), "ramp": lambda: R.steep_ramp(h, w),
             "tall": lambda: R.tall_phase(h, w)}[kind]()
    special = []
    if name == "nonfinite":
        phase[NAN_PIXEL] = np.nan
        phase[ZERO_PIXEL] = zero_disparity_phase(g, k, x0 + ZERO_PIXEL[1], y0 + ZERO_PIXEL[0])
        special = [list(NAN_PIXEL), list(ZERO_PIXEL)]
    return rig, g, phase, float(k), (x0, y0, w, h), special


def main():
    arrays, meta = {}, {}
    for name in CASES:
        rig, g, phase, k, roi, special = make_case(name)
        x0, y0, w, h = roi
        truth, det = R.cloud_from_geometry(g, phase, k, x0, y0, dtype=np.longdouble, details=True)
        mine = R.cloud_from_geometry(g, phase, k, x0, y0)
        keep = np.ones((h, w), dtype=bool)
        for y, x in special:
            keep[y, x] = False
            assert not np.isfinite(mine[y, x]).any(), (name, y, x, mine[y, x])
        assert np.isfinite(mine[keep]).all() and np.isfinite(truth[keep]).all(), name
        disp = det["disparity"][keep]
        assert disp.min() >= MIN_DISPARITY_RATIO * disp.max(), (name, float(disp.min()), float(disp.max()))
        assert np.abs(det["Xa"] - g[37]).min() >= MIN_EPIPOLE_DISTANCE, name
        assert det["Zp"].min() > 0, name
        numpy_err = float(R.rel_err(mine, truth)[keep].max())
        tol = TOL_FACTOR * max(numpy_err, TOL_FLOOR)
        # what the tolerance tells apart: four iterations instead of five, and pixel corners instead of centres
        four = float(R.rel_err(R.cloud_from_geometry(g, phase, k, x0, y0, iterations=4), truth)[keep].max())
        corner = float(R.rel_err(R.cloud_from_geometry(g, phase, k, x0 - 0.5, y0 - 0.5), truth)[keep].max())
        if rig["distCoeffs2"]:
            assert four > 1e3 * tol, (name, four, tol)
        assert corner > 1e3 * tol, (name, corner, tol)
        arrays[name + "__geom"] = g                          # an input: matrix products and inverses differ in the last bit between BLAS builds
        stored = h * w <= 4096
        if stored:
            arrays[name + "__phase"], arrays[name + "__truth"] = phase, truth.astype(np.float64)
            # the stored truth is the longdouble truth rounded to fp64: half an ulp, inside the floor of the tolerance
        meta[name] = {"shape": [h, w], "roi": [x0, y0, w, h], "k": k, "z_plane": Z_PLANE, "period": PERIOD, "rig": rig,
                      "stored": stored, "special": special, "numpy_err": numpy_err, "tol": tol,
                      "min_disparity_ratio": float(disp.min() / disp.max()), "four_iterations_err": four,
                      "corner_instead_of_centre_err": corner}
        print("%-14s %5d x %3d  dist %-2d  depth %7.1f .. %7.1f  disparity ratio %.2f  numpy_err %.2e  tol %.2e  4 it. %.1e  no +0.5 %.1e" %
              (name, h, w, len(rig["distCoeffs2"]), float(truth[keep][:, 2].min()), float(truth[keep][:, 2].max()),
               disp.min() / disp.max(), numpy_err, tol, four, corner))
    np.savez_compressed(os.path.join(HERE, "ftp_cloud_cases.npz"), **arrays)
    with open(os.path.join(HERE, "ftp_cloud_cases.json"), "w") as f:
        json.dump({"tol_factor": TOL_FACTOR, "tol_floor": TOL_FLOOR, "min_disparity_ratio": MIN_DISPARITY_RATIO,
                   "min_epipole_distance": MIN_EPIPOLE_DISTANCE, "cases": meta}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
