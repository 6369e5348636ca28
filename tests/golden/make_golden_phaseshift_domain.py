"""Writes tests/golden/phaseshift_domain_cases.json: the tolerances of the phase-shift decode on its whole input domain (the
511 x 511 grid of P.domain_stack, one period per axis) and on seeded uniform-noise stacks, where the heterodyne step meets exact
ties.  CPU only, numpy only, no input from outside the repository; run from the repository root:

    python tests/golden/make_golden_phaseshift_domain.py

No npz: the stacks are rebuilt from P.domain_stack and P.noise_stack (the seeds are in the json).  Nothing here imports
simplestereo_amd or runs a kernel.

Tolerances, by the rule of make_golden_phaseshift.py, unchanged:
  numpy_err : the worst |p - p_longdouble| of the fp64 restatement over the unmasked, non-flagged pixels (both coordinates)
  tol       = 16 * max(numpy_err, proj_extent * 2^-52), proj_extent the larger projector side
A pixel is FLAGGED if at any heterodyne step of either axis the fp64 restatement has |kk - rint(kk)| > 0.5 - BAND: its k hangs
on the last bit of arctan2, and fp64, long double and the device may each take the other neighbour.  BAND = 1e-9 is derived: two
evaluations of kk differ by the decode tolerance in phase units times the largest T0 / T, about 1e-12 * 2 pi / 1080 * 64 < 1e-12,
and 1e-9 is a thousand times that.  The grid has no heterodyne step and no flagged pixel.
Asserted, not measured -- conditions of the noise cases, which the seeds are chosen to meet:
  * the flagged count at BAND equals the count at 1e-12 (the pixels sit ON the tie: no status hangs on the band);
  * 1 <= flagged <= pixels / 2000;
  * long double and fp64 agree within 1e-9 on every non-flagged pixel;
  * on every flagged pixel the long-double result is within tol of a member of P.candidates (every tied step branched both ways).
Recorded for information: how many flagged pixels long double decodes a whole period away from fp64 (ld_other_k), and the largest
candidate set."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import _phaseshift_ref as P         # noqa: E402

TOL_FACTOR, FLOOR, TIGHT_BAND, AGREE, MAX_FLAGGED_SHARE = 16.0, 2.0 ** -52, 1e-12, 1e-9, 1.0 / 2000
GRID_EXTENTS = [(1, 1), (64, 32), (1920, 1080), (65536, 65536)]
NOISE_SEEDS = {"readme": 1, "small": 1, "ratios": 7, "eight": 1}          # ratios: seed 1 meets no tie


def tol_of(numpy_err, extent):
    return TOL_FACTOR * max(numpy_err, max(extent) * FLOOR)


def grid_case(stack, extent):
    d64 = P.decode(stack, P.DOMAIN_PERIODS, extent)
    dld = P.decode(stack, P.DOMAIN_PERIODS, extent, dtype=np.longdouble)
    assert np.isfinite(d64).all() and (d64 >= 0).all() and (d64[..., 0] < extent[0]).all() and (d64[..., 1] < extent[1]).all()
    numpy_err = float(np.abs(d64.astype(np.longdouble) - dld).max())
    return {"extent": list(extent), "periods": P.DOMAIN_PERIODS, "numpy_err": numpy_err, "tol": tol_of(numpy_err, extent), "flagged": 0}


def noise_case(name, seed):
    periods = P.NOISE_PERIODS[name]
    stack = P.noise_stack(seed, periods)
    d64, tie = P.decode(stack, periods, P.NOISE_PROJ, details=True)
    dld = P.decode(stack, periods, P.NOISE_PROJ, dtype=np.longdouble)
    flagged = tie > 0.5 - P.BAND
    n = int(flagged.sum())
    assert n == int((tie > 0.5 - TIGHT_BAND).sum()), (name, n)
    assert 1 <= n <= flagged.size * MAX_FLAGGED_SHARE, (name, n)
    err = np.abs(d64.astype(np.longdouble) - dld).max(axis=-1)
    assert err[~flagged].max() <= AGREE, (name, float(err[~flagged].max()))
    numpy_err = float(err[~flagged].max())
    tol = tol_of(numpy_err, P.NOISE_PROJ)
    dist, largest = P.distance_to_candidates(dld, stack, periods, P.NOISE_PROJ, flagged)
    assert dist.max() <= tol, (name, float(dist.max()), tol)
    return {"seed": seed, "periods": periods, "extent": list(P.NOISE_PROJ), "shape": list(P.NOISE_SHAPE), "numpy_err": numpy_err, "tol": tol,
            "flagged": n, "ld_other_k": int((err[flagged] > tol).sum()), "largest_candidate_set": largest,
            "ld_to_candidates": float(dist.max())}


def main():
    meta = {"tol_factor": TOL_FACTOR, "floor": FLOOR, "band": P.BAND, "tight_band": TIGHT_BAND, "agree": AGREE, "max_flagged_share": MAX_FLAGGED_SHARE,
            "numpy_err_of": "the fp64 restatement against the same chain in np.longdouble, non-flagged pixels", "grid": {}, "noise": {}}
    stack = P.domain_stack()
    a, b = P.domain_pairs()
    meta["distinct_theta"] = int(np.unique(np.mod(np.arctan2(a.astype(np.float64), b.astype(np.float64)), 2 * np.pi)).size)
    for extent in GRID_EXTENTS:
        c = meta["grid"]["%dx%d" % extent] = grid_case(stack, extent)
        print("grid  %-12s numpy_err %.3e  tol %.3e" % ("%dx%d" % extent, c["numpy_err"], c["tol"]))
    print("grid: %d distinct theta among %d pairs" % (meta["distinct_theta"], a.size))
    for name, seed in NOISE_SEEDS.items():
        c = meta["noise"][name] = noise_case(name, seed)
        print("noise %-12s seed %d  numpy_err %.3e  tol %.3e  flagged %d of %d (long double a period away on %d; sets of at most %d, long "
              "double within %.3e of one)" % (name, seed, c["numpy_err"], c["tol"], c["flagged"], P.NOISE_SHAPE[0] * P.NOISE_SHAPE[1],
                                             c["ld_other_k"], c["largest_candidate_set"], c["ld_to_candidates"]))
    assert "simplestereo_amd" not in sys.modules
    with open(P.DOMAIN_JSON, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s" % os.path.relpath(P.DOMAIN_JSON))


if __name__ == "__main__":
    main()
