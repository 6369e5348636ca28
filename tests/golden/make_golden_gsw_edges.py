#!/usr/bin/env python3
"""Record what the UNMODIFIED reference's computeGSW answers at the edges of its parameters.

Run where the reference sources are (oracle/Makefile builds them, where they lie, into oracle/_ref):

    make -C oracle ref && python tests/golden/make_golden_gsw_edges.py

Writes ``gsw_edge_cases.json`` (per case: input, parameters, sha256 of the input pair and of the map) and
``gsw_edge_cases.npz`` (one int16 map per case).  The inputs are generated (``inputs()`` below), not stored.  The reference
returns only the map after its left-right check and filling, so that is what is recorded;
``tests/test_oracle_golden_gsw_edges.py`` holds the oracle to every map, which is what licenses the oracle's RAW winners
as the standard of ``tests/test_gpu_gsw_raw.py``.

The parameter sets: a negative ``gamma`` turns every support weight the relaxation never reaches into
exp(+inf) = inf (gammas -1 .. -4 overflow reached weights as well: expf(dist / 4) is inf beyond dist = 355);
``gamma`` = 1 / 1000 are the steepest and the flattest positive tables; ``fMax`` = 0, -0.0 and a subnormal make every
cost (nearly) zero, +inf never caps, a negative cap makes every cost negative, a NaN cap makes every cost NaN
(std::min(fMax, e) returns fMax unless e < fMax).  ``fMax`` is kept as text ("nan", "inf", "-0.0"): JSON has no such numbers.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

OUT = os.path.dirname(os.path.abspath(__file__))
BASE = dict(winSize=5, maxDisparity=9, minDisparity=0, gamma=10, fMax="120.0", iterations=3, bins=20)


def inputs():
    """{name: (left, right)}: generated, the same arrays wherever this runs"""
    from simplestereo_amd.synth import make_pair
    a, b, _ = make_pair(20, 48, 12, 3)
    rng = np.random.default_rng(21)
    na = rng.integers(0, 256, (16, 40, 3), dtype=np.uint8)
    nb = rng.integers(0, 256, (16, 40, 3), dtype=np.uint8)
    return {"synth_20x48": (a, b), "noise_16x40": (na, nb)}


RECIPES = {"synth_20x48": "simplestereo_amd.synth.make_pair(20,48,12,seed=3)",
           "noise_16x40": "rng = np.random.default_rng(21); left, right = rng.integers(0,256,(16,40,3),dtype=uint8) twice"}


def parameter_sets():
    sets = {}
    for g in (-7, -5, -4, -1, 1, 1000):
        sets["gamma_%d" % g] = dict(BASE, gamma=g)
    for name, f in (("zero", "0.0"), ("minus_zero", "-0.0"), ("inf", "inf"), ("subnormal", "1e-40"), ("minus_5", "-5.0"), ("nan", "nan")):
        sets["fmax_" + name] = dict(BASE, fMax=f)
    sets["gamma_-7_iterations_0"] = dict(BASE, gamma=-7, iterations=0)
    sets["gamma_-7_win_11_d_16"] = dict(BASE, gamma=-7, winSize=11, maxDisparity=16)
    return sets


def main():
    from oracle import oracle
    ref = oracle.ref_module()
    if ref is None:
        raise SystemExit("oracle/_ref is not built: run `make -C oracle ref` first")
    maps, meta = {}, {}
    for iname, (a, b) in inputs().items():
        for pname, p in parameter_sets().items():
            cid = iname + "__" + pname
            d = ref.computeGSW(a, b, p["winSize"], p["maxDisparity"], p["minDisparity"], p["gamma"], float(p["fMax"]),
                               p["iterations"], p["bins"])
            again = ref.computeGSW(a, b, p["winSize"], p["maxDisparity"], p["minDisparity"], p["gamma"], float(p["fMax"]),
                                   p["iterations"], p["bins"])
            assert d.dtype == np.int16 and d.shape == a.shape[:2] and np.array_equal(d, again), cid
            maps[cid] = d
            meta[cid] = dict(input=iname, recipe=RECIPES[iname], params=p, shape=list(d.shape),
                             sha256=hashlib.sha256(d.tobytes()).hexdigest(),
                             input_sha256=hashlib.sha256(a.tobytes() + b.tobytes()).hexdigest())
            print("%-40s %s min %d max %d" % (cid, meta[cid]["sha256"][:16], d.min(), d.max()), flush=True)
    np.savez_compressed(os.path.join(OUT, "gsw_edge_cases.npz"), **maps)
    with open(os.path.join(OUT, "gsw_edge_cases.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
