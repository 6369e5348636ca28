"""Record the case matrix of the near-tie band measurement (tests/_asw_band_ref.py) with what the CPU knows about every case.

    python tests/golden/make_golden_asw_band.py [output directory, default: this one]

Writes ``asw_band_cases.json``: settings and recorded results only.  Per case: the input (generator, shape, seed), the matcher's
parameters, the kernel forms that run it, the band ``tol`` in cost-image ulps, the number of candidates measured, the plain fp32
emulation's per-candidate error against the fp64 oracle (``emu_E_max`` and ``emu_E_p999``, in cost-image ulps: the yardstick of
the GPU test's per-candidate bar; ``emu_E_max_above_zkey`` over the candidates above rule (d)'s floor ``zkey``), the number of
near pairs, how the emulation's images split them into the band and the floor class, and, for information, the emulation's own
worst differential error in each (``emu_D_max``, ``emu_D_max_floor``).  Needs the C oracle, no GPU.  Running it twice writes the same bytes; tests/test_asw_band_cpu.py recomputes
every figure."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import _asw_band_ref as B      # noqa: E402
import _tie_inputs as T        # noqa: E402

NAME = "asw_band_cases.json"


def record(name, oc):
    """the fixture's row of case `name`"""
    c = B.CASES[name]
    L, R, p = B.case_inputs(name)
    _, cost = oc.asw(L, R, return_costs=True, **p)
    tol = B.case_tol(name)
    emu = B.emulate32(L, R, p)
    zk = B.zkey(p["winSize"])
    e_max, e_p999, n = B.candidate_error(cost, emu)
    a_max, _, a_n = B.candidate_error(cost, emu, above=zk)
    d_max, band, f_max, floor = B.differential_error(cost, emu, tol, zk)
    pairs, _ = B.near_pairs(cost, tol)
    return dict(generator=c["generator"], shape=c["shape"], seed=c["seed"], params=c["params"], forms=c["forms"],
                differential=c["differential"], tol=tol, zkey=zk, measured=n, measured_above_zkey=a_n, emu_E_max=e_max,
                emu_E_p999=round(e_p999, 1), emu_E_max_above_zkey=a_max, near_pairs=int(pairs.sum()), emu_pairs_band=band,
                emu_pairs_floor=floor, emu_D_max=d_max, emu_D_max_floor=f_max)


def text():
    oc = T.OracleCache()
    return json.dumps({name: record(name, oc) for name in B.CASES}, indent=1, sort_keys=True) + "\n"


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else HERE
    with open(os.path.join(out, NAME), "w") as f:
        f.write(text())
    print("wrote", os.path.join(out, NAME))
