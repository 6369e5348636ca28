"""Record the launch planner's decisions (tile, kernel form, LDS, grid) over a sweep of shapes and tuning options.

    python tests/golden/make_golden_plan.py [output directory, default: this one]

The planner is host-only integer / double arithmetic behind ``ssamd_asw_geometry``, ``ssamd_asw_kernel_form`` and
``ssamd_gsw_geometry``: no GPU is needed.  The library queried is the one ``simplestereo_amd._native`` loads -- the tree's own
``libssamd.so``, or another build of the same ABI named by ``SSAMD_LIB`` (with ``SSAMD_EXPERIMENT=1``), which is how the
committed fixture was taken from the commit BEFORE the planner moved into its own headers.

Writes ``plan_cases.json`` (the sweep: axes of the shapes, the option sets) and ``plan_cases.npz``:

    asw      int32 [ASW option set][shape][13]   the 8 integers of asw_geometry, then the 5 of asw_kernel_form
    asw_err  int32 [ASW option set][shape]       0, or the error code of a query that fails (its 13 integers are 0 then)
    gsw      int32 [GSW option set][shape][9]    gsw_geometry; shapes with winSize <= gsw_max_win only
    gsw_err  int32 [GSW option set][shape]

Shapes are the product W x rows x winSize x nD in the order of ``itertools.product`` (nD varies fastest), all with
minDisparity = 0.  ``tests/test_plan_cpu.py`` replays the sweep and wants every integer back.
"""
import itertools
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

SWEEP = {
    "W": [40, 96, 384, 640, 1920, 4096],
    "rows": [1, 10, 135, 1080],
    "win": [3, 9, 15, 35, 65, 255],
    "nD": [1, 4, 8, 17, 18, 21, 33, 49, 64, 65, 129, 193, 257, 531],
    "gsw_max_win": 65,
    "asw_options": [
        {},
        {"SSAMD_ASW_WAVE": "0"},
        {"SSAMD_ASW_WAVE": "0", "SSAMD_ASW_PIPE": "0"},
        {"SSAMD_ASW_PIPE": "8"},
        {"SSAMD_ASW_PIPE": "16"},
        {"SSAMD_ASW_EVOL": "0"},
        {"SSAMD_ASW_WAVE": "0", "SSAMD_ASW_PIPE": "0", "SSAMD_ASW_NO_E2": "1"},
        {"SSAMD_ASW_WAVE": "0", "SSAMD_ASW_PIPE": "0", "SSAMD_ASW_XOR_ONLY": "1"},
        {"SSAMD_ASW_WAVE_RX": "4"},
        {"SSAMD_ASW_WAVE_RX": "8"},
        {"SSAMD_ASW_WAVE_MERGE": "0"},
        {"SSAMD_ASW_WAVE_RD": "4"},
        {"SSAMD_ASW_WAVE_WG": "4"},
        {"SSAMD_ASW_DEPHASE": "0"},
        {"SSAMD_ASW_GEOM": "3,5,8", "SSAMD_ASW_WAVE": "0"},
        {"SSAMD_ASW_GEOM": "6,4,16,8", "SSAMD_ASW_WAVE": "0"},
        {"SSAMD_ASW_GEOM": "4,6,4,4", "SSAMD_ASW_WAVE": "0"},
        {"SSAMD_ASW_GEOM": "96,8", "SSAMD_ASW_WAVE": "0"},          # 768 columns: fails ("does not fit LDS") from winSize 9 on
    ],
    # (the forced shapes of tests/test_gpu_gsw.py::test_gsw_forced_geometries_and_strip_heights_agree)
    "gsw_options": [{}] + [{"SSAMD_GSW_GEOM": g} for g in
                           ("8,4,1", "8,4,2", "5,3,2", "16,2,1", "3,7,2", "8,4,2,2", "5,3,2,4", "3,7,2,2", "6,7,2,8",
                            "64,8,2,2")],          # (... and one that is refused: more threads than a workgroup has)
}


def shapes(sweep, max_win=None):
    return [s for s in itertools.product(sweep["W"], sweep["rows"], sweep["win"], sweep["nD"]) if max_win is None or s[2] <= max_win]


def replay(sweep, _native):
    """The four arrays of the fixture, from the library ``_native`` has loaded."""
    def run(option_sets, shape_list, query, width):
        val = np.zeros((len(option_sets), len(shape_list), width), np.int32)
        err = np.zeros((len(option_sets), len(shape_list)), np.int32)
        for i, opts in enumerate(option_sets):
            with _native.options(**opts):
                for k, (W, rows, win, nD) in enumerate(shape_list):
                    try:
                        val[i, k] = query(W, rows, win, nD - 1, 0)
                    except _native.NativeError as e:
                        err[i, k] = e.code
        return val, err

    def asw(*a):
        return list(_native.asw_geometry(*a).values()) + list(_native.asw_kernel_form(*a).values())

    def gsw(*a):
        return list(_native.gsw_geometry(*a).values())

    a, ae = run(sweep["asw_options"], shapes(sweep), asw, 13)
    g, ge = run(sweep["gsw_options"], shapes(sweep, sweep["gsw_max_win"]), gsw, 9)
    return {"asw": a, "asw_err": ae, "gsw": g, "gsw_err": ge}


def main(out_dir):
    from simplestereo_amd import _native
    arrays = replay(SWEEP, _native)
    np.savez_compressed(os.path.join(out_dir, "plan_cases.npz"), **arrays)
    with open(os.path.join(out_dir, "plan_cases.json"), "w") as f:
        json.dump(SWEEP, f, indent=1)
    forms = {tuple(r) for r in arrays["asw"][arrays["asw_err"] == 0][:, 8:].tolist()}
    print("library", _native.LIB_PATH)
    print("asw", arrays["asw"].shape, "failing", int((arrays["asw_err"] != 0).sum()), "kernel forms", len(forms))
    print("gsw", arrays["gsw"].shape, "failing", int((arrays["gsw_err"] != 0).sum()))


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE)
