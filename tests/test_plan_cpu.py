"""The launch planner's decisions are pinned: tests/golden/plan_cases.npz holds what ssamd_asw_geometry, ssamd_asw_kernel_form
and ssamd_gsw_geometry answered, for a sweep of shapes under 18 ASW and 11 GSW option sets, BEFORE the planner moved out of
the library's host code, then all in ssamd_api.hip (tests/golden/make_golden_plan.py).  Host arithmetic only: no GPU."""
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_plan", os.path.join(GOLDEN, "make_golden_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def plan():
    with open(os.path.join(GOLDEN, "plan_cases.json")) as f:
        sweep = json.load(f)
    return sweep, dict(np.load(os.path.join(GOLDEN, "plan_cases.npz")))


def test_every_planner_decision_equals_the_recorded_one(plan):
    """each of the 13 (ASW) / 9 (GSW) integers of every query of the sweep, and the error code of every query that fails"""
    from simplestereo_amd import _native
    sweep, want = plan
    rec = _recorder()
    assert sweep == rec.SWEEP, "plan_cases.json is not the sweep of make_golden_plan.py"
    got = rec.replay(sweep, _native)
    assert sorted(got) == sorted(want)
    for name in sorted(want):
        assert got[name].shape == want[name].shape, name
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, "%s: %d integers differ, first at %s: got %d, recorded %d" % (
            name, len(bad), bad[0].tolist(), got[name][tuple(bad[0])], want[name][tuple(bad[0])])
    assert (want["asw_err"] != 0).any() and (want["asw_err"][0] == 0).all()      # the sweep does contain failing queries, none unforced


# Every option that forces a kernel form and is read by the planner, alone, with a value that changes a plan.  What the per-shape
# cache holds is the workgroup geometry and which wave kernel serves the range.  Eight options change that, and dropping the forcing
# condition of any of them fails the test (each tried): GEOM, PIPE, DEPHASE, EVOL, WAVE, WAVE_RX, NO_E2, XOR_ONLY.  The
# other five cannot be caught by a geometry query: WAVE_WG, WAVE_MERGE and WAVE_RD only shape the wave kernel's strip, which
# is laid out anew for every query and never cached (no shape was found where they change the cached part), and the planner never
# reads SSAMD_ASW_STATIC and SSAMD_ASW_EVOL_MAX_MB.  The three strip options are asked all the same.
FORCING = [("SSAMD_ASW_GEOM", "3,5,8"), ("SSAMD_ASW_PIPE", "0"), ("SSAMD_ASW_DEPHASE", "0"), ("SSAMD_ASW_EVOL", "0"), ("SSAMD_ASW_WAVE", "0"),
           ("SSAMD_ASW_WAVE_RX", "8"), ("SSAMD_ASW_WAVE_WG", "4"), ("SSAMD_ASW_WAVE_MERGE", "0"), ("SSAMD_ASW_WAVE_RD", "4"),
           ("SSAMD_ASW_NO_E2", "1"), ("SSAMD_ASW_XOR_ONLY", "1")]

_ORDERING_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from simplestereo_amd import _native
sys.path.insert(0, sys.argv[2])
import make_golden_plan as rec
sweep = json.load(open(sys.argv[2] + "/plan_cases.json")); want = np.load(sys.argv[2] + "/plan_cases.npz")
forcing = json.loads(sys.argv[3])

def ordering(options, shape_list, unforced, query, used):
    # shapes nobody has asked about in this process (the per-shape cache is cold): the forced query comes FIRST, the unforced one
    # must then give the recorded unforced answer.  Needs a shape whose forced answer differs, or a leak could not show.
    told_apart = 0
    for k, (W, rows, win, nD) in enumerate(shape_list):
        if k in used or told_apart >= 3:
            continue
        used.add(k)
        with _native.options(**options):
            try:
                forced = query(W, rows, win, nD - 1, 0)
            except _native.NativeError:
                forced = None
        got = query(W, rows, win, nD - 1, 0)
        assert got == unforced[k].tolist(), ("a forced geometry was served to an unforced call", options, shape_list[k], got, unforced[k].tolist())
        told_apart += forced != got
    assert told_apart >= 3, ("no shape of the sweep tells this option's plans from the unforced ones", options)

asw = lambda *a: list(_native.asw_geometry(*a).values()) + list(_native.asw_kernel_form(*a).values())
gsw = lambda *a: list(_native.gsw_geometry(*a).values())
used = set()
for name, value in forcing:
    ordering({name: value}, rec.shapes(sweep), want["asw"][0], asw, used)
used = set()
for opts in sweep["gsw_options"][1:]:
    ordering(opts, rec.shapes(sweep, sweep["gsw_max_win"]), want["gsw"][0], gsw, used)
print("ok")
"""


def test_unforced_answer_after_a_forced_query_of_the_same_shape():
    """a forced geometry must never reach the per-shape cache.  In a fresh process, for every forcing option on its own and every
    forced GSW geometry: shapes that are cold in the cache and whose forced plan differs are asked forced FIRST, then with no option,
    and the unforced answer must be the recorded one.  An option that stops forcing writes its plan into the cache and fails here."""
    import json
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if not k.startswith("SSAMD_")}
    r = subprocess.run([sys.executable, "-c", _ORDERING_CHILD, ROOT, GOLDEN, json.dumps(FORCING)], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-1500:]
