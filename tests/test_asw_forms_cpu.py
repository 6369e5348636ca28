"""CPU tier of the kernel-form catalogue (tests/_asw_forms.py): every form that a GPU test forces is asked of the planner here,
at the test's own shape and parameters -- ssamd_asw_kernel_form and ssamd_asw_geometry are host-side queries and need no device.
A planner or option change that makes a forced form unreachable fails here, before a GPU is involved.  Then the helper itself:
`forced` has teeth (an expectation that the unforced plan does not meet raises) and puts every option back, also after a block
that raised."""
import numpy as np
import pytest

import _asw_band_ref as B
import _asw_forms as F
import test_gpu_asw
import test_gpu_asw_alternate
import test_gpu_asw_workgroup_build
import test_gpu_exact_forms
import test_gpu_pipe_build
import test_gpu_pipe_persist

GPU_FILES = (test_gpu_asw, test_gpu_asw_alternate, test_gpu_asw_workgroup_build, test_gpu_exact_forms, test_gpu_pipe_build,
             test_gpu_pipe_persist)
BAND_ROWS = [(form, c["shape"][1], c["shape"][0], c["params"]) for name, c in sorted(B.CASES.items()) for form in c["forms"]]
# FORMS entries whose expectation the unforced plan already meets at every band case that lists them.  "planner" expects nothing
# (it only keeps the tuner out) and "chunks" names what the planner does by itself for a range of 600 disparities.  The others
# are listed by cases made for them -- a range and window at which the planner picks that very kernel (17 / 18 disparities for
# "wave6", up to 20 for "wave4", up to 40 for "wave8", 66 and 72 for "pipe") -- so that the options pin what a later change of
# the planner's preferences would move; their teeth show at the rows of the GPU tests, which force them against the plan.
MET_UNFORCED = {"planner", "chunks", "wave4", "wave6", "wave8", "pipe", "pipe_evol0"}


def _rows(module):
    return list(module.forced_rows())


def _meets(plan, expect):
    return all(v(plan[k]) if callable(v) else plan[k] == v for k, v in expect.items())


def _split(form):
    return F.FORMS[form] if isinstance(form, str) else form


@pytest.mark.parametrize("module", GPU_FILES + (None,), ids=[m.__name__ for m in GPU_FILES] + ["test_gpu_asw_band"])
def test_every_forced_row_of_the_gpu_tests_is_reachable(module):
    rows = _rows(module) if module else BAND_ROWS
    assert rows
    for row in rows:
        with F.forced(*row) as plan:
            assert len(plan) == 13 and set(_split(row[0])[1]) <= set(plan)


def test_wave_tiles_that_may_not_fit_lds():
    """the rows the tests of tests/test_gpu_asw.py leave out when the planner reports another wave kernel: nothing else about
    them may be amiss, and each test keeps the number of rows it needs"""
    for rows, least in test_gpu_asw.rows_that_may_not_fit():
        assert sum(test_gpu_asw._fits(row) for row in rows) >= least, rows


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_forms_run_what_they_say(name):
    """the planner's answer under every form's options (a host-side query: no GPU), with and without the cost-image hook, which
    forces nothing"""
    c = B.CASES[name]
    (H, W), p = c["shape"], c["params"]
    for form in c["forms"]:
        opts, want = F.FORMS[form]
        seen = []
        for hook in ({}, dict(SSAMD_ASW_COST_KEYS="1")):
            with F.forced(dict(opts, **hook), W, H, p, want) as f:
                seen.append(f)
        assert seen[0] == seen[1], (name, form)


def test_forced_has_teeth():
    """an expectation that the unforced plan of the row's shape does not meet raises without the options; the named forms that the
    unforced plan meets everywhere are the two listed above, and no row goes unjudged"""
    rows = BAND_ROWS + [row for m in GPU_FILES for row in _rows(m)]
    met, raised = set(), 0
    for form, W, H, p in rows:
        expect = _split(form)[1]
        if _meets(F.planned(W, H, p), expect):
            if isinstance(form, str):
                met.add(form)
            continue
        with pytest.raises(F.FormMismatch) as e:
            with F.forced({}, W, H, p, expect):
                pass
        assert e.value.key in expect and e.value.planned == F.planned(W, H, p)
        assert str(p) in str(e.value) and e.value.key in str(e.value)
        raised += 1
    unmet = {f for f, W, H, p in BAND_ROWS if not _meets(F.planned(W, H, p), F.FORMS[f][1])}
    assert MET_UNFORCED == set(F.FORMS) - unmet, (met, unmet)
    assert {form for form, _, _, _ in BAND_ROWS} == set(F.FORMS)          # every named form is some case's
    assert raised > len(rows) // 2, (raised, len(rows))
    with pytest.raises(AssertionError):                          # options without a statement of what must run
        with F.forced(dict(SSAMD_ASW_WAVE="0"), 128, 96, dict(winSize=9, maxDisparity=15)):
            pass


def test_forced_puts_the_options_back():
    """after a block that raised inside, after a mismatch, and after a plain block: the plan is the one from before"""
    W, H, p = 128, 24, dict(winSize=9, maxDisparity=15)
    before = F.planned(W, H, p)
    form = F.workgroup_tile("6,5,8,8")
    assert not _meets(before, form[1])
    with pytest.raises(ZeroDivisionError):
        with F.forced(form, W, H, p) as plan:
            assert plan != before and F.planned(W, H, p) == plan
            1 / 0
    assert F.planned(W, H, p) == before
    with pytest.raises(F.FormMismatch):
        with F.forced(F.also(form, tile_x=7), W, H, p):
            pass
    assert F.planned(W, H, p) == before
    with F.forced(form, W, H, p):
        pass
    assert F.planned(W, H, p) == before


def test_same_costs_is_the_strict_rule():
    a = np.array([0.0, 1.0, np.nan, 2.0], np.float32)
    assert F.same_costs(a, a.copy()) == 0
    assert F.same_costs(np.array([-0.0, 1.0, np.nan, 2.0], np.float32), a) == 1          # the sign of a zero
    assert F.same_costs(np.array([0.0, 1.0, 3.0, np.nan], np.float32), a) == 2           # the NaN pattern
    other_nan = np.array([0, 0x3F800000, 0x7FC00001, 0x40000000], np.uint32).view(np.float32)
    assert F.same_costs(other_nan, a) == 0                                               # a NaN's payload is not a cost
