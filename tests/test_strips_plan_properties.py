"""CPU tier: properties of the row-strip partition and of the halo transfer plan for arbitrary image heights,
world sizes and window sizes (hypothesis) -- the multi-GPU path is correct by construction only if these hold; the plan of one
rank, the whole-rounds cut of the interior launch and the overlap policy, each a function of plain values."""
import importlib.util
import json
import os
import types

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

from simplestereo_amd import strips


@settings(max_examples=300, deadline=None)
@given(H=st.integers(1, 400), world=st.integers(1, 16), pad=st.integers(0, 127))
def test_partition_and_transfer_plan(H, world, pad):
    own = [strips.strip_bounds(H, world, r) for r in range(world)]
    # contiguous partition of [0, H), sizes differ by at most one row
    assert own[0][0] == 0 and own[-1][1] == H
    assert all(own[r][1] == own[r + 1][0] for r in range(world - 1))
    sizes = [b - a for a, b in own]
    assert max(sizes) - min(sizes) <= 1
    plan = strips.transfer_plan(H, world, pad)
    got = {r: np.zeros(H, np.int32) for r in range(world)}
    for src, dst, lo, hi in plan:
        assert src != dst and 0 <= lo < hi <= H
        assert own[src][0] <= lo and hi <= own[src][1]            # the sender owns what it sends
        got[dst][lo:hi] += 1
    for r in range(world):
        r0, r1 = own[r]
        h0, h1 = strips.halo_bounds(H, r0, r1, pad)
        need = np.zeros(H, np.int32)
        if r1 > r0:
            need[h0:r0] = 1
            need[r1:h1] = 1
            assert h0 == max(0, r0 - pad) and h1 == min(H, r1 + pad)
        assert np.array_equal(got[r], need)                        # every halo row exactly once, nothing else
    # deterministic and identical on every rank: the plan is a pure function of (H, world, pad)
    assert plan == strips.transfer_plan(H, world, pad)


# ---- the plan of one rank, against what StripContext planned before the plan had a function of its own ----

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _strip_plan_recorder():
    spec = importlib.util.spec_from_file_location("make_golden_strip_plan", os.path.join(GOLDEN, "make_golden_strip_plan.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_planned_row_equals_the_recorded_one():
    """tests/golden/strip_plan_cases.json: pad, strip, halo, the halo-free cut, rows_max and both message lists of every rank of
    worlds 1 / 2 / 3 / 8 on frames of 1 .. 1080 rows, through the public constructor on CPU -- and the same integers from
    strip_plan itself"""
    rec = _strip_plan_recorder()
    with open(os.path.join(GOLDEN, "strip_plan_cases.json")) as f:
        want = json.load(f)
    assert want["grid"] == rec.GRID and tuple(want["fields"]) == rec.FIELDS, "strip_plan_cases.json is not the grid of make_golden_strip_plan.py"
    got = rec.replay(rec.GRID)
    assert len(got) == len(want["rows"]) == 7 * (1 + 2 + 3 + 8) * 5
    for g, w in zip(got, want["rows"]):
        assert g == w, (dict(zip(("H", "world", "rank", "matcher") + rec.FIELDS, g)), "recorded", w)
    empty = thin = one_sided = 0
    for H, world, rank, k, pad, r0, r1, h0, h1, top, bot, interior, rows_max, sends, recvs in want["rows"]:
        p = strips.strip_plan(H, world, rank, pad)
        assert list(p[:5]) + list(p[7:]) + [p.rows_max] == [r0, r1, h0, h1, [tuple(t) for t in sends], top, bot, interior, rows_max]
        assert p.recvs == [tuple(t) for t in recvs] and top + interior + bot == r1 - r0
        empty += r1 == r0
        thin += 0 < r1 - r0 < pad
        one_sided += r1 > r0 and (h0 < r0) != (h1 > r1)
    assert empty and thin and one_sided          # the grid does hold the three kinds of edge
    spot = {(r[0], r[1], r[2], r[3]): r[4 + rec.FIELDS.index("h0"):4 + rec.FIELDS.index("rows_max")] for r in want["rows"]}
    assert spot[(1080, 8, 1, 3)] == [118, 287, 17, 17, 101] and spot[(1080, 2, 0, 3)] == [0, 557, 0, 17, 523]


# ---- the whole-rounds cut: the arithmetic alone, then through the launch planner (host arithmetic: no GPU) ----

@pytest.mark.parametrize("args,rows", [((101, 16, 768, 161200, 256), 96), ((236, 16, 768, 161200, 256), 224),
                                       ((506, 16, 768, 161200, 256), 496), ((236, 47, 768, 163504, 256), 234),
                                       ((101, 20, 256, 79920, 256), 76), ((10, 24, 512, 127280, 256), 0),
                                       ((200, 4, 768, 120128, 256), 192)])
def test_whole_rounds_arithmetic(args, rows):
    """(interior rows, workgroups per row, threads, lds_bytes, compute units) -> rows of the interior launch, as recorded from
    StripContext._whole_rounds before the arithmetic had a function of its own"""
    assert strips.whole_rounds(*args) == rows
    interior, per_row, threads, lds, cus = args
    rounds = interior * per_row // (cus * strips.resident_workgroups(threads, lds))           # whole rounds the halo-free rows fill
    assert rows <= interior and (rows > 0) == (rounds >= 1)
    assert rows == rounds * cus * strips.resident_workgroups(threads, lds) // per_row           # the rows that fit into them


@pytest.mark.parametrize("shape,rows", [((1920, 101, 35, 192), 96), ((4096, 236, 35, 256), 234), ((1920, 101, 35, 64), 76),
                                        ((1920, 101, 35, 16), 101),                   # wave kernel: uncut
                                        ((1920, 10, 35, 192), 0), ((640, 200, 21, 128), 192)])
def test_interior_cut_through_the_planner(shape, rows):
    """(W, interior, winSize, maxDisparity) at minDisparity 0 on 256 compute units"""
    W, interior, win, maxD = shape
    m = types.SimpleNamespace(winSize=win, maxDisparity=maxD, minDisparity=0)
    assert strips.asw_interior_cut(m, W, interior, 256) == rows


def test_interior_cut_keeps_the_rows_when_the_planner_refuses_the_shape():
    from simplestereo_amd import _native
    m = types.SimpleNamespace(winSize=35, maxDisparity=192, minDisparity=0)
    with _native.options(SSAMD_ASW_GEOM="96,8", SSAMD_ASW_WAVE="0"):        # 768 columns: does not fit LDS from winSize 9 on
        with pytest.raises(_native.NativeError):
            _native.asw_geometry(1920, 101, 35, 192, 0)
        assert strips.asw_interior_cut(m, 1920, 101, 256) == 101
    assert strips.asw_interior_cut(m, 1920, 101, 256) == 96


# ---- the overlap policy, against its rules ----

FACTS = dict(on_gpu=True, world_size=2, messages=4, top=17, bot=0, interior=83)
KINDS = {"asw": ("StereoASW", False, False), "asw consistent": ("StereoASW", True, False), "asw alternate": ("StereoASW", False, True),
         "gsw": ("StereoGSW", False, False), "unknown": ("SimpleNamespace", False, False)}


def _rule(name, mode, wanted):
    """the rules, restated: what overlaps when every fact of the run allows it"""
    if not wanted or mode == "0":
        return False
    if name == "asw":
        return True
    if name in ("asw consistent", "gsw"):
        return mode in ("force", "all", "gsw")
    return False                                  # alternate rows, any other matcher type


@pytest.mark.parametrize("mode", ["0", "1", "force", "all", "gsw", "yes"])
@pytest.mark.parametrize("name", sorted(KINDS))
def test_overlap_policy_table(name, mode):
    kind, consistent, alternate = KINDS[name]
    for wanted in (True, False):
        assert strips.overlap_policy(kind, consistent, alternate, mode, wanted, **FACTS) is _rule(name, mode, wanted), (name, mode, wanted)
    if mode == "yes":                             # any string other than the five named ones is the default
        assert _rule(name, "yes", True) == _rule(name, "1", True)
    # each fact of the run false in turn: never overlapped, whatever the matcher and the mode
    for off in (dict(on_gpu=False), dict(world_size=1), dict(messages=0), dict(interior=0), dict(top=0, bot=0)):
        assert strips.overlap_policy(kind, consistent, alternate, mode, True, **dict(FACTS, **off)) is False, (name, mode, off)
    # ... and a halo on the other side alone is a border all the same
    assert strips.overlap_policy(kind, consistent, alternate, mode, True, **dict(FACTS, top=0, bot=17)) is _rule(name, mode, True)


def test_context_reads_the_mode_once_and_keeps_the_cut_without_overlap(monkeypatch):
    """on CPU nothing overlaps and nothing is cut, in any mode; top / bot / interior are set all the same"""
    for mode in ("0", "1", "force", "yes"):
        monkeypatch.setenv("SSAMD_STRIP_OVERLAP", mode)
        ctx = strips.StripContext(types.SimpleNamespace(winSize=35), 1080, 4, 1, 8, "cpu")
        assert ctx.overlap is False and (ctx.top, ctx.interior, ctx.bot) == (17, 101, 17)
