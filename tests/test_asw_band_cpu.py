"""CPU tier of the near-tie band measurement (tests/test_gpu_asw_band.py): the reference image, the emulation, the inputs and
the case matrix of tests/_asw_band_ref.py, judged by the fp64 oracle's own costs.

A case of the differential measure needs near pairs (d*, c) -- the oracle's first minimum and a candidate whose fp64 cost image
lies a nonzero distance of at most 8 bands above it, both below cost 39 and on one side of 20.  Exact ties (gap 0) say nothing
about the kernels' differential error, and make_pair frames have no pair this close: the floors below are about half of what
each input has (counts in the comments), and every differential case has at least 200 of the band class -- pairs whose winner
lies above rule (d)'s floor, judged by the emulation's images here and by the kernels' own on the GPU."""
import json
import os
import sys

import numpy as np
import pytest

import _asw_band_ref as B
import _tie_inputs as T

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, G)
import make_golden_asw_band as M      # noqa: E402

with open(os.path.join(G, M.NAME)) as _f:
    FIXTURE = json.load(_f)

# near pairs of the band class per case: floor (measured).  Cases without a floor are measured per candidate only: a window of 3
# or 9 at a large gammaC has too few taps of small weight, the noisy low-contrast frames have candidates a few per cent apart,
# not a few 1e-5, and nearly every near pair of the three "flush" cases is of the floor class (rule (d): _asw_band_ref.py).
FLOORS = {
    "w35_g5_wave4": 2000,       # 4 134
    "w35_g5_pipe": 7000,        # 14 814
    "w35_g0.7_wave8": 4300,     # 8 705
    "w35_g50_pipe": 950,        # 1 977
    "w9_g0.7_wave6": 4500,      # 9 058
    "w255_g5": 1350,            # 2 746
    "w151_g0.7": 2300,          # 4 651
    "w21_g5_pipe": 9500,        # 19 629
    "w61_g50": 550,             # 1 107
    "w21_g0.7_wave8": 10000,    # 21 112
    "w61_g5_pipe": 6500,        # 13 619
}
# ... and of the floor class in the flush cases (378, 240, 764)
FLUSH_FLOORS = {"w21_g0.7_flush": 180, "w35_g0.7_flush": 120, "w9_g0.7_flush": 380}


@pytest.fixture(scope="module")
def oc():
    return T.OracleCache()


def test_image64():
    f = np.array([0.0, 1.0, 20.0, 37.0, 39.0, 40.0, np.nan])
    i = B.image64(f)
    assert i.tolist() == [0, 0x3F800000, 0x41A00000, 0xC0000000 - 0x40400000, 0xC0000000 - 0x3F800000, 0xC0000000, -1]
    # the image of cost 37 is the bit pattern of a float NaN: existence is told by the dump's fill word, never by isnan
    assert np.isnan(np.array([0xC0000000 - 0x40400000], np.uint32).view(np.float32)[0])
    assert B.image32(np.array([0xFFFFFFFF, 0x7FC00000, 5], np.uint32).view(np.float32)).tolist() == [-1, 0x7FC00000, 5]
    c = np.sort(np.random.default_rng(1).uniform(0, 40, 20000))
    assert np.all(np.diff(B.image64(c)) >= 0)                                   # monotone across the seam at 20
    assert B.image64(np.nextafter(20.0, 40.0)) >= B.HIGH > B.image64(20.0)
    # one image ulp below 20 is one float32 ulp of the cost; above it one float32 ulp of 40 - cost
    assert B.image64(np.float64(np.nextafter(np.float32(3.0), np.float32(4.0)))) - B.image64(3.0) == 1
    assert B.image64(38.0) - B.image64(40.0 - float(np.nextafter(np.float32(2.0), np.float32(3.0)))) == 1


def test_near_pairs_and_differential_on_a_hand_made_row():
    u = float(np.spacing(np.float32(1.0)))
    cost = np.array([[[1.0 + 5 * u, 1.0, 1.0, 1.0 + 2000 * u, np.nan, 39.5, 1.0 + 3 * u]]])
    m, ds = B.near_pairs(cost, 128)
    assert ds[0, 0] == 1                                                         # the FIRST minimum
    assert m[0, 0].tolist() == [True, False, False, False, False, False, True]   # gap 0, gap > 8 tol, none, > 39: out
    i64 = B.image64(cost)
    i32 = i64.copy()
    i32[0, 0, 1] += 7                                                            # the winner's image 7 ulps high, c exact
    assert B.differential_error(cost, i32, 128, B.zkey(35)) == (7, 2, 0, 0)
    assert B.differential_error(cost, i32, 128, int(i32[0, 0, 1])) == (0, 0, 7, 2)       # a winner at rule (d)'s floor
    assert B.candidate_error(cost, i32)[::2] == (7, 5)                           # (39.5 is not measured)
    assert B.candidate_error(cost, i32, above=int(i64[0, 0, 1]))[::2] == (0, 3)
    # exact_zkey: the image of 2 win^2 40 2^-126
    assert B.zkey(13) == int(np.array([T.zero_floor(13)], np.float32).view(np.uint32)[0])


def test_emulation_follows_the_oracle(oc):
    """a small frame: the same candidates exist, and the fp32 restatement stays within a few dozen image ulps of the oracle"""
    L, R = T.pair("shifted_noisy", 9, 40, 7, seed=2)
    p = dict(winSize=7, maxDisparity=7, minDisparity=0, gammaC=5.0, gammaP=17.5)
    _, cost = oc.asw(L, R, return_costs=True, **p)
    emu = B.emulate32(L, R, p)
    assert np.array_equal(emu < 0, np.isnan(cost))
    e_max, _, n = B.candidate_error(cost, emu)
    assert n > 2000 and e_max <= 32, (e_max, n)


def test_perturbed_and_shifted_generators():
    for kind in ("patches", "stripes", "quantised"):
        L, R = T.pair(kind, 24, 128, 19, seed=3)
        L2, R2 = T.pair("perturbed:" + kind, 24, 128, 19, seed=3)
        assert np.array_equal(L, L2) and R2.dtype == np.uint8 and R2.flags["C_CONTIGUOUS"]
        d = R2.astype(np.int32) - R
        assert np.abs(d).max() == 1 and np.all(np.count_nonzero(d, axis=2) <= 1)            # +-1 on one channel
        share = np.count_nonzero(d.any(axis=2)) / (24 * 128)
        assert 0.005 <= share <= 0.03, (kind, share)                                         # about 2 % (fewer where a step is clipped)
        assert np.array_equal(R2, T.pair("perturbed:" + kind, 24, 128, 19, seed=3)[1])       # seeded
    L, R = T.pair("stripes", 6, 50, 9, seed=3)
    assert np.all(L == L[:, :1]) and np.abs(R.astype(np.int32) - L).sum(axis=2).max() == 1
    L, R = T.pair("shifted_noisy", 12, 64, 9, seed=3)
    assert L.max() - L.min() < 50                                                            # low contrast


def test_matrix_covers_the_corners_of_the_scaling_rule():
    cs = B.CASES.values()
    wg = {(c["params"]["winSize"], c["params"]["gammaC"]) for c in cs}
    assert {(35, 5.0), (35, 0.7), (35, 50.0), (9, 0.7), (255, 5.0), (151, 0.7)} <= wg
    assert {w for w, _ in wg} == {3, 9, 21, 35, 61, 151, 255}
    assert {g for _, g in wg} == {0.7, 5.0, 50.0}
    assert {c["params"]["gammaP"] for c in cs} == {3.0, 17.5, 100.0}
    assert len(wg) >= 12
    assert sorted(n for n, c in B.CASES.items() if c["differential"]) == sorted(FLOORS)
    assert set().union(*(c["forms"] for c in cs)) >= {"planner", "wave4", "wave8", "wave6", "pipe", "pipe_evol0", "workgroup", "chunks"}
    assert T.tol(35, 5.0) == 128 and T.tol(35, 50.0) == 128 and T.tol(35, 0.7) == 914 and T.tol(255, 5.0) == 932


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_case_near_pairs_and_fixture(name, oc):
    """every figure of the fixture recomputed; the near-pair floors"""
    c, fx = B.CASES[name], FIXTURE[name]
    L, R, p = B.case_inputs(name)
    assert T.taps(L, p) <= T.MAX_TAPS
    got = M.record(name, oc)
    print(name, got)
    exact = [k for k in got if not k.startswith("emu_")]
    assert {k: got[k] for k in exact} == {k: fx[k] for k in exact}
    # the emulation's figures: numpy's float32 exp2 and sqrt may differ in the last place between builds, which moves a sum of
    # win^2 weighted terms by far less than an image ulp -- a maximum over 1e4 ... 1e6 candidates can still move by one or two
    for k in got:
        if k.startswith("emu_"):
            assert abs(got[k] - fx[k]) <= 2 + 0.05 * abs(fx[k]), (k, got[k], fx[k])
    if c["differential"]:
        assert got["emu_pairs_band"] >= FLOORS[name] >= B.MIN_PAIRS, (name, got["emu_pairs_band"])
    else:
        assert name not in FLOORS
    if name in FLUSH_FLOORS:
        assert got["emu_pairs_floor"] >= FLUSH_FLOORS[name] and got["emu_D_max_floor"] > got["tol"], (name, got)


def test_fixture_lists_the_matrix():
    assert sorted(FIXTURE) == sorted(B.CASES)

