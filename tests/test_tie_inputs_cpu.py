"""CPU tier: the inputs of tests/test_gpu_exact_forms.py really are tie-rich, judged by the fp64 oracle's own costs.

A pixel is 'unresolved' when its best two fp64 costs lie closer than fp32 resolves them (1e-5 relative below cost 20, the
near-tie rule's sat_abs above it).  The floors below are about half of what each input has (counts in the comments), so a
generator that loses its ties fails here, without a GPU."""
import numpy as np
import pytest

import _tie_inputs as T


# (generator, shape, params, floor): the GPU matrix's inputs; measured counts of unresolved pixels in the comments
CASES = [
    ("quantised", (24, 128), dict(winSize=21, maxDisparity=39, gammaC=5.0), 80),        # 161 of 3 072
    ("quantised", (24, 128), dict(winSize=9, maxDisparity=19, gammaC=0.7), 1200),       # 2 566
    ("quantised", (16, 200), dict(winSize=15, maxDisparity=40, gammaC=7.0), 1200),      # 2 526
    ("black_margins", (24, 128), dict(winSize=21, maxDisparity=39, gammaC=5.0), 350),   # 744
    ("black_margins", (24, 128), dict(winSize=9, maxDisparity=19, gammaC=0.7), 700),    # 1 413
    ("black_margins", (16, 200), dict(winSize=15, maxDisparity=40, gammaC=7.0), 450),   # 963
    ("patches", (24, 128), dict(winSize=9, maxDisparity=19, gammaC=0.7), 1300),         # 2 712
]


@pytest.fixture(scope="module")
def oc():
    return T.OracleCache()


@pytest.mark.parametrize("kind,shape,params,floor", CASES)
def test_generators_are_tie_rich(kind, shape, params, floor, oc):
    H, W = shape
    p = dict(params, minDisparity=0, gammaP=17.5)
    L, R = T.pair(kind, H, W, p["maxDisparity"], seed=3)
    assert L.dtype == np.uint8 and L.shape == (H, W, 3) and R.shape == L.shape
    assert T.taps(L, p) <= T.MAX_TAPS
    L2, R2 = T.pair(kind, H, W, p["maxDisparity"], seed=3)
    assert np.array_equal(L, L2) and np.array_equal(R, R2)              # deterministic
    _, c = oc.asw(L, R, return_costs=True, **p)
    n = T.fp32_unresolved(c, p["winSize"])
    print("%s %s %s: %d of %d pixels below fp32 resolution" % (kind, shape, params, n, H * W))
    assert n >= floor, (kind, n, floor)


def test_oracle_cache_calls_the_oracle_once():
    oc = T.OracleCache()
    L, R = T.pair("quantised", 8, 40, 7, seed=1)
    p = dict(winSize=5, maxDisparity=7, minDisparity=0, gammaC=5.0, gammaP=17.5)
    a = oc.asw(L, R, **p)
    assert oc.asw(L, R, **p) is a
    from oracle import oracle
    assert np.array_equal(a, oracle.asw(L, R, **p))
    assert T.nthreads() <= 16


def test_lone_zero_frame_in_fp64():
    """the lone zero-cost winner of test_gpu_exact_forms.py, fp64 side: (b) the reference picks D1, whose cost is positive and
    below D0's; D0's fp64 cost is below rule (d)'s floor Z / 2 (the bound the fix rests on) and D1's above the few denormals that
    rule (a) spans at 0 (c, on the fp64 cost: the GPU test checks the fp32 image)"""
    from oracle import oracle
    L, R, p = T.lone_zero_pair()
    d, c = oracle.asw(L, R, return_costs=True, **p)
    x, d0, d1 = T.LZ_X, T.LZ_D0, T.LZ_D1
    row = c[0, x]
    assert int(d[0, x]) == d1
    assert 0.0 < row[d1] < row[d0] < T.zero_floor(p["winSize"]) / 2
    assert int(np.argmin(row)) == d1 and np.count_nonzero(row <= row[d0]) == 2       # D0 is the runner-up, nothing else is close
    assert row[d1] > 100 * T.tol(p["winSize"], p["gammaC"]) * 2.0 ** -149
    assert row[d1] < T.zero_floor(p["winSize"])                                       # rule (d) queues it
