"""CPU tier of the phase-shift decode on its whole input domain: the mask threshold of ``active._mod_thr2`` against an independent
reference (tests/_phaseshift_ref.mod_thr2, a bisection on rationals) and against the rule itself -- a set masks its pixel iff
a^2 + b^2 < 4 m^2 in exact arithmetic on the double m --, the recorded tolerances of tests/golden/phaseshift_domain_cases.json
against their rule, and the conditions the tie-aware comparison of tests/test_gpu_phaseshift_domain.py rests on, re-checked on the
stacks the GPU tier rebuilds from the same seeds.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _phaseshift_ref as P

META = P.load_domain()
PINNED = ((None, 0), (0, 0), (0.5, 1), (1.5, 9), (50, 10000), (1e200, P.MOD_ALL), (np.inf, P.MOD_ALL))     # test_phaseshift_cpu.py pins the same


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


# ------------------------------------------------------------------------------------------------ the mask threshold
def _follows_the_rule(t, m):
    """(s < t) == (s < 4 m^2, exactly) for every integer s = a^2 + b^2 in 0 .. 130050"""
    want = 4 * Fraction(m) ** 2
    if t == 0:
        return want <= 0
    if t == P.MOD_ALL:
        return want > P.MOD_ALL - 1
    return 0 < t < P.MOD_ALL and t - 1 < want <= t


def test_threshold_is_the_exact_rule_at_every_sum_of_squares(ss):
    """m at sqrt(s) / 2 and the two doubles either side of it, for every s = 0 .. 130051: package == reference == rule.
    ``ceil(4.0 * m * m)`` in double misses the rule at some 6 % of these"""
    thr = ss.active._mod_thr2
    s = np.arange(P.MOD_ALL + 1, dtype=np.float64)
    mid = np.sqrt(s) / 2
    ms = [mid]
    for direction in (-np.inf, np.inf):
        m = mid
        for _ in range(2):
            m = np.nextafter(m, direction)
            ms.append(m)
    ms = np.stack(ms, axis=1)                                # [s, 5]
    float_formula = np.minimum(np.ceil(np.minimum(4.0 * ms * ms, float(P.MOD_ALL))), P.MOD_ALL)
    checked = off = 0
    for row, formula in zip(ms.tolist(), float_formula.tolist()):
        for m, f in zip(row, formula):
            if m < 0:                                        # below sqrt(0) / 2
                continue
            t = thr(m)
            assert type(t) is int and t == P.mod_thr2(m) and _follows_the_rule(t, m), (m.hex(), t, P.mod_thr2(m))
            checked += 1
            off += t != f
    print("%d values of m, the double formula ceil(4.0 * m * m) off at %d" % (checked, off))
    assert checked == 5 * (P.MOD_ALL + 1) - 2 and off > 20000         # the defect this replaces is in the probed set


@pytest.mark.parametrize("m", [5e-324, 1e-200, 1e-163, 1e-160, 1e154, 1e200, np.inf])
def test_threshold_at_the_ends_of_the_double_range(ss, m):
    t = ss.active._mod_thr2(m)
    assert t == P.mod_thr2(m) == (1 if m < 1 else P.MOD_ALL)            # 0 < m masks a = b = 0; no overflow, no underflow to 0
    assert m == np.inf or _follows_the_rule(t, m)
    assert P.masks(0, m) and P.masks(P.MOD_ALL - 1, m) == (m > 1)


def test_threshold_named_values(ss):
    for m, t in PINNED:
        assert ss.active._mod_thr2(m) == P.mod_thr2(m) == t, m
    half_sqrt2, half_sqrt17 = math.sqrt(2.0) / 2, math.sqrt(17.0) / 2
    assert half_sqrt2 == 0.7071067811865476 and 4 * Fraction(half_sqrt2) ** 2 > 2           # fl(sqrt(2) / 2) lies above sqrt(2) / 2 ...
    assert ss.active._mod_thr2(half_sqrt2) == P.mod_thr2(half_sqrt2) == 3 and not math.sqrt(2.0) / 2 < half_sqrt2    # ... the float test says 2
    assert 4 * Fraction(half_sqrt17) ** 2 > 17 and math.ceil(4.0 * half_sqrt17 * half_sqrt17) == 17      # ... the double formula says 17
    assert ss.active._mod_thr2(half_sqrt17) == P.mod_thr2(half_sqrt17) == 18
    for bad in (-1, -5e-324, np.nan, -np.inf, "1", True):
        with pytest.raises(ValueError):
            ss.active._mod_thr2(bad)
    assert ss.active._mod_thr2(np.float32(1.5)) == ss.active._mod_thr2(3) // 4 == 9


# ------------------------------------------------------------------------------------------------ the grid
def test_grid_holds_every_pair_twice_and_its_tolerances_follow_the_rule():
    a, b = P.domain_pairs()
    assert a.shape == (511, 511) and (a.min(), a.max(), b.min(), b.max()) == (-255, 255, -255, 255)
    assert len(set(zip(a.ravel().tolist(), b.ravel().tolist()))) == 511 * 511
    plain, lifted = P.domain_stack().astype(np.int64), P.domain_stack(lifted=True).astype(np.int64)
    assert plain.shape == lifted.shape == (8, 511, 511)
    for s in (plain, lifted):                                # the x-set holds (a, b), the y-set (b, a)
        assert np.array_equal(s[3] - s[1], a) and np.array_equal(s[0] - s[2], b) and np.array_equal(s[7] - s[5], b) and np.array_equal(s[4] - s[6], a)
    assert (plain != lifted).mean() > 0.99                   # other bytes (all but those of |a|, |b| = 255), the same integers
    theta = np.mod(np.arctan2(a.astype(np.float64), b.astype(np.float64)), 2 * np.pi)
    assert np.unique(theta).size == META["distinct_theta"] == 158598
    assert sorted(META["grid"]) == ["1920x1080", "1x1", "64x32", "65536x65536"]
    stack = P.domain_stack()
    for name, c in META["grid"].items():
        extent = tuple(c["extent"])
        assert name == "%dx%d" % extent and c["periods"] == P.DOMAIN_PERIODS and c["flagged"] == 0
        assert c["tol"] == META["tol_factor"] * max(c["numpy_err"], max(extent) * META["floor"])
        d64 = P.decode(stack, P.DOMAIN_PERIODS, extent)
        dld = P.decode(stack, P.DOMAIN_PERIODS, extent, dtype=np.longdouble)
        err = float(np.abs(d64.astype(np.longdouble) - dld).max())
        print("grid %s: restatement against long double %.3e (recorded %.3e, tolerance %.3e)" % (name, err, c["numpy_err"], c["tol"]))
        assert err <= c["tol"]
        for d in (d64, dld):                                 # the truth itself stays in [0, extent)
            assert (d >= 0).all() and (d[..., 0] < extent[0]).all() and (d[..., 1] < extent[1]).all()
    assert (META["tol_factor"], META["floor"], META["band"], META["tight_band"], META["agree"]) == (16.0, 2.0 ** -52, P.BAND, 1e-12, 1e-9)


# ------------------------------------------------------------------------------------------------ noise: the conditions of the tie-aware comparison
@pytest.mark.parametrize("name", sorted(P.NOISE_PERIODS))
def test_noise_case_meets_the_conditions_its_comparison_rests_on(name):
    c = META["noise"][name]
    periods, proj = P.NOISE_PERIODS[name], P.NOISE_PROJ
    assert c["periods"] == periods and tuple(c["extent"]) == proj and tuple(c["shape"]) == P.NOISE_SHAPE
    assert c["tol"] == META["tol_factor"] * max(c["numpy_err"], max(proj) * META["floor"])
    stack = P.noise_stack(c["seed"], periods)
    assert stack.shape == (4 * (len(periods[0]) + len(periods[1])),) + P.NOISE_SHAPE and stack.dtype == np.uint8
    d64, tie = P.decode(stack, periods, proj, details=True)
    dld = P.decode(stack, periods, proj, dtype=np.longdouble)
    flagged = tie > 0.5 - P.BAND
    n = int(flagged.sum())
    assert n == int((tie > 0.5 - META["tight_band"]).sum()) == c["flagged"]              # on the tie, not near it: no status hangs on the band
    assert 1 <= n <= flagged.size * META["max_flagged_share"] == 131.072                 # the tie path is executed, and stays an exception
    err = np.abs(d64.astype(np.longdouble) - dld).max(axis=-1)
    worst = float(err[~flagged].max())
    print("noise %s: %d flagged, restatement against long double elsewhere %.3e (recorded %.3e, tolerance %.3e)" % (name, n, worst, c["numpy_err"], c["tol"]))
    assert worst <= META["agree"] and worst <= c["tol"]
    # the enumerator: the restatement's own value is a member, bit for bit; long double is within tol of one, although it lies a
    # whole period from the restatement on some of these pixels
    for got, bound in ((d64, 0.0), (dld, c["tol"])):
        dist, largest = P.distance_to_candidates(got, stack, periods, proj, flagged)
        assert dist.shape == (n, 2) and dist.max() <= bound and 2 <= largest <= 2 ** 7
    assert int((err[flagged] > c["tol"]).sum()) == c["ld_other_k"]
    # away from a tie the enumerator is the restatement on scalars: one member, its bits
    rng = np.random.default_rng(0)
    for y, x in zip(rng.integers(0, P.NOISE_SHAPE[0], 50), rng.integers(0, P.NOISE_SHAPE[1], 50)):
        if not flagged[y, x]:
            cx, cy = P.pixel_candidates(stack, periods, proj, y, x)
            assert cx == [d64[y, x, 0]] and cy == [d64[y, x, 1]]
    # min_modulation = 50 is no trivial mask on noise
    masked = np.isnan(P.decode(stack, periods, proj, thr2=P.mod_thr2(50))[..., 0])
    assert min(int(masked.sum()), int((~masked).sum())) >= 100           # (16 sets leave 0.16 % of the pixels unmasked)
