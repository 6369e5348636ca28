"""Arguments that aim at every branch of the unwrapping kernel's ``unwrap_fmod_2pi`` (simplestereo_amd/csrc/unwrap_kernels.hip.h),
and a host-side model of that function that says which branch an argument takes.

The kernel restates IEEE ``fmod(x, 2 pi)``: ``|x| >= 2^40`` and non-finite ``x`` go to the library fmod; otherwise
``k = trunc(x * (1 / m))``, ``r = fma(-k, m, x)`` and a correction of ``k`` by one when ``r`` has the wrong sign (towards zero)
or is a whole period away (away from zero).  ``branch_census`` evaluates exactly that in integers: the product ``x * c`` is
one fp64 multiplication by the double ``c = 1.0 / m`` (what the compiler folds the constant to), the remainder ``x - k m`` is
exact rational arithmetic, and the comparison ``r >= m`` is made on the remainder rounded to fp64 as the fma rounds it.

The probes reach the kernel through the public batch call as maps ``[[0, a]]``: pass 1 computes ``W(a)`` (fmod argument
``a + pi``), pass 2 ``W(a - W(a))`` -- a multiple of 2 pi up to rounding -- and the main pass more of the same.
``fmod_arguments`` records every fmod argument of the plain restatement (tests/_unwrap_ref.py) on such maps.
"""
import math
from fractions import Fraction

import numpy as np

import _unwrap_ref

M = 2 * math.pi
C = 1.0 / M
PI = math.pi
SWITCH = 2.0 ** 40

BRANCHES = ("library", "pos_direct", "pos_r_lt_0", "pos_r_ge_m", "neg_direct", "neg_r_gt_0", "neg_r_le_minus_m")
# `r >= m` for x >= 0 and `r <= -m` for x < 0 cannot happen for any double: C lies above the exact reciprocal of the
# double M (test_unwrap_cpu.py::test_reciprocal_of_two_pi_is_rounded_up asserts it), so x * C >= x / M >= floor(x / M)
# exactly, rounding to nearest is monotonic and floor(x / M) < 2^38 is representable: k is never below the true quotient.
DEAD = ("pos_r_ge_m", "neg_r_le_minus_m")

_MN, _MD = M.as_integer_ratio()


def branch(x):
    """Which branch of unwrap_fmod_2pi the double x takes (one of BRANCHES)."""
    if not (abs(x) < SWITCH):                      # NaN and +-inf included
        return "library"
    k = math.trunc(x * C)
    xn, xd = x.as_integer_ratio()
    num = xn * _MD - k * _MN * xd                  # sign of x - k m (denominator xd * _MD > 0)
    if x >= 0:
        if num < 0:
            return "pos_r_lt_0"
        if num > 0 and float(Fraction(num, xd * _MD)) >= M:
            return "pos_r_ge_m"
        return "pos_direct"
    if num > 0:
        return "neg_r_gt_0"
    if num < 0 and float(Fraction(num, xd * _MD)) <= -M:
        return "neg_r_le_minus_m"
    return "neg_direct"


def branch_census(args):
    """{branch: count} over an iterable of fmod arguments.  A float prefilter settles the clear cases (the naive fp64
    remainder is off by a few ulps of x at most); the rest go through the exact model."""
    x = np.asarray(list(args) if not isinstance(args, np.ndarray) else args, dtype=np.float64)
    out = dict.fromkeys(BRANCHES, 0)
    lib = ~(np.abs(x) < SWITCH)
    out["library"] = int(lib.sum())
    x = x[~lib]
    k = np.trunc(x * C)
    r = x - k * M                                   # naive: error below 4 ulps of |x| + M
    slack = 8 * np.spacing(np.abs(x) + M)
    clear_mid = (np.abs(r) > slack) & (np.abs(r) < M - slack) & ((r > 0) == (x >= 0))
    clear_back = (np.abs(r) > slack) & (np.abs(r) < M - slack) & ((r > 0) != (x >= 0))
    pos = x >= 0
    out["pos_direct"] += int((clear_mid & pos).sum())
    out["neg_direct"] += int((clear_mid & ~pos).sum())
    out["pos_r_lt_0"] += int((clear_back & pos).sum())
    out["neg_r_gt_0"] += int((clear_back & ~pos).sum())
    for v in x[~(clear_mid | clear_back)].tolist():
        out[branch(v)] += 1
    return out


def _steps(v, n):
    """v moved by n ulps (n may be negative)"""
    for _ in range(abs(n)):
        v = math.nextafter(v, math.inf if n > 0 else -math.inf)
    return v


def probes(seed=7):
    """float64 array of the values a of the issue's list, each with both signs (about 2 * 10^5 values)."""
    rng = np.random.default_rng(seed)
    a = []
    # k * 2 pi and k * 2 pi - pi, each +- 0, 1, 2 ulps: k spread logarithmically up to 2^38 ...
    ks = sorted({int(round(2.0 ** (j / 4.0))) for j in range(0, 153)} | {0, 3, 5, 7})
    for k in ks:
        for base in (k * M, k * M - PI):
            a.extend(_steps(base, n) for n in (-2, -1, 0, 1, 2))
    # ... and densely for small k (a + pi lands within an ulp or two of a multiple of 2 pi: the corrections towards zero)
    kd = np.arange(1, 100000, 7, dtype=np.float64)
    base = kd * M - PI
    for n in (-2, -1, 0, 1, 2):
        v = base.copy()
        for _ in range(abs(n)):
            v = np.nextafter(v, np.inf if n > 0 else -np.inf)
        a.extend(v.tolist())
    # |a + pi| within a few ulps either side of 2^40, the switch to the library fmod
    for n in range(-6, 7):
        a.append(_steps(SWITCH, n) - PI)
        a.append(_steps(SWITCH - PI, n))
    # powers of two and random mantissas at exponents from 2^40 to 2^1023, 1e300
    for e in range(40, 1024):
        a.append(math.ldexp(1.0, e))
        a.append(math.ldexp(1.0 + float(rng.random()), e))
    a.append(1e300)
    a.append(float(np.finfo(np.float64).max))
    # zero, denormals, the neighbours of pi and 2 pi
    a.extend([0.0, 5e-324, 2.0 ** -1060, 2.0 ** -1023, float(np.finfo(np.float64).tiny), PI, M,
              math.nextafter(PI, 0.0), math.nextafter(PI, math.inf), math.nextafter(M, 0.0), math.nextafter(M, math.inf)])
    a.extend(math.ldexp(float(rng.random()), -1022) for _ in range(50))
    # uniformly random exponents over the whole range
    e = rng.integers(-1074, 1024, 30000)
    a.extend(np.ldexp(1.0 + rng.random(30000), e).tolist())
    a = np.array(a, dtype=np.float64)
    return np.concatenate([a, -a])


def fmod_arguments(maps, tau):
    """(outputs, arguments): the restatement's unwrapped maps of `maps` [n, h, w] and every argument it passed to fmod."""
    seen = []
    plain = _unwrap_ref._W

    def recording(v):
        seen.append(v + PI)
        return plain(v)

    _unwrap_ref._W = recording
    try:
        out = np.stack([_unwrap_ref.unwrap(m, tau) for m in maps])
    finally:
        _unwrap_ref._W = plain
    return out, np.array(seen, dtype=np.float64)


def pair_maps(a):
    """[n, 1, 2] maps [[0, a]]"""
    z = np.zeros((len(a), 1, 2))
    z[:, 0, 1] = a
    return z


def square_maps(a, seed=11):
    """[n, 2, 2] maps [[0, a], [b, a]] with b a permutation of a"""
    b = np.random.default_rng(seed).permutation(a)
    z = np.zeros((len(a), 2, 2))
    z[:, 0, 1] = a
    z[:, 1, 0] = b
    z[:, 1, 1] = a
    return z
