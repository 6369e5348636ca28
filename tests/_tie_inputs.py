"""Tie-rich stereo pairs for the fp64 tie-break pass of StereoASW, and a per-module cache of the fp64 oracle's maps.

On make_pair frames the fp32 argmin equals the fp64 one almost everywhere, so a kernel form whose near-tie epilogue queues
nothing still returns the oracle's map.  The generators here make many pixels whose best two fp64 costs lie closer than fp32
resolves them (tests/test_tie_inputs_cpu.py pins how many), so that a form which loses near-ties shows it.  Helper module,
not a test."""
import os

import numpy as np

from simplestereo_amd.synth import make_pair

# one oracle call stays at or below this many H * W * nD * win^2 taps (the C oracle's cost on 16 threads: well under a second)
MAX_TAPS = 3e8


def nthreads():
    """the C oracle sizes its pool by sysconf (the whole machine): pass the CPUs this process may use instead"""
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "16"))
    except ValueError:
        n = 16
    return max(1, min(16, n))


def quantised(H, W, maxd, seed):
    """colours rounded to multiples of 64 and a mirrored right view: wide flat regions, most candidates saturated (cost near 40)"""
    L, R, _ = make_pair(H, W, max(8, maxd), seed)
    return np.ascontiguousarray(L // 64 * 64), np.ascontiguousarray(R[:, ::-1])


def black_margins(H, W, maxd, seed):
    """black bands on both views as rectified frames have them (left and top), the left view also black on the right"""
    L, R, _ = make_pair(H, W, max(8, maxd), seed)
    b = max(2, W // 3)
    L[:, :b] = 0; R[:, :b] = 0
    L[:H // 8] = 0; R[:H // 8] = 0
    L[:, W - W // 16:] = 0
    return np.ascontiguousarray(L), np.ascontiguousarray(R)


def patches(H, W, maxd, seed):
    """flat patches of a few colours repeated along the row (both views, shifted): many candidates tie exactly or saturate"""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (5, 3), dtype=np.uint8)
    cols = np.repeat(rng.integers(0, 5, (W + 64) // 4 + 1), 4)
    rows = np.repeat(rng.integers(0, 2, H // 3 + 1), 3)[:H]
    row = pal[cols]                                             # [W + 64 + ..][3]
    big = np.where(rows[:, None, None] == 0, row[None], row[None, ::-1])
    L = np.ascontiguousarray(big[:, 32:32 + W])
    R = np.ascontiguousarray(big[:, 32 + 5:32 + 5 + W])
    return L, R


# (L // 8 + 100, the low-contrast recipe of test_large_windows_against_the_oracle, has no pixel below fp32 resolution at these
# sizes: not a tie-rich input)
GENERATORS = {"quantised": quantised, "black_margins": black_margins, "patches": patches}


def shifted_noisy(H, W, maxd, seed):
    """the recipe of tests/test_gpu_fuzz.py::_shifted_pair: low-contrast smooth texture and a shifted copy with noise of -2 .. 2
    on every channel -- candidates are rarely saturated, and many lie a few cost-image ulps apart without tying exactly"""
    rng = np.random.default_rng(seed)
    L = make_pair(H, W, 8, seed)[0]
    L = (110 + (L.astype(np.int32) - 128) // 6).astype(np.uint8)
    d0 = int(rng.integers(0, max(0, min(maxd, W // 2)) + 1))
    R = np.roll(L, -d0, axis=1).astype(np.int32) + rng.integers(-2, 3, size=L.shape)
    return np.ascontiguousarray(L), np.ascontiguousarray(np.clip(R, 0, 255).astype(np.uint8))


def stripes(H, W, maxd, seed):
    """every row one colour (a textureless scene: all candidates of a pixel see the same windows), the right view one level
    brighter in one channel: every tap has TAD 1 and every candidate away from the left border costs exactly 1.  For
    `perturbed`: a step in a row of another colour moves a cost by that row's (small) weight -- near-ties that are not exact"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(8, 248, (H, 1, 3))
    L = np.ascontiguousarray(np.broadcast_to(rows, (H, W, 3)).astype(np.uint8))
    R = L.copy()
    R[:, :, rng.integers(0, 3)] += 1
    return L, R


def soft_stripes(H, W, maxd, seed):
    """stripes whose row colours are a random walk of up to 12 levels per channel and row: neighbouring rows lie a few Lab
    units apart, so that at gammaC = 0.7 (where a row of stripes()'s colours weighs 1e-60) a step in the next row still moves a cost"""
    rng = np.random.default_rng(seed)
    rows = np.clip(128 + np.cumsum(rng.integers(-12, 13, (H, 1, 3)), axis=0), 8, 247)
    L = np.ascontiguousarray(np.broadcast_to(rows, (H, W, 3)).astype(np.uint8))
    R = L.copy()
    R[:, :, rng.integers(0, 3)] += 1
    return L, R


GENERATORS["shifted_noisy"] = shifted_noisy
GENERATORS["stripes"] = stripes
GENERATORS["soft_stripes"] = soft_stripes


def perturbed(kind, H, W, maxd, seed, share=0.02):
    """generator `kind` with +-1 on one channel of about 2 % of the right view's pixels: its exact ties (identical windows, whose
    fp32 and fp64 costs differ by the same amount) become near-ties that are not exact"""
    L, R = GENERATORS[kind](H, W, maxd, seed)
    rng = np.random.default_rng(seed + 7919)
    ys, xs = np.nonzero(rng.random((H, W)) < share)
    ch = rng.integers(0, 3, ys.size)
    step = rng.integers(0, 2, ys.size) * 2 - 1
    R = R.astype(np.int32)
    R[ys, xs, ch] += step
    return L, np.ascontiguousarray(np.clip(R, 0, 255).astype(np.uint8))


def pair(kind, H, W, maxd, seed=1):
    """`kind`: a generator's name, or "perturbed:<name>" """
    if kind.startswith("perturbed:"):
        return perturbed(kind.split(":", 1)[1], H, W, maxd, seed)
    return GENERATORS[kind](H, W, maxd, seed)


def taps(L, p):
    H, W = L.shape[:2]
    return H * W * (p["maxDisparity"] - p.get("minDisparity", 0) + 1) * p["winSize"] ** 2


class OracleCache:
    """oracle.asw once per (input, params); every kernel form of a module reuses the map (and the costs, if asked for)"""

    def __init__(self):
        self._maps = {}

    def asw(self, L, R, return_costs=False, **p):
        assert taps(L, p) <= MAX_TAPS, ("oracle call too large", L.shape, p)
        key = (L.shape, L.tobytes(), R.tobytes(), tuple(sorted(p.items())), bool(return_costs))
        if key not in self._maps:
            from oracle import oracle
            self._maps[key] = oracle.asw(L, R, nthreads=nthreads(), return_costs=return_costs, **p)
        return self._maps[key]


def sat_abs(win):
    """the absolute band of the saturated side (cost > 20) of the near-tie rule, as asw_exact_prepare computes it"""
    return float(np.float32(1.5 * 2.0 * 2.0 * (win * win + 3.0) * 1.1102230246251565e-16 * 40.0))


def tol(win, gammaC, exact_tol=128):
    """rule (a)'s band in cost-image ulps, as asw_exact_prepare computes it"""
    return int(min(1.0e6, exact_tol * max(1.0, 5.0 / gammaC) * max(1.0, win / 35.0)))


def fp32_unresolved(costs, win):
    """pixels whose best two fp64 costs lie closer than fp32 resolves them: within 1e-5 relative below cost 20, within
    sat_abs(win) above it (costs: the oracle's [H][W][nD], NaN where a candidate does not exist)"""
    c = np.where(np.isnan(costs), np.inf, costs)
    two = np.sort(c, axis=2)[:, :, :2] if c.shape[2] >= 2 else np.full(c.shape[:2] + (2,), np.inf)
    a, b = two[..., 0], two[..., 1]
    ok = np.isfinite(b)
    low = ok & (a <= 20.0) & (b - a <= 1e-5 * np.maximum(a, 1e-30))
    high = ok & (a > 20.0) & (b - a <= sat_abs(win))
    return int(np.count_nonzero(low | high))


# ---- a lone zero-cost winner -----------------------------------------------------------------------------------------------
# One row; window 13; the left pixel X is black (A) between a grey U and a white V, everything else a saturated blue F whose
# weights are below 1e-50.  gammaC puts V's colour distance from A at 87.6 gammaC: exp(-87.6) = 2^-126.4, which v_exp_f32
# flushes to 0 -- in fp64 it is 9.2e-39.
#   D0: right taps U, A, A -> TAD 0, 0, 40; the TAD-40 tap has the flushed weight: fp32 cost exactly 0, fp64 cost 3.2e-37.
#   D1: right taps U', A, V (U' = U + 1 in blue) -> TAD 1, 0, 0; the TAD-1 tap weighs exp(-42.8) * exp(-42.8) = 6.7e-38
#       (both factors normal): fp32 and fp64 cost 6.0e-38 -- the reference's argmin, 8e6 cost-image ulps above 0.
# Every other candidate of X costs 40 or 9.4e-18.
LZ_X, LZ_D0, LZ_D1 = 30, 3, 19


def lone_zero_pair():
    from oracle import oracle

    def lab(c):
        return oracle.bgr2lab(np.array([[c]], np.uint8))[0, 0]
    A, V, F, U, U1 = (0, 0, 0), (255, 255, 255), (255, 0, 0), (116, 116, 116), (117, 116, 116)
    gammaC = float(np.linalg.norm(lab(V) - lab(A))) / 87.6
    W, x, d0, d1 = 48, LZ_X, LZ_D0, LZ_D1
    L = np.array([F] * W, np.uint8)
    R = L.copy()
    L[x - 1], L[x], L[x + 1] = U, A, V
    R[x - d0 - 1], R[x - d0], R[x - d0 + 1] = U, A, A
    R[x - d1 - 1], R[x - d1], R[x - d1 + 1] = U1, A, V
    p = dict(winSize=13, maxDisparity=20, minDisparity=0, gammaC=gammaC, gammaP=17.5)
    return np.ascontiguousarray(L[None]), np.ascontiguousarray(R[None]), p


def zero_floor(win):
    """rule (d)'s Z: the largest fp64 cost of a candidate whose fp32 cost flushed to 0, times 2"""
    return win * win * 40.0 * 2.0 ** -126 * 2.0

