"""The fp32 cost images of the ASW aggregation kernels against the near-tie band of the fp64 tie-break pass: reference image,
measured set, near pairs, a plain fp32 emulation and the case matrix.  Helper module, not a test (tests/test_asw_band_cpu.py,
tests/test_gpu_asw_band.py and tests/golden/make_golden_asw_band.py use it).

The band (asw_exact_prepare, mirrored by _tie_inputs.tol) is counted in ulps of the 32-bit cost IMAGE of asw_cost_key:
    cost <= 20:  bits(float32(cost))                    cost > 20:  0xC0000000 - bits(float32(40 - cost))
A candidate is re-decided in fp64 only if its image lies within `tol` of the fp32 winner's.  With i32 / i64 the kernel's and the
reference's image of a candidate, d* the reference's first minimum and c any other candidate, the band is sufficient when
    D(c) = (i32(d*) - i32(c)) - (i64(d*) - i64(c)) <= tol:
i64(d*) <= i64(c), so i32(d*) - i32(c) <= tol for EVERY c, the fp32 winner included -- d* is always queued.
Rule (d) of exact_near queues a candidate on its own image: i32(d*) <= zkey(win), the image of Z = 2 win^2 40 2^-126.  It is there
because v_exp_f32 returns 0 for a weight below 2^-126: a cost of 1e-38 made of such weights is 0, or wrong by a binade or two,
in fp32, and no band counted in ulps covers that.  So a near pair is of the BAND class when i32(d*) > zkey -- D <= tol is what
gets d* queued -- and of the FLOOR class otherwise, where rule (d) does and D is reported only.

The measured set.  The oracle returns the quotient num / den only, each a sum of n = win^2 fp64 terms: a relative rounding noise
of about (n + 3) u on each, u = 2^-53, together 2 (n + 3) u relative, i.e. at most 2 (n + 3) u 40 absolute.  At the largest
allowed window (255: n = 65 025) that is 1.45e-11 relative, 5.8e-10 absolute.  Below cost 20 an image ulp is at least 2^-24
relative (6.0e-8): the noise is under 2.5e-4 ulps.  Between 20 and 39 the image holds 40 - cost in [1, 20), whose ulp is at
least 2^-23 = 1.19e-7 absolute: the noise is under 4.9e-3 ulps -- below 1/16 of an image ulp for every window up to 255.  Above
39 the ulp of 40 - cost shrinks without bound while the noise does not: such candidates belong to rule (b) (sat_abs) and are
left to the exact-mode map tests.  A candidate whose two images lie either side of cost 20 (rule (c)'s seam, where the image
changes form) is not measured either; a pair enters a measure only if all four images lie on one side."""
import numpy as np

import _tie_inputs as T
from _asw_forms import FORMS        # noqa: F401  (the case matrix names its forms)

NONE32 = 0xFFFFFFFF                    # the dump's word where a candidate does not exist
HIGH = 0xC0000000 - 0x41A00000         # images at or above this hold 40 - cost (EXACT_KEY_HIGH)
MEASURED_MAX = 39.0
NEAR_FACTOR = 8                        # a near pair's fp64 image gap is at most this many bands
MIN_PAIRS = 200                        # a case of the differential measure has at least this many near pairs
E_FLOOR = 8                            # per-candidate bar: 2 x max(emulation's E max, this many ulps)


def _bits(f32):
    return np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.int64)


def image64(cost):
    """cost image (int64; -1 where the candidate does not exist) of the fp64 oracle's costs"""
    c = np.asarray(cost, np.float64)
    ok = ~np.isnan(c)
    cz = np.where(ok, c, 0.0)
    low = _bits(cz.astype(np.float32))
    high = 0xC0000000 - _bits((40.0 - cz).astype(np.float32))
    return np.where(ok, np.where(cz <= 20.0, low, high), -1)


def image32(dump):
    """the kernels' dump (SSAMD_ASW_COST_KEYS=1: bit patterns in a float32 array) as int64; -1 where no candidate exists"""
    w = np.ascontiguousarray(dump).view(np.uint32).astype(np.int64)
    return np.where(w == NONE32, -1, w)


def measured(cost, i32, i64):
    """the measured set: the candidate exists, costs at most 39 and both of its images lie on one side of 20"""
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(cost) & (cost <= MEASURED_MAX)
    return ok & (i32 >= 0) & ((i32 >= HIGH) == (i64 >= HIGH))


def first_minimum(cost):
    """[H][W] index of the oracle's first minimum (its strict `<` scan from the smallest disparity); every pixel has a candidate
    when minDisparity is 0"""
    return np.argmin(np.where(np.isnan(cost), np.inf, cost), axis=2)


def near_pairs(cost, tol, i64=None):
    """[H][W][nD] mask of the candidates c that form a near pair (d*, c): the fp64 image gap is nonzero and at most 8 tol, both
    images lie on the same side of 20 and both costs are at most 39.  Returns (mask, d*)."""
    i64 = image64(cost) if i64 is None else i64
    ds = first_minimum(cost)
    cs = np.take_along_axis(cost, ds[..., None], 2)
    ws = np.take_along_axis(i64, ds[..., None], 2)
    gap = i64 - ws
    with np.errstate(invalid="ignore"):
        m = (i64 >= 0) & (ws >= 0) & (gap != 0) & (gap <= NEAR_FACTOR * tol) & ((i64 >= HIGH) == (ws >= HIGH)) & \
            (cost <= MEASURED_MAX) & (cs <= MEASURED_MAX)
    return m, ds


def zkey(win):
    """rule (d)'s floor as exact_zkey computes it: the image of Z = 2 win^2 40 2^-126.  A candidate whose fp32 image is at most
    this is queued whatever the winner's image, so the band (rule (a)) has nothing to cover for it."""
    return int((np.float32(win * win) * np.float32(9.4039548065783e-37)).reshape(1).view(np.uint32)[0])


def candidate_error(cost, i32, above=-1):
    """E = |image32 - image64| over the measured set, or over its candidates whose fp64 image lies above `above`:
    (max, 99.9th percentile, number measured)"""
    i64 = image64(cost)
    m = measured(cost, i32, i64) & (i64 > above)
    e = np.abs(i32[m] - i64[m])
    if e.size == 0:
        return 0, 0.0, 0
    return int(e.max()), float(np.percentile(e, 99.9)), int(e.size)


def differential_error(cost, i32, tol, zk):
    """D over the near pairs whose fp32 images also lie on the pair's side of 20, in two classes.  Band: the winner's fp32 image
    lies above rule (d)'s floor `zk`, so only D <= tol gets it queued.  Floor: it does not, and rule (d) queues it whatever D
    is.  Returns (max D, pairs) of the band class and (max D, pairs) of the floor class."""
    i64 = image64(cost)
    m, ds = near_pairs(cost, tol, i64)
    w64 = np.take_along_axis(i64, ds[..., None], 2)
    w32 = np.take_along_axis(i32, ds[..., None], 2)
    m = m & (i32 >= 0) & (w32 >= 0) & ((i32 >= HIGH) == (i64 >= HIGH)) & ((w32 >= HIGH) == (w64 >= HIGH))
    d = (w32 - i32) - (w64 - i64)
    out = []
    for cls in (m & (w32 > zk), m & (w32 <= zk)):
        out += [int(d[cls].max()) if cls.any() else 0, int(np.count_nonzero(cls))]
    return tuple(out)


def emulate32(L, R, p):
    """What the kernels are meant to compute, in plain numpy float32: float32 Lab records, weights exp2(kC dist) times the float32
    proximity table (an exp2 below 2^-126 is 0, as the hardware instruction returns it), w = wl wr, sequential float32 sums of
    w e and w (40 - e) over the window in raster order, asw_cost_key's image.  Returns the images as image32 does.  The
    yardstick of the per-candidate bar -- not a bit model of any kernel (their tap order and fused multiply-adds differ)."""
    from oracle import oracle
    f32 = np.float32
    H, W = L.shape[:2]
    win, minD, maxD = p["winSize"], p.get("minDisparity", 0), p["maxDisparity"]
    pad, nD = win // 2, maxD - minD + 1
    labL, labR = oracle.bgr2lab(L).astype(f32), oracle.bgr2lab(R).astype(f32)
    kC = f32(-1.4426950408889634 / p["gammaC"])
    k = np.arange(win) - pad
    prox = np.exp(-np.sqrt((k[:, None] ** 2 + k[None, :] ** 2).astype(np.float64)) / p["gammaP"]).astype(f32)
    xr = np.arange(W)[:, None] - (minD + np.arange(nD))[None, :]                # [W][nD] right column of candidate (x, d)
    exists = xr >= 0
    xrc = np.where(exists, xr, 0)
    tad = np.abs(L[:, :, None, :].astype(np.int32) - R[:, xrc, :].astype(np.int32)).sum(-1)
    e = np.where(exists[None], np.minimum(tad, 40), 0).astype(f32)              # [H][W][nD]
    accN, accS = np.zeros((H, W, nD), f32), np.zeros((H, W, nD), f32)
    tiny = f32(2.0 ** -126)

    def weights(lab, dy, dx, pr):
        """[H][W] weight of the tap (dy, dx) of every centre; 0 where the tap lies outside the image"""
        w = np.zeros((H, W), f32)
        y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        if y0 < y1 and x0 < x1:
            d = lab[y0 + dy:y1 + dy, x0 + dx:x1 + dx] - lab[y0:y1, x0:x1]
            dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
            ex = np.exp2(dist * kC)
            w[y0:y1, x0:x1] = pr * np.where(ex < tiny, f32(0), ex)             # v_exp_f32 returns no denormals
        return w

    et = np.zeros_like(e)
    for i in range(win):
        dy = i - pad
        if dy <= -H or dy >= H:
            continue
        for j in range(win):
            dx = j - pad
            if dx <= -W or dx >= W:
                continue
            wl, wr = weights(labL, dy, dx, prox[i, j]), weights(labR, dy, dx, prox[i, j])
            # the tap of candidate (x, d): left column x + dx, right column x - d + dx; outside either image one factor is 0
            w = wl[:, :, None] * np.where(exists[None], wr[:, xrc], f32(0))
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            et[:] = 0
            et[y0:y1, x0:x1] = e[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            accN += w * et
            accS += w * (f32(40) - et)
    with np.errstate(invalid="ignore", divide="ignore"):
        t40 = accN + accS
        low = accN <= accS
        img = np.where(low, _bits(f32(40) * accN / t40), 0xC0000000 - _bits(f32(40) * accS / t40))
    return np.where(exists[None], img, -1)


# ---- the case matrix ----------------------------------------------------------------------------------------------------------
# Kernel forms: the catalogue of tests/_asw_forms.py, by name.
# name: generator (of _tie_inputs), shape, seed, params (minDisparity 0), forms, differential measure or per candidate only
CASES = {}


def _case(name, kind, H, W, seed, win, maxd, gammaC, gammaP, forms, differential=True):
    CASES[name] = dict(generator=kind, shape=[H, W], seed=seed, forms=list(forms), differential=differential,
                       params=dict(winSize=win, maxDisparity=maxd, minDisparity=0, gammaC=gammaC, gammaP=gammaP))


# The three "flush" cases: at gammaC = 0.7 the perturbed patches have thousands of candidates whose fp64 cost is 1e-38 or less --
# every tap with TAD > 0 has a weight that exp2 flushed.  Their fp32 images are off by up to 3e7 ulps (the kernels and the
# emulation agree on that to the ulp), and rule (d) exists for them: their near pairs are of the floor class.
S, F, P, N = "perturbed:stripes", "perturbed:soft_stripes", "perturbed:patches", "shifted_noisy"
#     name               input  H    W  seed win maxd gammaC gammaP forms
_case("w35_g5_wave4",      S,  16,  96, 3,  35,  19,  5.0,  17.5, ("planner", "wave4", "workgroup"))        # the bench's parameters
_case("w35_g5_pipe",       S,  12, 140, 3,  35,  71,  5.0,  17.5, ("planner", "pipe", "pipe_evol0", "workgroup"))
_case("w35_g5_noisy",      N,  12, 140, 3,  35,  39,  5.0,  17.5, ("planner", "wave8", "workgroup"), differential=False)
_case("w35_g0.7_wave8",    F,  12, 100, 3,  35,  39,  0.7,  17.5, ("planner", "wave8", "workgroup"))
_case("w35_g0.7_flush",    P,   8, 300, 3,  35,  39,  0.7,  17.5, ("planner", "workgroup"), differential=False)
_case("w35_g50_pipe",      S,  12, 140, 3,  35,  71, 50.0,   3.0, ("pipe", "workgroup"))
_case("w9_g0.7_wave6",     F,  24, 128, 3,   9,  17,  0.7,   3.0, ("planner", "wave6", "wave4x5", "workgroup"))
_case("w9_g0.7_flush",     P,  24, 128, 3,   9,  17,  0.7,   3.0, ("wave6", "workgroup"), differential=False)
_case("w255_g5",           S,   4, 280, 3, 255,   3,  5.0, 100.0, ("planner", "workgroup"))
_case("w151_g0.7",         S,   6, 200, 3, 151,   7,  0.7,  17.5, ("planner", "workgroup"))
_case("w3_g5_chunks",      N,   8, 640, 3,   3, 599,  5.0,   3.0, ("chunks",), differential=False)
_case("w21_g5_pipe",       S,  12, 140, 3,  21,  71,  5.0, 100.0, ("planner", "pipe8", "pipe8_evol0"))
_case("w61_g50",           S,  10, 140, 3,  61,  11, 50.0, 100.0, ("planner", "workgroup"))
_case("w21_g0.7_wave8",    F,  16, 200, 3,  21,  29,  0.7, 100.0, ("wave8", "workgroup"))
_case("w21_g0.7_flush",    P,  16, 200, 3,  21,  29,  0.7, 100.0, ("wave8", "workgroup"), differential=False)
_case("w9_g50_wave4",      N,  24, 128, 3,   9,  19, 50.0,  17.5, ("wave4", "workgroup"), differential=False)
_case("w61_g5_pipe",       S,   6, 150, 3,  61,  65,  5.0,   3.0, ("pipe", "workgroup"))
del S, F, P, N


def case_inputs(name):
    c = CASES[name]
    H, W = c["shape"]
    L, R = T.pair(c["generator"], H, W, c["params"]["maxDisparity"], seed=c["seed"])
    return L, R, dict(c["params"])


def case_tol(name):
    p = CASES[name]["params"]
    return T.tol(p["winSize"], p["gammaC"])
