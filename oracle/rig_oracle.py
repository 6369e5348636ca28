"""oracle/rig_oracle.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Independent CPU restatements (plain per-pixel Python/numpy loops, deliberately NOT sharing code
with simplestereo_amd/_rigs.py) of the two OpenCV calls around the matching path that the
reference makes and that this repo runs as HIP kernels:

  remap_bilinear  -- cv2.remap(img, mapx, mapy, INTER_LINEAR / INTER_NEAREST, BORDER_CONSTANT 0),
                     called by RectifiedStereoRig.rectifyImages (reference _rigs.py:564-565)
  reproject       -- cv2.reprojectImageTo3D(disparity, Q) called by get3DPoints (_rigs.py:628)
  reproject_exact / reproject_longdouble -- the same in exact rational arithmetic (sampled pixels) and in
                     numpy.longdouble (whole frames), with the error bound derived for an fp64 evaluation

PARITY UNPINNED: OpenCV is not installed in this environment, so these restatements of the
published OpenCV semantics (imgwarp.cpp: map coordinates cvRound-ed to 1/32 pixel, 15-bit integer bilinear
weights summing to 32768, FixedPtCast (sum + 16384) >> 15 so that ties round up; homogeneous divide)
cannot be checked against cv2 itself.  They pin the HIP kernels and the numpy host path against
each other only.  Only tests/ may import this module.
"""
import math
from fractions import Fraction

import numpy as np


_INT_MIN = -2 ** 31


def cv_round(v):
    """OpenCV's cvRound of a double on x86 (cvtsd2si): round half to even; NaN, +-inf and every value whose rounding leaves
    the int32 range give INT_MIN ("integer indefinite")."""
    if not math.isfinite(v):
        return _INT_MIN
    r = round(v)                                           # Python: exact, half to even
    return r if -2 ** 31 <= r < 2 ** 31 else _INT_MIN


def _saturate_short(v):
    return max(-32768, min(32767, v))


def remap_bilinear(img, mapx, mapy, nearest=False):
    """Out-of-range coordinates are DEFINED here, once, by OpenCV's published conversion of float maps:
    ``saturate_cast<short>(cvRound(v * 32) >> 5)`` (nearest: ``saturate_cast<short>(cvRound(v))``).  NaN, +-inf and any
    v with |v * 32| >= 2^31 (|v| >= 2^26; nearest: |v| >= 2^31) become INT_MIN, i.e. a cell at or below -32768: outside every
    image, so the pixel is the constant border value 0.  The saturation to short never moves a cell into an image
    (sources here are narrower than 32767 pixels)."""
    img = np.asarray(img)
    Hs, Ws = img.shape[:2]
    H, W = mapx.shape
    out = np.zeros((H, W, img.shape[2]), np.uint8)
    for y in range(H):
        for x in range(W):
            mx, my = float(mapx[y, x]), float(mapy[y, x])
            if nearest:
                xi, yi = _saturate_short(cv_round(mx)), _saturate_short(cv_round(my))
                if 0 <= xi < Ws and 0 <= yi < Hs:
                    out[y, x] = img[yi, xi]
                continue
            qx, qy = cv_round(mx * 32.0), cv_round(my * 32.0)
            x0, y0 = _saturate_short(qx >> 5), _saturate_short(qy >> 5)      # floor division, also for negatives
            fx, fy = qx & 31, qy & 31
            # OpenCV's BilinearTab_i entry for (fy, fx): shorts, round(weight * 32768), here exact
            tab = [[(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32], [fy * (32 - fx) * 32, fy * fx * 32]]
            for ch in range(img.shape[2]):
                total = 0
                for dy in (0, 1):
                    for dx in (0, 1):
                        xx, yy = x0 + dx, y0 + dy
                        if 0 <= xx < Ws and 0 <= yy < Hs:
                            total += tab[dy][dx] * int(img[yy, xx, ch])
                out[y, x, ch] = min(255, max(0, (total + (1 << 14)) >> 15))
    return out


def reproject(disparity, Q):
    d = np.asarray(disparity)
    H, W = d.shape
    Q = np.asarray(Q, dtype=np.float64)
    out = np.empty((H, W, 3), np.float32)
    for y in range(H):
        for x in range(W):
            v = Q.dot(np.array([x, y, float(d[y, x]), 1.0]))
            w = v[3]
            out[y, x] = [v[0] / w if w != 0 else math.copysign(math.inf, v[0]) if v[0] != 0 else math.nan,
                         v[1] / w if w != 0 else math.copysign(math.inf, v[1]) if v[1] != 0 else math.nan,
                         v[2] / w if w != 0 else math.copysign(math.inf, v[2]) if v[2] != 0 else math.nan]
    return out


# ---------------------------------------------------------------- high-precision reprojection
# The kernel evaluates Q [x y d 1]^T in fp64 (possibly contracted into fmas) and forms each quotient from one reciprocal with
# one fma correction.  With t the exact component, kX = sum|terms| / |sum terms| of its numerator and kW likewise of the
# denominator, the derived bound is
#     |got - t| <= 0.5 ulp32(t) + |t| * 8 * 2^-53 * (kX + kW)
# (8 covers four products, three sums and the refined quotient of each of the two dot products; 0.5 ulp32 is the final
# rounding to float32).  |t| * kX = sum|numerator terms| / |W| keeps the bound defined where the numerator cancels to 0.
_FLT_MAX = Fraction(float(np.finfo(np.float32).max))
_EPS64 = Fraction(1, 2 ** 53)


def _ulp32(t):
    """ulp of float32 in the binade of |t| (a Fraction); 2^-149 below the normal range"""
    a = abs(t)
    if a == 0:
        return Fraction(1, 2 ** 149)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1                                             # 2^e <= a < 2^(e+1)
    return Fraction(2) ** max(e - 23, -149)


def reproject_exact(Q, x, y, d):
    """One pixel in exact rational arithmetic on the doubles of Q and the integers x, y, d.  Returns three entries, each
    ("value", t, tol) with t and the derived tolerance as Fractions, ("inf", sign) where the exact W is 0 or |t| exceeds
    the float32 range, or ("nan",) where W and the numerator are both 0."""
    Q = np.asarray(Q, dtype=np.float64)
    v = (Fraction(int(x)), Fraction(int(y)), Fraction(int(d)), Fraction(1))
    terms = [[Fraction(float(Q[r, c])) * v[c] for c in range(4)] for r in range(4)]
    Wc = sum(terms[3])
    aW = sum(abs(a) for a in terms[3])
    out = []
    for r in range(3):
        n = sum(terms[r])
        aN = sum(abs(a) for a in terms[r])
        if Wc == 0:
            out.append(("nan",) if n == 0 else ("inf", 1 if n > 0 else -1))
            continue
        t = n / Wc
        tol = _ulp32(t) / 2 + 8 * _EPS64 * (aN / abs(Wc) + abs(t) * aW / abs(Wc))
        if abs(t) - tol > _FLT_MAX + _ulp32(_FLT_MAX) / 2:
            out.append(("inf", 1 if t > 0 else -1))
        else:
            out.append(("value", t, tol))
    return out


def reproject_check_exact(got, Q, x, y, d):
    """None when the three float32 values `got` of pixel (x, y) with disparity d satisfy the derived bound, else a message"""
    for r, want in enumerate(reproject_exact(Q, x, y, d)):
        g = float(got[r])
        if want[0] == "nan":
            ok = math.isnan(g)
        elif want[0] == "inf":
            ok = math.isinf(g) and (g > 0) == (want[1] > 0)
        elif math.isinf(g):                                # only where the exact value rounds to infinity within the bound
            ok = abs(want[1]) + want[2] >= _FLT_MAX + _ulp32(_FLT_MAX) / 2 and (g > 0) == (want[1] > 0)
        else:
            ok = (not math.isnan(g)) and abs(Fraction(g) - want[1]) <= want[2]
        if not ok:
            return "pixel (x=%d, y=%d, d=%d) component %d: got %r, want %s" % (
                x, y, d, r, g, want[0] if want[0] != "value" else "%.17g +- %.3g" % (float(want[1]), float(want[2])))
    return None


def reproject_longdouble(disparity, Q, rows=None):
    """Whole frame in numpy.longdouble (64-bit significand on x86); `rows` gives the image row of each row of `disparity`
    when that is a selection of rows (default 0 .. H-1).  Returns (t, tol, cls): t [H,W,3] longdouble, tol the
    derived bound plus this evaluation's own error (the same expression with 2^-64 for 2^-53 -- products of a double and a
    16-bit integer are not exact in 64 bits), cls [H,W,3] int8: 0 value, +1 / -1 infinity of that sign, 2 NaN (exact W = 0:
    the sum of longdouble terms is exactly 0 only where the test's Q makes every term exact)."""
    LD = np.longdouble
    d = np.asarray(disparity)
    H, W = d.shape
    Ql = np.asarray(Q, dtype=np.float64).astype(LD)
    yy, xx = np.meshgrid(np.arange(H) if rows is None else np.asarray(rows), np.arange(W), indexing="ij")
    v = np.stack([xx.astype(LD), yy.astype(LD), d.astype(LD), np.ones((H, W), LD)], -1)            # [H,W,4]
    terms = v[:, :, None, :] * Ql[None, None, :, :]                                                 # [H,W,4,4]
    s = terms.sum(-1)
    a = np.abs(terms).sum(-1)
    Wc, aW = s[..., 3:4], a[..., 3:4]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = s[..., :3] / Wc
        at = np.abs(t)
        e = np.floor(np.log2(np.where(at > 0, at, LD(1)))).astype(LD)
        e = np.where(LD(2) ** e > at, e - 1, e)                                                     # log2 rounding at binade edges
        ulp = LD(2) ** np.maximum(e - 23, -149)
        ulp = np.where(at > 0, ulp, LD(2) ** -149)
        tol = ulp / 2 + (LD(8) * LD(2) ** -53 + LD(8) * LD(2) ** -64) * (a[..., :3] / np.abs(Wc) + at * aW / np.abs(Wc))
    cls = np.zeros((H, W, 3), np.int8)
    zero = np.broadcast_to(Wc == 0, cls.shape)
    n = s[..., :3]
    cls[zero & (n > 0)] = 1
    cls[zero & (n < 0)] = -1
    cls[zero & (n == 0)] = 2
    fmax = LD(np.finfo(np.float32).max)
    with np.errstate(invalid="ignore"):
        big = ~zero & (at - tol > fmax * (1 + LD(2) ** -24))
    cls[big & (t > 0)] = 1
    cls[big & (t < 0)] = -1
    return t, tol, cls


def reproject_check_longdouble(got, disparity, Q, rows=None):
    """Number of components of the float32 frame `got` [H,W,3] outside the bound of reproject_longdouble, and the first few
    (row of `got`, x, component)"""
    t, tol, cls = reproject_longdouble(disparity, Q, rows)
    g = np.asarray(got)
    gl = g.astype(np.longdouble)
    with np.errstate(invalid="ignore"):
        fmax = np.longdouble(np.finfo(np.float32).max)
        ok_val = np.isfinite(g) & (np.abs(gl - t) <= tol)
        ok_val |= np.isinf(g) & (np.sign(gl) == np.sign(t)) & (np.abs(t) + tol >= fmax)             # rounds to infinity within the bound
        ok = np.where(cls == 0, ok_val, np.where(cls == 2, np.isnan(g), np.isinf(g) & (np.sign(gl) == cls)))
    bad = np.argwhere(~ok)
    return len(bad), [tuple(int(i) for i in b) for b in bad[:5]]
