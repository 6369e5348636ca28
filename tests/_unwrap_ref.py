"""Plain-Python restatement of the reference's infinite-impulse-response phase unwrapper
(``simplestereo._unwrapping.infiniteImpulseResponse``), written from its specification, with every
visited flag starting at zero (what the reference computes whenever its flag allocation does not
corrupt the heap).

All arithmetic is Python floats (IEEE fp64, one rounding per operation, no fused multiply-adds) and
``math.fmod`` (C fmod, exact).  ``W(a) = r - pi if r >= 0 else r + pi`` with ``r = fmod(a + pi, 2 pi)``.
A step at (y, x) averages ``u + tau * W(cur - u)`` over the flagged pixels of the clipped 3x3 window in
row-major order (``temp`` starts at 0.0 and is divided by the count, or ``cur`` when nothing is flagged).
Passes: row 0 forward, row 0 backward down to x = 1, then every row forward; the flag is set after the
step.  Slow (a few microseconds per pixel): for test-sized maps.
"""
import math

import numpy as np

_PI = math.pi
_TWO_PI = 2 * math.pi


def _W(a):
    v = a + _PI
    r = math.fmod(v, _TWO_PI) if math.isfinite(v) else math.nan     # (C fmod of +-inf is NaN; math.fmod raises)
    return r - _PI if r >= 0 else r + _PI


def identical(a, b):
    """Bit-for-bit equality of two float64 arrays, NaN payloads aside: NaN in the same places, every other value's bits equal."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


def unwrap(phase, tau=1.0):
    """float64 [h, w] -> float64 [h, w] (a new array); ``phase`` is read as float64."""
    ph = np.asarray(phase, dtype=np.float64)
    h, w = ph.shape
    tau = float(tau)
    rows = ph.tolist()
    u = [[0.0] * w for _ in range(h)]
    flag = [[False] * w for _ in range(h)]

    def step(y, x):
        cur = rows[y][x]
        temp, S = 0.0, 0
        for i in range(max(0, y - 1), min(y + 2, h)):
            fi, ui = flag[i], u[i]
            for j in range(max(0, x - 1), min(x + 2, w)):
                if fi[j]:
                    S += 1
                    temp += ui[j] + tau * _W(cur - ui[j])
        u[y][x] = temp / S if S > 0 else cur

    if h > 0:
        for x in range(w):
            step(0, x)
            flag[0][x] = True
        for x in range(w - 1, 0, -1):
            step(0, x)
            flag[0][x] = True
    for y in range(h):
        for x in range(w):
            step(y, x)
            flag[y][x] = True
    return np.array(u, dtype=np.float64).reshape(h, w)
