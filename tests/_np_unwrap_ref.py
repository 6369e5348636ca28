"""A plain sequential restatement of np.unwrap's float path (numpy/lib/_function_base_impl.py), the arithmetic
csrc/np_unwrap_kernels.hip.h reproduces, plus the inputs and the comparison tests/test_np_unwrap_cpu.py and
tests/test_gpu_np_unwrap.py share.  The oracle of those tests is np.unwrap itself; this file documents the contract -- every
operation fp64 and rounded once, the running sum strictly left to right -- and catches a numpy whose unwrap differs."""
import numpy as np

PI = np.pi
# (discont, period) pairs every tier runs
PARAMS = [(None, 2 * PI), (PI, 2 * PI), (0.0, 2 * PI), (10.0, 2 * PI), (1.0, 2 * PI), (None, 1.0), (None, 360.0), (np.nan, 2 * PI)]


def unwrap_ref(p, discont=None, axis=-1, period=2 * PI):
    p = np.asarray(p, dtype=np.float64)
    hi = period / 2
    lo = -hi
    if discont is None:
        discont = hi
    q = np.moveaxis(p, axis, 0)                       # the scanned axis first; every other index is a line of its own
    out = np.array(q, copy=True)                      # out[0] = p[0]
    s = None
    with np.errstate(all="ignore"):
        for i in range(1, q.shape[0]):
            dd = q[i] - q[i - 1]
            m = np.fmod(dd - lo, period)              # C fmod: the exact remainder, sign of the dividend
            m = np.where((m != 0) & (m < 0), m + period, m)
            m = np.where(m == 0, 0.0, m)              # np.mod gives +0.0 for a positive divisor
            ddmod = m + lo
            ddmod = np.where((ddmod == lo) & (dd > 0), hi, ddmod)
            c = ddmod - dd
            c = np.where(np.abs(dd) < discont, 0.0, c)
            s = c if s is None else s + c             # sequential: one rounded add per sample
            out[i] = q[i] + s
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def blocked_unwrap(p, block, axis=-1):
    """np.unwrap's corrections summed in blocks of `block` samples plus block offsets: the order a blocked or tree scan uses.
    NOT what numpy computes -- the order-sensitivity tests assert that it differs."""
    q = np.moveaxis(np.asarray(p, dtype=np.float64), axis, 0)
    dd = np.diff(q, axis=0)
    ddmod = np.mod(dd + PI, 2 * PI) - PI
    np.copyto(ddmod, PI, where=(ddmod == -PI) & (dd > 0))
    c = ddmod - dd
    np.copyto(c, 0.0, where=np.abs(dd) < PI)
    s = np.empty_like(c)
    offset = np.zeros(c.shape[1:])
    for k0 in range(0, c.shape[0], block):
        part = np.cumsum(c[k0:k0 + block], axis=0)
        s[k0:k0 + block] = offset + part
        offset = offset + part[-1]
    out = np.array(q, copy=True)
    out[1:] = q[1:] + s
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def equal(a, b):
    """Same shape and dtype, NaN at the same positions, identical 64-bit patterns everywhere else (the sign of zero counts)."""
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype != np.float64:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    ua, ub = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
    return bool(np.array_equal(ua[~na], ub[~nb]))


def differing_fraction(a, b):
    return float(np.mean(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))


def _along(shape, axis, line):
    """Broadcast a 1-D pattern along `axis` of `shape`."""
    idx = [None] * len(shape)
    idx[axis] = slice(None)
    return np.ascontiguousarray(np.broadcast_to(line[tuple(idx)], shape))


def steep_ramp(shape, axis, seed=0):
    """angle(exp(1j (2.9 k + N(0, 0.1)))) along the scanned axis: a jump at about half the samples, sums of hundreds of radians
    whose roundings tell a sequential sum from a blocked one."""
    rng = np.random.default_rng(seed)
    k = _along(shape, axis, np.arange(shape[axis], dtype=np.float64))
    return np.angle(np.exp(1j * (2.9 * k + rng.normal(0, 0.1, shape))))


def inputs(shape, axis, seed=0):
    """name -> float64 array of `shape`: the inputs every shape is run on."""
    rng = np.random.default_rng(1000 + seed)
    n = shape[axis]
    out = {"steep_ramp": steep_ramp(shape, axis, seed),
           "random_50": rng.normal(0, 50, shape),
           "random_400": rng.normal(0, 400, shape)}
    alt = np.where(np.arange(n) % 2 == 1, PI, 0.0)
    out["exact_pi"] = _along(shape, axis, alt)
    out["exact_minus_pi"] = -out["exact_pi"]                       # starts at -0.0
    special = np.array([0.0, 1e300, -1e300, 5e-324, -0.0])
    out["special"] = _along(shape, axis, special[np.arange(n) % 5])
    nonfinite = rng.uniform(-PI, PI, shape)
    flat = nonfinite.reshape(-1)
    if flat.size:
        pos = rng.choice(flat.size, size=min(3, flat.size), replace=False)
        for where, v in zip(pos, (np.nan, np.inf, -np.inf)):
            flat[where] = v
    out["nonfinite"] = nonfinite
    return out


def nan_tail_positions(p, axis):
    """Where np.unwrap's result must be NaN: from the first sample whose difference to the one before is not finite (a NaN or
    infinite sample, or the one after it) to the end of its line -- fmod of it is NaN and the running sum carries that -- and at
    a NaN first sample.  (Holds for a finite or NaN discont.)"""
    q = np.moveaxis(p, axis, 0)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(np.diff(q, axis=0))
    tail = np.zeros(q.shape, dtype=bool)
    tail[1:] = np.maximum.accumulate(bad, axis=0)
    tail |= np.isnan(q)
    return np.moveaxis(tail, 0, axis)
