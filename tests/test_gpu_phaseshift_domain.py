"""GPU tier of phaseshift_decode_kernel on its whole input domain and on unstructured input (tests/golden/phaseshift_domain_cases.json,
tests/golden/make_golden_phaseshift_domain.py).

The grid: a = I3 - I1 and b = I0 - I2 are integers in -255 .. 255, so a 511 x 511 stack with one period per axis
(P.domain_stack) puts every one of the 261 121 pairs through the kernel's atan2 and its wrap, once per axis; the truth is the
np.longdouble chain, the tolerance the recorded 16 * max(numpy_err, extent * 2^-52).  The mask is compared with the rule itself,
a^2 + b^2 < 4 m^2 in rationals.  511 x 511 pixels are 256 workgroups with a ragged end, rows of 511 bytes put the four-byte plane
loads at every alignment, and the roi at (1, 3) of a 513-wide frame moves them again.

Noise: seeded uniform stacks of 256 x 1024 pixels meet exact ties kk = n + 1/2 of the heterodyne step, where k hangs on the last
bit of atan2.  Pixels the fp64 restatement flags (|kk - rint(kk)| > 0.5 - BAND at some step) are compared with the set
P.candidates enumerates -- each tied step taken both ways --, every other pixel plainly, all within the recorded tolerance."""
import math

import numpy as np
import pytest

import _phaseshift_ref as P

pytestmark = pytest.mark.gpu
META = P.load_domain()
BITS_PROJ = (1920, 1080)                                    # the extent of the bit-for-bit comparisons
HALF_SQRT17 = math.sqrt(17.0) / 2
MODULATIONS = (None, 0, 5e-324, 0.5, math.sqrt(2.0) / 2, HALF_SQRT17, math.nextafter(HALF_SQRT17, 0.0), math.nextafter(HALF_SQRT17, 9.0), 2.5, 127.5,
               180.3122, 1e200)
# (a, b): theta = pi, the origin, the +2 pi wrap just below 2 pi, the axes, the saturated values, the diagonals
PINNED = [(0, 0), (0, -1), (0, -255), (-1, 255), (-255, 255), (255, 0), (-255, 0), (0, 255)]
PINNED += [(sa * k, sb * k) for k in range(1, 256) for sa in (1, -1) for sb in (1, -1)]


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()                                 # (a copy: the shared arrays are read-only)


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _grid():
    return _once("grid", P.domain_stack)


def _base(ss, extent=BITS_PROJ):
    """The host call on the plain grid, no maps, no roi: what every other form of the same integers must give the bits of"""
    return _once(("base", extent), lambda: ss.active.phaseShiftDecode(_grid(), P.DOMAIN_PERIODS, extent))


def _both_routes(ss, torch, stack, extent, maps=None, **kw):
    """The host call's result, after the device-tensor call has given the same bits"""
    host = ss.active.phaseShiftDecode(stack, P.DOMAIN_PERIODS, extent, maps=maps, **kw)
    dmaps = None if maps is None else tuple(_dev(torch, m) for m in maps)
    dev = ss.active.phaseShiftDecode(_dev(torch, stack), P.DOMAIN_PERIODS, extent, maps=dmaps, **kw)
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and dev.is_cuda and dev.dtype == torch.float64
    assert P.same_bits(_np(dev), host)                                          # host route == device route, bit for bit
    return host


def _where(pair):
    """[(row, col, coordinate)] of the pair (a, b): in the x-set at (a + 255, b + 255), in the y-set at the transposed pixel"""
    a, b = pair
    return [(a + 255, b + 255, 0), (b + 255, a + 255, 1)]


# ------------------------------------------------------------------------------------------------ the grid: truth, range, pinned pairs
@pytest.mark.parametrize("name", sorted(META["grid"], key=lambda n: META["grid"][n]["extent"]))
def test_every_pair_decodes_to_the_long_double_truth_inside_the_extent(ss, torch, name):
    c = META["grid"][name]
    extent = tuple(c["extent"])
    truth = _once(("truth", extent), lambda: P.decode(_grid(), P.DOMAIN_PERIODS, extent, dtype=np.longdouble))
    got = _both_routes(ss, torch, _grid(), extent)
    assert got.shape == (P.DOMAIN_N, P.DOMAIN_N, 2) and not np.isnan(got).any()
    err = np.abs(got.astype(np.longdouble) - truth)
    outside = (got < 0) | (got >= np.array(extent, dtype=np.float64)) | np.signbit(got)
    failures = ["(a, b) = %r on %s: %r, truth %r%s" % (pair, "xy"[v], got[r, q, v], float(truth[r, q, v]), ", outside [0, %d)" % extent[v] if outside[r, q, v] else "")
                for pair in PINNED for r, q, v in _where(pair) if err[r, q, v] > c["tol"] or outside[r, q, v]]
    assert not failures, "%d pinned pairs fail (tolerance %.3e): %s" % (len(failures), c["tol"], "; ".join(failures[:12]))
    worst = np.unravel_index(int(np.argmax(err)), err.shape)
    print("grid %s: worst |p - truth| %.3e at (a, b) = %r (numpy %.3e, tolerance %.3e)"
          % (name, float(err.max()), (int(worst[0]) - 255, int(worst[1]) - 255) if worst[2] == 0 else (int(worst[1]) - 255, int(worst[0]) - 255),
             c["numpy_err"], c["tol"]))
    assert float(err.max()) <= c["tol"]
    assert not outside.any(), "%d results outside [0, extent) or with the sign bit set, the first at %r" % (int(outside.sum()), tuple(np.argwhere(outside)[0]))
    assert got[255, 255, 0] == 0 and got[255, 255, 1] == 0                      # a = b = 0: +0
    if extent[0] == extent[1]:                                                  # a pair decodes alike on both axes
        assert np.array_equal(got[..., 0], got[..., 1].T)


# ------------------------------------------------------------------------------------------------ the same integers by other routes
def test_other_bytes_with_the_same_differences_give_the_same_bits(ss, torch):
    lifted = P.domain_stack(lifted=True)
    assert not np.array_equal(lifted, _grid())
    assert P.same_bits(_both_routes(ss, torch, lifted, BITS_PROJ), _base(ss))


def test_identity_maps_give_the_bits_of_the_call_without_maps(ss, torch):
    yy, xx = np.mgrid[0:P.DOMAIN_N, 0:P.DOMAIN_N].astype(np.float32)
    assert P.same_bits(_both_routes(ss, torch, _grid(), BITS_PROJ, maps=(xx, yy)), _base(ss))


def test_a_roi_at_an_odd_origin_gives_the_bits_of_the_aligned_call(ss, torch):
    x0, y0 = 1, 3
    frame = np.random.default_rng(3).integers(0, 256, (8, 515, 513), dtype=np.uint8)
    frame[:, y0:y0 + P.DOMAIN_N, x0:x0 + P.DOMAIN_N] = _grid()
    assert P.same_bits(_both_routes(ss, torch, frame, BITS_PROJ, roi=(x0, y0, P.DOMAIN_N, P.DOMAIN_N)), _base(ss))
    assert P.same_bits(_both_routes(ss, torch, _grid(), BITS_PROJ), _base(ss))  # the aligned call itself, both routes, again


# ------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("m", MODULATIONS, ids=lambda m: repr(m))
def test_mask_is_the_exact_rule_on_every_pair(ss, torch, m):
    a, b = P.domain_pairs()
    s = a * a + b * b                                                           # of the x-set; the y-set holds (b, a): the same sum
    values, inverse = np.unique(s, return_inverse=True)
    want = np.array([P.masks(v, m) for v in values.tolist()], dtype=bool)[inverse.reshape(s.shape)]
    got = _both_routes(ss, torch, _grid(), BITS_PROJ, min_modulation=m)
    nan = np.isnan(got)
    print("min_modulation %r: %d of %d pixels masked" % (m, int(want.sum()), want.size))
    wrong = np.argwhere(nan[..., 0] != want)
    assert wrong.size == 0, "%d pixels, the first (a, b) = %r" % (len(wrong), (int(wrong[0][0]) - 255, int(wrong[0][1]) - 255))
    assert np.array_equal(nan[..., 1], want)                                    # on both coordinates
    unmasked = np.where(want[..., None], np.nan, _base(ss))
    assert P.same_bits(got, unmasked)                                           # and the other pixels are what they were
    if m in (None, 0):
        assert not want.any()
    elif m == 5e-324:
        assert int(want.sum()) == 1 and want[255, 255]                          # 0 < m masks a = b = 0, and nothing else
    elif m == 1e200:
        assert want.all()


# ------------------------------------------------------------------------------------------------ noise: the heterodyne step, ties included
def _noise(name):
    def make():
        c = META["noise"][name]
        periods = P.NOISE_PERIODS[name]
        stack = P.noise_stack(c["seed"], periods)
        want, tie = P.decode(stack, periods, P.NOISE_PROJ, details=True)
        return stack, want, tie > 0.5 - P.BAND
    return _once(("noise", name), make)


@pytest.mark.parametrize("name", sorted(P.NOISE_PERIODS))
def test_noise_decodes_to_the_restatement_or_across_a_tie_to_its_other_branch(ss, torch, name):
    c = META["noise"][name]
    periods, proj, tol = P.NOISE_PERIODS[name], P.NOISE_PROJ, c["tol"]
    stack, want, flagged = _noise(name)
    assert int(flagged.sum()) == c["flagged"] >= 1
    t = _dev(torch, stack)
    dev = ss.active.phaseShiftDecode(t, periods, proj)
    got = _np(dev)
    assert got.shape == want.shape and not np.isnan(got).any()
    err = np.abs(got - want).max(axis=-1)
    dist, largest = P.distance_to_candidates(got, stack, periods, proj, flagged)
    other = int((err[flagged] > tol).sum())
    print("noise %s: worst |p - restatement| off the ties %.3e (numpy %.3e, tolerance %.3e); %d flagged pixels, %d of them on the other k than numpy, "
          "worst distance to a candidate %.3e (sets of at most %d)" % (name, float(err[~flagged].max()), c["numpy_err"], tol, int(flagged.sum()), other,
                                                                        float(dist.max()), largest))
    assert float(err[~flagged].max()) <= tol                                    # not flagged: plain
    assert float(dist.max()) <= tol                                             # flagged: one member of the enumerated set, per axis
    host =ss.active.phaseShiftDecode(stack, periods, proj)
    assert P.same_bits(host, got)                                               # host route == device route, flagged pixels included
    assert P.same_bits(_np(ss.active.phaseShiftDecode(t, periods, proj)), got)  # a second call: the same bits


@pytest.mark.parametrize("name", sorted(P.NOISE_PERIODS))
def test_noise_mask_is_the_restatements(ss, torch, name):
    periods, proj = P.NOISE_PERIODS[name], P.NOISE_PROJ
    stack = _noise(name)[0]
    want = np.isnan(P.decode(stack, periods, proj, thr2=P.mod_thr2(50)))
    assert min(int(want[..., 0].sum()), int((~want[..., 0]).sum())) >= 100      # no trivial mask
    t = _dev(torch, stack)
    got = _np(ss.active.phaseShiftDecode(t, periods, proj, min_modulation=50))
    assert np.array_equal(np.isnan(got), want)
    plain = _np(ss.active.phaseShiftDecode(t, periods, proj))
    assert P.same_bits(got, np.where(want, np.nan, plain))
    assert P.same_bits(ss.active.phaseShiftDecode(stack, periods, proj, min_modulation=50), got)
