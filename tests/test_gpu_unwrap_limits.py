"""GPU: iir_unwrap_kernel at its stated limits -- every tier of its dynamic LDS ((w + 2 R) * 8 bytes, R = rows per band rounded
up to 64: below 48 KiB, the opt-in range up to 64 KiB, the range only gfx950 has, and the maximum of 147 456 bytes at 16384
columns with 1024-row bands), the whole argument domain of its restated fmod, and batches with several bands per map and with
more workgroups than the device holds at once.  Every comparison is bitwise against the plain restatement
tests/_unwrap_ref.py (or the reference's own recorded hash for the map that is too large for it)."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, G)

import _unwrap_probes                               # noqa: E402
import _unwrap_ref                                  # noqa: E402
import make_golden_unwrap                           # noqa: E402

with open(os.path.join(G, "unwrap_cases.json")) as f:
    CASES = json.load(f)["cases"]


@pytest.fixture(scope="module")
def uw():
    import torch
    assert torch.cuda.is_available()
    from simplestereo_amd import unwrapping
    return unwrapping


def _lds_bytes(h, w, cap=1024):
    bands = (h + cap - 1) // cap
    R = ((h + bands - 1) // bands + 63) // 64 * 64
    return (w + 2 * R) * 8


def _ramp(h, w, seed):
    """a noisy wrapped ramp: the unwrapped map grows along the row, so an error anywhere shows in everything after it"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(np.fmod(0.37 * x + 0.21 * y + rng.normal(0, 0.3, (h, w)), 2 * np.pi))


# ---------------------------------------------------------------------------------------------- A1: LDS tiers, width limit
@pytest.mark.parametrize("h,w,rows,lo,hi", [(5, 7000, None, 48 * 1024, 64 * 1024),          # the opt-in range below 64 KiB
                                             (3, 16384, None, 64 * 1024, 160 * 1024),        # few rows, the widest line
                                             (70, 12000, 64, 64 * 1024, 160 * 1024)],        # two bands, hand-off over a wide line
                         ids=["5x7000", "3x16384", "70x12000_rows64"])
def test_lds_tiers_vs_restatement(uw, h, w, rows, lo, hi):
    from simplestereo_amd import _native
    assert lo < _lds_bytes(h, w, rows or 1024) <= hi
    ph = _ramp(h, w, 1000 + h)
    ref = _unwrap_ref.unwrap(ph, 0.8)
    if rows is None:
        assert _unwrap_ref.identical(uw.infiniteImpulseResponse(ph, 0.8), ref)
    else:
        with _native.options(SSAMD_UNWRAP_ROWS=rows):
            assert _unwrap_ref.identical(uw.infiniteImpulseResponse(ph, 0.8), ref)


def test_wide_map_with_special_values_vs_restatement_in_two_bands(uw):
    """golden frame_wide_special (70 x 12000 with NaN / +-inf, recorded from the reference by hash) once more under 64-row
    bands and against the restatement in full"""
    from simplestereo_amd import _native
    c = CASES["frame_wide_special"]
    ph = make_golden_unwrap.phase_input(c["recipe"])
    assert make_golden_unwrap.sha(ph) == c["input_sha256"]
    ref = _unwrap_ref.unwrap(ph, c["tau"])
    assert make_golden_unwrap.sha_canonical_nan(ref) == c["output_sha256_canonical_nan"]
    with _native.options(SSAMD_UNWRAP_ROWS=64):
        assert _unwrap_ref.identical(uw.infiniteImpulseResponse(ph, c["tau"]), ref)
    assert _unwrap_ref.identical(uw.infiniteImpulseResponse(ph, c["tau"]), ref)


def test_grant_sequence_small_max_small_70k_max(uw):
    """the LDS grant is cached per device and kernel: a smaller request after a larger one must still launch, a larger one
    must be granted again.  small -> maximum (147 456 B) -> small -> 70 KiB -> maximum in one process."""
    c = CASES["frame_wide16384"]
    assert (c["recipe"]["h"], c["recipe"]["w"]) == (1024, 16384) and _lds_bytes(1024, 16384) == 147456
    big = make_golden_unwrap.phase_input(c["recipe"])
    assert make_golden_unwrap.sha(big) == c["input_sha256"]
    small = _ramp(9, 40, 1)
    small_ref = _unwrap_ref.unwrap(small, 0.8)
    mid = _ramp(2, 8800, 2)                                    # (8800 + 128) * 8 = 71 424 B
    assert 69 * 1024 < _lds_bytes(2, 8800) < 71 * 1024
    mid_ref = _unwrap_ref.unwrap(mid, 0.8)

    def run_big():
        out = uw.infiniteImpulseResponse(big, c["tau"])
        assert not np.isnan(out).any() and make_golden_unwrap.sha(out) == c["output_sha256"]

    assert _unwrap_ref.identical(uw.infiniteImpulseResponse(small, 0.8), small_ref)
    run_big()
    assert _unwrap_ref.identical(uw.infiniteImpulseResponse(small, 0.8), small_ref)
    assert _unwrap_ref.identical(uw.infiniteImpulseResponse(mid, 0.8), mid_ref)
    run_big()


def test_16384_columns_accepted_16385_refused(uw):
    """the documented width limit through both C entry points and both Python functions; the refusal is a host-side
    argument check (code -5, SSAMD_ELIMIT) that a Python caller sees as NativeError with the message below"""
    import torch
    from simplestereo_amd import _native
    lib = _native.lib()
    ok = _ramp(2, 16384, 3)
    ref = _unwrap_ref.unwrap(ok, 1.0)
    bad = np.zeros((2, 16385))
    msg = "phase maps wider than 16384 columns are not supported (width 16385)"
    # C ABI, host buffers
    out = np.empty_like(ok)
    assert lib.ssamd_iir_unwrap(ok.ctypes.data, 1, 2, 16384, 1.0, out.ctypes.data, -1) == 0
    assert _unwrap_ref.identical(out, ref)
    ob = np.empty_like(bad)
    assert lib.ssamd_iir_unwrap(bad.ctypes.data, 1, 2, 16385, 1.0, ob.ctypes.data, -1) == -5
    assert lib.ssamd_last_error().decode() == msg
    # C ABI, device buffers
    t, tb = torch.from_numpy(ok).cuda(), torch.from_numpy(bad).cuda()
    o, obd = torch.empty_like(t), torch.empty_like(tb)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.ssamd_iir_unwrap_device(t.data_ptr(), 1, 2, 16384, 1.0, o.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert _unwrap_ref.identical(o.cpu().numpy(), ref)
    assert lib.ssamd_iir_unwrap_device(tb.data_ptr(), 1, 2, 16385, 1.0, obd.data_ptr(), stream) == -5
    assert lib.ssamd_last_error().decode() == msg
    # Python, host and device, single and batch
    assert _unwrap_ref.identical(uw.infiniteImpulseResponse(ok, 1.0), ref)
    assert _unwrap_ref.identical(uw.infiniteImpulseResponse(t, 1.0).cpu().numpy(), ref)
    assert _unwrap_ref.identical(uw.infiniteImpulseResponseBatch(ok[None], 1.0)[0], ref)
    assert _unwrap_ref.identical(uw.infiniteImpulseResponseBatch(t[None], 1.0)[0].cpu().numpy(), ref)
    for call, arg in ((uw.infiniteImpulseResponse, bad), (uw.infiniteImpulseResponse, tb),
                      (uw.infiniteImpulseResponseBatch, bad[None]), (uw.infiniteImpulseResponseBatch, tb[None])):
        with pytest.raises(_native.NativeError) as e:
            call(arg, 1.0)
        assert type(e.value) is _native.NativeError and e.value.code == -5 and e.value.message == msg


# ---------------------------------------------------------------------------------------------- A2: the argument domain of W
@pytest.fixture(scope="module")
def probe_values():
    return _unwrap_probes.probes()


@pytest.mark.parametrize("tau", [1.0, 0.7])
def test_fmod_domain_through_the_batch_call(uw, probe_values, tau):
    """about 2 * 10^5 maps [[0, a]]: multiples of 2 pi and odd multiples of pi +- 0..2 ulps up to 2^38, the switch to the
    library fmod at 2^40, every exponent up to 2^1023, zero and denormals, random exponents.  The whole output is compared
    bitwise with the restatement (math.fmod is exact; a quotient off by one is an output off by 2 pi).

    Census of the branches of unwrap_fmod_2pi over every fmod argument of these maps in the host-side model
    (tests/_unwrap_probes.py), tau = 1 / tau = 0.7, of 1 469 678 arguments each:
        library fmod (|x| >= 2^40, non-finite)   161 627 / 161 613
        x >= 0, k right at once                  905 539 / 920 619
        x >= 0, r < 0  -> k - 1                   28 759 /  19 606
        x >= 0, r >= m -> k + 1                        0 /       0   (unreachable for every double: see _unwrap_probes.DEAD)
        x <  0, k right at once                  344 988 / 348 230
        x <  0, r > 0  -> k + 1                   28 765 /  19 610
        x <  0, r <= -m -> k - 1                       0 /       0   (unreachable)
    The test recomputes the census and asserts that every reachable branch is taken.

    What this can and cannot see through W: a correction in the WRONG direction (or a quotient off by one anywhere else)
    moves the output by 2 pi and fails here.  Leaving a correction OUT altogether is invisible in W, provably: the
    estimate is one too large only when x is within rounding of a multiple of m, so r = x - k m is a tiny negative multiple
    of 2^-50 (x >= m and k m are), and W's `r + pi` for r < 0 is then exact and equals `(r + m) - pi`, the value with the
    corrected quotient, bit for bit.  The corrections matter for fmod's own contract (remainder with the sign of x), which
    tests/test_unwrap_cpu.py holds the modelled algorithm to against math.fmod."""
    maps = _unwrap_probes.pair_maps(probe_values)
    ref, args = _unwrap_probes.fmod_arguments(maps, tau)
    census = _unwrap_probes.branch_census(args)
    print("tau", tau, "maps", len(maps), "census", census)
    for b in _unwrap_probes.BRANCHES:
        if b in _unwrap_probes.DEAD:
            assert census[b] == 0, (b, census)
        else:
            assert census[b] >= 100, (b, census)
    got = uw.infiniteImpulseResponseBatch(maps, tau)
    assert got.shape == maps.shape
    same = (np.isnan(got) == np.isnan(ref)) & ((got.view(np.uint64) == ref.view(np.uint64)) | np.isnan(ref))
    bad = np.argwhere(~same.reshape(len(maps), -1).all(1)).ravel()
    assert bad.size == 0, "%d maps differ, first a = %r: got %r want %r" % (
        bad.size, float(probe_values[bad[0]]), got[bad[0]].tolist(), ref[bad[0]].tolist())
    assert _unwrap_ref.identical(got, ref)


def test_fmod_domain_square_maps(uw, probe_values):
    """2 x 2 maps [[0, a], [b, a]] (b a permutation of the probes): the four-neighbour step of the main pass on the same values"""
    import torch
    maps = _unwrap_probes.square_maps(probe_values[::4])
    ref, args = _unwrap_probes.fmod_arguments(maps, 0.7)
    census = _unwrap_probes.branch_census(args)
    print("square maps", len(maps), "census", census)
    assert all(census[b] >= 100 for b in _unwrap_probes.BRANCHES if b not in _unwrap_probes.DEAD), census
    assert _unwrap_ref.identical(uw.infiniteImpulseResponseBatch(maps, 0.7), ref)
    assert _unwrap_ref.identical(uw.infiniteImpulseResponseBatch(torch.from_numpy(maps).cuda(), 0.7).cpu().numpy(), ref)


# ---------------------------------------------------------------------------------------------- A3: batches
def _batch_with_specials(n, h, w, seed, special_maps):
    rng = np.random.default_rng(seed)
    phs = rng.uniform(-np.pi, np.pi, (n, h, w))
    phs += np.linspace(0, 3, n)[:, None, None] * np.arange(w)[None, None, :] * 0.01          # every map different
    for j, k in enumerate(special_maps):
        # late in the map, so that most of it stays finite (everything after a NaN is NaN)
        phs[k, h - 1, w - 3 - j] = (np.nan, np.inf, -np.inf)[j % 3]
        phs[k, h // 2, w - 2] = (np.inf, -np.inf, np.nan)[j % 3]
    return np.ascontiguousarray(phs)


def _check_batch(uw, phs, tau, special_maps):
    import torch
    n = len(phs)
    host = uw.infiniteImpulseResponseBatch(phs, tau)
    t = torch.from_numpy(phs).cuda()
    dev = uw.infiniteImpulseResponseBatch(t, tau)
    assert host.shape == phs.shape and tuple(dev.shape) == phs.shape
    bits = dev.view(torch.int64)                         # (one kernel, one device: NaNs carry the same bits too)
    assert torch.equal(bits, torch.from_numpy(host).cuda().view(torch.int64))
    for k in range(n):                                   # every map equals its single call
        assert torch.equal(uw.infiniteImpulseResponse(t[k], tau).view(torch.int64), bits[k]), k
    sample = sorted({0, n - 1, n // 2, n // 3, n // 4, n // 5, 1, n - 2} | set(special_maps))
    assert len(sample) >= 8
    for k in sample:
        assert _unwrap_ref.identical(host[k], _unwrap_ref.unwrap(phs[k], tau)), k
    assert all(np.isnan(host[k]).any() and np.isfinite(host[k]).any() for k in special_maps)


def test_batch_with_three_bands_per_map(uw):
    """300 maps of 130 x 33 under 64-row bands: three bands per workgroup, with the line hand-off, in a batch"""
    from simplestereo_amd import _native
    special = [0, 7, 150, 299]
    phs = _batch_with_specials(300, 130, 33, 21, special)
    with _native.options(SSAMD_UNWRAP_ROWS=64):
        _check_batch(uw, phs, 0.8, special)


def test_batch_larger_than_the_device_holds_at_once(uw):
    """Small maps never fill the device (64 threads and 1 KiB of LDS allow thousands of resident workgroups), so the LDS
    limits residency: 320 maps of 3 x 10500 need 83 KiB each, one workgroup per CU and 256 resident on 256 CUs -- the
    rest of the grid starts as earlier workgroups finish"""
    assert _lds_bytes(3, 10500) <= 160 * 1024 < 2 * _lds_bytes(3, 10500)
    special = [0, 255, 256, 319]
    phs = _batch_with_specials(320, 3, 10500, 22, special)
    _check_batch(uw, phs, 0.8, special)
