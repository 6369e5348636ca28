"""GPU: ss.unwrapping (iir_unwrap_kernel, the wavefront restatement of the reference's _unwrapping.infiniteImpulseResponse)
against the reference's own outputs (golden/unwrap_cases.*, both full frames by sha256) and against the plain restatement
tests/_unwrap_ref.py on random maps.  Every comparison is bitwise (uint64 views; NaN wherever the restatement has NaN)."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, G)

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


def _bitwise(a, b):
    return _unwrap_ref.identical(a, b)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["whole"]))
def test_small_goldens(uw, name):
    z = np.load(os.path.join(G, "unwrap_cases.npz"))
    out = uw.infiniteImpulseResponse(z[name + "__in"], CASES[name]["tau"])
    assert out.dtype == np.float64 and _bitwise(out, z[name + "__out"])
    if not np.isnan(out).any():
        assert make_golden_unwrap.sha(out) == CASES[name]["output_sha256"]


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if not c["whole"]))
def test_full_frame_goldens(uw, name):
    c = CASES[name]
    ph = make_golden_unwrap.phase_input(c["recipe"])
    assert make_golden_unwrap.sha(ph) == c["input_sha256"]
    out = uw.infiniteImpulseResponse(ph, c["tau"])
    if "output_sha256_canonical_nan" in c:         # a map with NaN: sign and payload of a NaN are the processor's
        assert make_golden_unwrap.sha_canonical_nan(out) == c["output_sha256_canonical_nan"]
    else:
        assert not np.isnan(out).any() and make_golden_unwrap.sha(out) == c["output_sha256"]


def _random_map(rng, h, w, special):
    kind = rng.integers(0, 3)
    if kind == 0:
        ph = rng.uniform(-np.pi, np.pi, (h, w))
    elif kind == 1:
        y, x = np.mgrid[0:h, 0:w]
        ph = np.fmod(rng.uniform(-2, 2) * x + rng.uniform(-2, 2) * y + rng.normal(0, 0.3, (h, w)), 2 * np.pi)
    else:
        ph = rng.uniform(-1e4, 1e4, (h, w))
    if special:
        m = rng.random((h, w))
        ph[m < 0.03] = np.nan
        ph[(m >= 0.03) & (m < 0.05)] = np.inf
        ph[(m >= 0.05) & (m < 0.07)] = -np.inf
    return np.ascontiguousarray(ph)


def _random_cases():
    rng = np.random.default_rng(2024)
    cases = []
    for i in range(40):
        h = int(rng.choice([1, 2, 3, 5, 17, 63, 64, 65, 66, 129, 130])) if i % 3 else int(rng.integers(1, 90))
        w = int(rng.integers(1, 120 if h < 70 else 20))
        tau = float(rng.choice([0.0, 0.25, 0.5, 0.8, 1.0, rng.random(), np.nan]))
        cases.append((i, h, w, tau, i % 5 == 4, int(rng.integers(0, 2 ** 31))))
    return cases


@pytest.mark.parametrize("case", _random_cases(), ids=lambda c: "r%d_%dx%d" % (c[0], c[1], c[2]))
def test_random_vs_restatement(uw, case):
    from simplestereo_amd import _native
    i, h, w, tau, special, seed = case
    ph = _random_map(np.random.default_rng(seed), h, w, special)
    ref = _unwrap_ref.unwrap(ph, tau)
    assert _bitwise(uw.infiniteImpulseResponse(ph, tau), ref)
    # bands of 64 rows: the hand-off from one band's last row to the next band's first row
    with _native.options(SSAMD_UNWRAP_ROWS=64):
        assert _bitwise(uw.infiniteImpulseResponse(ph, tau), ref)


def test_strided_input(uw):
    rng = np.random.default_rng(5)
    big = rng.uniform(-np.pi, np.pi, (80, 150))
    for view in (big[::2, ::3], big[:, 10:77], big.T[:60, :50], np.asfortranarray(big[:30, :40])):
        assert not view.flags.c_contiguous
        assert _bitwise(uw.infiniteImpulseResponse(view, 0.8), _unwrap_ref.unwrap(np.ascontiguousarray(view), 0.8))


def test_device_tensor_on_a_side_stream(uw):
    import torch
    rng = np.random.default_rng(6)
    ph = rng.uniform(-np.pi, np.pi, (70, 90))
    ref = _unwrap_ref.unwrap(ph, 0.5)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t = torch.from_numpy(ph).cuda()
        out = uw.infiniteImpulseResponse(t, 0.5)
        assert out.is_cuda and out.device == t.device and out.dtype == torch.float64 and tuple(out.shape) == (70, 90)
        res = out.cpu().numpy()
    s.synchronize()
    assert _bitwise(res, ref)
    # a non-contiguous device tensor is made contiguous; a non-float64 one is refused
    tt = torch.from_numpy(np.ascontiguousarray(ph.T)).cuda().t()
    assert _bitwise(uw.infiniteImpulseResponse(tt, 0.5).cpu().numpy(), ref)
    with pytest.raises(TypeError):
        uw.infiniteImpulseResponse(t.float(), 0.5)
    with pytest.raises(ValueError, match="Wrong phase dimensions!"):
        uw.infiniteImpulseResponse(t[0], 0.5)


@pytest.mark.parametrize("n", [1, 3, 64])
def test_batch_equals_single_calls(uw, n):
    import torch
    rng = np.random.default_rng(100 + n)
    phs = np.ascontiguousarray(rng.uniform(-np.pi, np.pi, (n, 37, 53)))
    singles = np.stack([uw.infiniteImpulseResponse(phs[k], 0.8) for k in range(n)])
    host = uw.infiniteImpulseResponseBatch(phs, 0.8)
    assert host.shape == (n, 37, 53) and np.array_equal(host.view(np.uint64), singles.view(np.uint64))
    dev = uw.infiniteImpulseResponseBatch(torch.from_numpy(phs).cuda(), 0.8)
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), singles.view(np.uint64))
    assert _bitwise(singles[0], _unwrap_ref.unwrap(phs[0], 0.8))


def test_repeated_calls_identical(uw):
    rng = np.random.default_rng(7)
    ph = rng.uniform(-np.pi, np.pi, (300, 257))
    a = uw.infiniteImpulseResponse(ph, 1)
    b = uw.infiniteImpulseResponse(ph, 1)
    assert a is not b and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_accepted_probes(uw):
    """int / bool tau accepted; NaN tau gives a NaN map (golden/unwrap_errors.json)."""
    ph = np.arange(6.0).reshape(2, 3)
    assert _bitwise(uw.infiniteImpulseResponse(ph, 1), _unwrap_ref.unwrap(ph, 1.0))
    assert _bitwise(uw.infiniteImpulseResponse(ph, True), _unwrap_ref.unwrap(ph, 1.0))
    assert _bitwise(uw.infiniteImpulseResponse(ph, 0), _unwrap_ref.unwrap(ph, 0.0))
    assert np.isnan(uw.infiniteImpulseResponse(ph, float("nan"))).all()


def test_profile_slot_counts_launches(uw):
    from simplestereo_amd import _native
    lib = _native.lib()
    lib.ssamd_profile_enable(1)
    try:
        lib.ssamd_profile_reset()
        uw.infiniteImpulseResponse(np.zeros((10, 12)), 0.5)
        uw.infiniteImpulseResponseBatch(np.zeros((4, 10, 12)), 0.5)
        ms, n = _native.profile_read()
        assert n[_native.K_UNWRAP] == 2 and ms[_native.K_UNWRAP] > 0
        assert sum(n) == 2
    finally:
        lib.ssamd_profile_enable(0)
        lib.ssamd_profile_reset()
