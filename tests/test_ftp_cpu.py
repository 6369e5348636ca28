"""CPU: the host side of ss.active.ftpPhase -- the band planner (csrc/ftp_plan.h through ssamd_ftp_band) against numpy's own
mask, the Python-level checks (every exception is raised before any native call), and the integrity of the fixture
tests/golden/ftp_cases.* that tests/test_gpu_ftp.py measures the kernel against."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, G)

import _ftp_ref                                      # noqa: E402
import make_golden_ftp                               # noqa: E402

WIDTHS = [1, 2, 3, 16, 49, 63, 64, 97, 257, 1000, 4096]


def _planner(w, fmin, fmax):
    from simplestereo_amd import _native
    fmin = np.ascontiguousarray(fmin, dtype=np.float64)
    fmax = np.ascontiguousarray(fmax, dtype=np.float64)
    h = fmin.shape[0]
    lo = np.full(h, 12345, dtype=np.int32)
    hi = np.full(h, 12345, dtype=np.int32)
    _native.check(_native.lib().ssamd_ftp_band(w, h, fmin.ctypes.data, fmax.ctypes.data, lo.ctypes.data, hi.ctypes.data))
    return lo.astype(np.int64), hi.astype(np.int64)


def _agree(w, fmin, fmax):
    lo, hi = _planner(w, fmin, fmax)
    rlo, rhi = _ftp_ref.band_ranges(w, fmin, fmax)             # asserts that numpy's kept bins are contiguous
    bad = np.flatnonzero((lo != rlo) | (hi != rhi))
    assert bad.size == 0, (w, fmin[bad[:3]], fmax[bad[:3]], lo[bad[:3]], hi[bad[:3]], rlo[bad[:3]], rhi[bad[:3]])


def _around(v):
    return [np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)]


@pytest.mark.parametrize("w", WIDTHS)
def test_band_bounds_on_and_next_to_every_bin(w):
    """fmin and fmax exactly a bin's frequency and one ulp either side of it, for every bin (a sample of 64 at 4096)."""
    freqs = np.fft.fftfreq(w)
    pick = np.arange(w) if w <= 1000 else np.unique(np.concatenate([np.arange(0, w, 67), [0, 1, w // 2 - 1, w // 2, w // 2 + 1, w - 1]]))
    edges = np.array([e for k in pick for e in _around(freqs[k])])
    _agree(w, edges, np.full_like(edges, np.inf))                       # the lower bound alone
    _agree(w, np.full_like(edges, -np.inf), edges)                      # the upper bound alone
    rng = np.random.default_rng(w)
    other = rng.choice(edges, edges.size)
    _agree(w, np.minimum(edges, other), np.maximum(edges, other))
    _agree(w, np.maximum(edges, other), np.minimum(edges, other))       # fmin above fmax: empty unless they meet on a bin


def test_width_49_distinguishes_fftfreq_from_a_division():
    """k * (1.0 / 49) and k / 49.0 differ for some k: a planner that divides puts those band edges on the wrong bin."""
    w = 49
    s = _ftp_ref.signed_bins(w)
    freqs = np.fft.fftfreq(w)
    assert np.array_equal(freqs, s * (1.0 / w))
    differ = np.flatnonzero(freqs != s / float(w))
    assert differ.size > 0
    for k in differ:
        divided = s[k] / float(w)
        for e in (freqs[k], divided):
            _agree(w, np.array([e]), np.array([np.inf]))
            _agree(w, np.array([-np.inf]), np.array([e]))
        # between the two values the bin is on one side for fftfreq and on the other for a division
        lo, hi = _planner(w, np.array([max(freqs[k], divided)]), np.array([np.inf]))
        assert (lo[0] == s[k]) == (freqs[k] > divided)


@pytest.mark.parametrize("w", WIDTHS)
def test_band_special_bounds(w):
    nan, inf = np.nan, np.inf
    nyq = 0.5
    fmin = np.array([-0.3, -0.75, 0.1, 0.1, nan, 0.1, nan, -inf, inf, 0.2, -inf, inf, 0.3, 0.26, 0.0, -0.0])
    fmax = np.array([0.2, 0.75, nyq, 0.9, 0.2, nan, nan, inf, inf, -inf, -inf, -inf, 0.1, 0.26000001, 0.0, -0.0])
    _agree(w, fmin, fmax)
    lo, hi = _planner(w, fmin, fmax)
    assert lo[6] == -(w // 2) and hi[6] == (w - 1) // 2                  # NaN on both sides masks nothing
    assert lo[7] == -(w // 2) and hi[7] == (w - 1) // 2
    for k in (8, 9, 10, 11, 12):
        assert (lo[k], hi[k]) == (0, -1)                                # the one spelling of an empty band
    assert (lo[14], hi[14]) == (0, 0) and (lo[15], hi[15]) == (0, 0)


@pytest.mark.parametrize("w", WIDTHS)
def test_band_random_bounds(w):
    rng = np.random.default_rng(1000 + w)
    n = 2000
    fc = rng.uniform(-0.1, 0.6, n)
    rf = rng.choice([0.0, 0.01, 0.3, 0.5, 0.9, 1.0, 1.5, 10.0], n)
    fmin, fmax = _ftp_ref.band(fc, rf, n)                               # rf > 1: negative fmin; fmax beyond Nyquist
    snap = rng.random(n) < 0.3                                          # some bounds snapped onto a bin
    fmin[snap] = rng.choice(np.fft.fftfreq(w), int(snap.sum()))
    _agree(w, fmin, fmax)


def test_band_rejects_bad_sizes():
    from simplestereo_amd import _native
    z = np.zeros(1)
    o = np.zeros(1, dtype=np.int32)
    assert _native.lib().ssamd_ftp_band(0, 1, z.ctypes.data, z.ctypes.data, o.ctypes.data, o.ctypes.data) == -1
    assert _native.lib().ssamd_ftp_band(4, 1, None, z.ctypes.data, o.ctypes.data, o.ctypes.data) == -1
    assert _native.lib().ssamd_ftp_band(4, 0, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------- Python-level checks
class _NoNative:
    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were checked" % name)


@pytest.fixture
def active(monkeypatch):
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _NoNative())
    return ss.active


def test_exported():
    import simplestereo_amd as ss
    assert "active" in ss.__all__ and ss.active.ftpPhase.__module__ == "simplestereo_amd.active"
    assert "ftpPhase" in ss.active.__all__
    assert ss.active.MAX_WIDTH == make_golden_ftp.MAX_WIDTH
    header = open(os.path.join(os.path.dirname(HERE), "include", "ssamd.h")).read()
    assert "#define SSAMD_FTP_MAX_W %d" % ss.active.MAX_WIDTH in header
    assert "active.py:675-737" in header and "active.py:675-737" in ss.active.ftpPhase.__doc__
    assert "not ``StereoFTP``" in ss.active.ftpPhase.__doc__


def test_exceptions_before_any_native_call(active):
    g = np.zeros((4, 8), dtype=np.uint8)
    bgr = np.zeros((4, 8, 3), dtype=np.uint8)
    f = active.ftpPhase
    with pytest.raises(TypeError):
        f(g.astype(np.float32), g, 0.1)
    with pytest.raises(TypeError):
        f(g, g.astype(np.int8), 0.1)
    with pytest.raises(TypeError):
        f(g.tolist(), g, 0.1)
    for bad in (np.zeros(8, dtype=np.uint8), np.zeros((4, 8, 3, 1), dtype=np.uint8), np.zeros((4, 8, 1), dtype=np.uint8),
                np.zeros((4, 8, 4), dtype=np.uint8)):
        with pytest.raises(ValueError):
            f(bad, g, 0.1)
        with pytest.raises(ValueError):
            f(g, bad, 0.1)
    with pytest.raises(ValueError):
        f(g, np.zeros((4, 9), dtype=np.uint8), 0.1)
    with pytest.raises(ValueError):
        f(bgr, np.zeros((5, 8), dtype=np.uint8), 0.1)
    for bad_fc in (np.full(3, 0.1), np.full(5, 0.1), np.full((4, 1), 0.1), "0.1", None, [0.1, "x", 0.1, 0.1], 1j):
        with pytest.raises(ValueError):
            f(g, g, bad_fc)
    for bad_rf in ("0.5", None, [0.5], 1j):
        with pytest.raises(ValueError):
            f(g, g, 0.1, radius_factor=bad_rf)
    for bad_unwrap in ("IIR", "none", 1, True, b"iir"):
        with pytest.raises(ValueError):
            f(g, g, 0.1, unwrap=bad_unwrap)
    for bad_tau in (-0.1, 1.5, "1", None):
        with pytest.raises(ValueError):
            f(g, g, 0.1, unwrap="iir", tau=bad_tau)
    wide = np.zeros((1, active.MAX_WIDTH + 1), dtype=np.uint8)
    with pytest.raises(ValueError):
        f(wide, wide, 0.1)


def test_mixed_host_and_device_is_a_type_error(active):
    class FakeTensor:                                  # what _is_device_tensor looks at, without a GPU
        is_cuda = True
        ndim = 2
        shape = (4, 8)
        device = "cuda:0"

        def contiguous(self):
            return self
    FakeTensor.__module__ = "torch"
    import torch
    FakeTensor.dtype = torch.uint8
    g = np.zeros((4, 8), dtype=np.uint8)
    with pytest.raises(TypeError):
        active.ftpPhase(FakeTensor(), g, 0.1)
    with pytest.raises(TypeError):
        active.ftpPhase(g, FakeTensor(), 0.1)
    other = FakeTensor()
    other.device = "cuda:1"
    with pytest.raises(TypeError):
        active.ftpPhase(FakeTensor(), other, 0.1)


def test_empty_images_give_empty_arrays(active):
    for shape in ((0, 8), (4, 0), (0, 0)):
        e = np.zeros(shape, dtype=np.uint8)
        out = active.ftpPhase(e, np.zeros(shape + (3,), dtype=np.uint8), 0.1, unwrap="iir", tau=0.5)
        assert out.shape == shape and out.dtype == np.float64
    out = active.ftpPhase(np.zeros((0, 8), dtype=np.uint8), np.zeros((0, 8), dtype=np.uint8), np.zeros(0))
    assert out.shape == (0, 8)


def test_band_the_python_layer_hands_down(monkeypatch):
    """fmin / fmax reach the library as the reference computes them: radius = radius_factor * fc in fp64, per row."""
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    seen = {}

    class Lib:
        def ssamd_ftp_phase(self, obj, cho, ref, chr_, h, w, fmin, fmax, uw, tau, out, dev):
            seen["fmin"] = np.ctypeslib.as_array(ctypes.cast(fmin, ctypes.POINTER(ctypes.c_double)), (h,)).copy()
            seen["fmax"] = np.ctypeslib.as_array(ctypes.cast(fmax, ctypes.POINTER(ctypes.c_double)), (h,)).copy()
            seen["args"] = (cho, chr_, h, w, uw, tau, dev)
            return 0
    monkeypatch.setattr(_native, "lib", lambda: Lib())
    g = np.zeros((3, 8), dtype=np.uint8)
    fc = np.array([0.1, 0.3, 0.07])
    ss.active.ftpPhase(g, np.zeros((3, 8, 3), dtype=np.uint8), fc, radius_factor=0.7, unwrap="iir", tau=0.8)
    rmin, rmax = _ftp_ref.band(fc, 0.7, 3)
    assert np.array_equal(seen["fmin"], rmin) and np.array_equal(seen["fmax"], rmax)
    assert seen["args"] == (1, 3, 3, 8, 1, 0.8, -1)
    ss.active.ftpPhase(g, g, 0.2)
    assert np.array_equal(seen["fmin"], np.full(3, 0.2 - 0.5 * 0.2)) and seen["args"][4] == 0


# ---------------------------------------------------------------------------------------------- the fixture itself
with open(os.path.join(G, "ftp_cases.json")) as _f:
    META = json.load(_f)


@pytest.fixture(scope="module")
def fixture_arrays():
    z = np.load(os.path.join(G, "ftp_cases.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_covers_the_generator():
    assert sorted(META["cases"]) == sorted(make_golden_ftp.CASES)
    assert META["tol_factor"] == 16.0 and META["tol_floor"] == float(np.pi * 2.0 ** -52) and META["min_ratio"] == 0.01
    for name, c in META["cases"].items():
        assert c["tol"] == META["tol_factor"] * max(c["numpy_err"], META["tol_floor"]), name
        assert c["tol"] < 1e-13, name                  # a fault is off by more than 1e-3


@pytest.mark.parametrize("name", sorted(make_golden_ftp.CASES))
def test_fixture_integrity(fixture_arrays, name):
    c = META["cases"][name]
    obj, ref, fc, truth = (fixture_arrays[name + s] for s in ("__obj", "__ref", "__fc", "__truth"))
    gobj, gref, gfc, grf = make_golden_ftp.make_case(name)
    assert np.array_equal(obj, gobj) and np.array_equal(ref, gref) and np.array_equal(fc, gfc) and grf == c["radius_factor"]
    assert list(truth.shape) == c["shape"] and truth.dtype == np.float64
    assert [1 if a.ndim == 2 else 3 for a in (obj, ref)] == c["channels"]
    # numpy's own arithmetic on the stored inputs is within its recorded error of the stored truth
    err = float(_ftp_ref.wrap_err(_ftp_ref.ftp_phase_numpy(obj, ref, fc, c["radius_factor"]), truth).max())
    assert err <= c["numpy_err"], (err, c["numpy_err"])
    # the conditioning the tolerance rests on, recomputed
    again, ratio = _ftp_ref.truth_longdouble(obj, ref, fc, c["radius_factor"])
    assert ratio.min() >= META["min_ratio"]
    assert float(_ftp_ref.wrap_err(again, truth).max()) <= META["tol_floor"]
    lo, hi = _ftp_ref.band_ranges(truth.shape[1], *_ftp_ref.band(fc, c["radius_factor"], truth.shape[0]))
    assert [int(v) for v in lo] == c["slo"] and [int(v) for v in hi] == c["shi"]
    plo, phi = _planner(truth.shape[1], *_ftp_ref.band(fc, c["radius_factor"], truth.shape[0]))
    assert np.array_equal(plo, lo) and np.array_equal(phi, hi)


def test_fixture_special_cases():
    c = META["cases"]
    assert c["empty_middle_row"]["slo"][1] > c["empty_middle_row"]["shi"][1]
    assert c["empty_middle_row"]["shi"][0] >= c["empty_middle_row"]["slo"][0]
    assert c["w257_all_bins"]["slo"] == [-128, -128] and c["w257_all_bins"]["shi"] == [128, 128]
    assert c["w64_edges_on_bins"]["slo"] == [4] * 4 and c["w64_edges_on_bins"]["shi"] == [12] * 4
    assert c["w2_both_bins"]["slo"] == [-1] and c["w2_both_bins"]["shi"] == [0]
    assert c["max_width"]["shape"][1] == META["max_width"]
