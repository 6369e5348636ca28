"""What the Python layer hands to libssamd.so for host arrays: entry point, scalar arguments in the order of include/ssamd.h, and
pointers to arrays of the right type and size.  No GPU and no library: ``_native.lib`` is a recorder.  The expected tuples are
written out by hand from the header, not computed by the code under test."""
import ctypes
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PI = float(np.pi)
PTR = object()          # placeholder of a pointer argument in an expected tuple


class Recorder:
    """Stands in for the CDLL: every ``ssamd_*`` attribute records ``(name, args)`` and returns 0.  ``peek[name] = {argument
    index: (dtype, count)}`` copies what such a pointer addresses while the call is running (temporaries die with it)."""

    def __init__(self, peek=None):
        self.calls = []
        self.peeked = []
        self.peek = peek or {}

    def __getattr__(self, name):
        if not name.startswith("ssamd_"):
            raise AttributeError(name)
        if name == "ssamd_last_error":
            return lambda: b""

        def fn(*args):
            self.calls.append((name, args))
            seen = {}
            for i, (dtype, count) in self.peek.get(name, {}).items():
                seen[i] = np.frombuffer((ctypes.c_char * (np.dtype(dtype).itemsize * count)).from_address(args[i]), dtype).copy()
            self.peeked.append(seen)
            return 0
        return fn

    def names(self):
        return [c[0] for c in self.calls]


@pytest.fixture
def rec(monkeypatch):
    from simplestereo_amd import _native
    r = Recorder()
    monkeypatch.setattr(_native, "lib", lambda: r)
    return r


@pytest.fixture(scope="module")
def pair():
    rng = np.random.default_rng(11)
    return rng.integers(0, 256, (12, 16, 3)).astype(np.uint8), rng.integers(0, 256, (12, 16, 3)).astype(np.uint8)


@pytest.fixture(scope="module")
def phase():
    return np.random.default_rng(12).uniform(-3, 3, (6, 8))


def _expect(call, name, want):
    """name, number of arguments, the scalars with their exact Python types; returns the pointer arguments as ints"""
    got_name, args = call
    assert got_name == name
    assert len(args) == len(want), (name, args)
    ptrs = []
    for i, (g, w) in enumerate(zip(args, want)):
        if w is PTR:
            assert type(g) is int and g != 0, (name, i, g)
            ptrs.append(g)
        else:
            assert type(g) is type(w) and g == w, (name, i, g, w)
    return ptrs


def _is_result(ptr, out, dtype, shape):
    assert isinstance(out, np.ndarray) and out.dtype == dtype and out.shape == shape and out.flags.c_contiguous
    assert ptr == out.ctypes.data


ASW = dict(winSize=5, maxDisparity=7, minDisparity=1, gammaC=4, gammaP=9.5, consistent=True)
ASW_SCALARS = (5, 7, 1, 4.0, 9.5, 1)           # winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent
GSW = dict(winSize=5, maxDisparity=7, minDisparity=1, gamma=9, fMax=100, iterations=2, bins=13)
GSW_SCALARS = (5, 7, 1, 9, 100.0, 2, 13)       # winSize, maxDisparity, minDisparity, gamma, fMax, iterations, bins


@pytest.mark.parametrize("kw, entry, counter", [
    (dict(), "ssamd_asw_exact", True),                       # exact="auto" without alternate: the tie-break entry point
    (dict(exact=False), "ssamd_asw", False),
    (dict(alternate=True), "ssamd_asw_alternate", False),
])
def test_asw_host_arrays_one_device(rec, pair, kw, entry, counter):
    import simplestereo_amd as ss
    a, b = pair
    for device, dev in ((None, -1), (2, 2)):
        del rec.calls[:]
        out = ss.passive.StereoASW(device=device, **ASW, **kw).compute(a, b)
        # int ssamd_asw*(img1, img2, height, width, winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent, disparity, device)
        p = _expect(rec.calls[0], entry, (PTR, PTR, 12, 16) + ASW_SCALARS + (PTR, dev))
        assert p[0] == a.ctypes.data and p[1] == b.ctypes.data
        _is_result(p[2], out, np.int16, (12, 16))
        # exact host calls then read the overflow flag of the device they ran on: ssamd_counter(device, name, value)
        assert rec.names() == [entry] + (["ssamd_counter"] if counter else [])
        if counter:
            assert rec.calls[1][1][:2] == (dev, b"exact_overflow")


@pytest.mark.parametrize("kw, entry", [
    (dict(), "ssamd_asw_exact_multi"),
    (dict(exact=False), "ssamd_asw_multi"),
    (dict(alternate=True), "ssamd_asw_alternate_multi"),
])
def test_asw_host_arrays_devices(rec, pair, kw, entry):
    import simplestereo_amd as ss
    a, b = pair
    out = ss.passive.StereoASW(device=2, **ASW, **kw).compute(a, b, devices=[1, 0])
    assert rec.names() == [entry]
    # int ssamd_asw*_multi(img1, img2, height, width, winSize, ..., consistent, disparity, const int *devices, n_devices)
    args = rec.calls[0][1]
    p = _expect((entry, args[:11] + args[12:]), entry, (PTR, PTR, 12, 16) + ASW_SCALARS + (PTR, 2))
    assert p[0] == a.ctypes.data and p[1] == b.ctypes.data
    _is_result(p[2], out, np.int16, (12, 16))
    assert isinstance(args[11], ctypes.Array) and args[11]._type_ is ctypes.c_int and list(args[11]) == [1, 0]


def test_asw_host_arrays_not_contiguous(monkeypatch, pair):
    """a strided view is copied: the library sees 12 * 16 * 3 contiguous bytes with the view's contents"""
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    r = Recorder({"ssamd_asw": {0: (np.uint8, 12 * 16 * 3), 1: (np.uint8, 12 * 16 * 3)}})
    monkeypatch.setattr(_native, "lib", lambda: r)
    rng = np.random.default_rng(13)
    wide = rng.integers(0, 256, (12, 32, 3)).astype(np.uint8)
    a, b = wide[:, ::2], pair[1]
    ss.passive.StereoASW(exact=False, **ASW).compute(a, b)
    p = _expect(r.calls[0], "ssamd_asw", (PTR, PTR, 12, 16) + ASW_SCALARS + (PTR, -1))
    assert p[0] != a.ctypes.data and p[1] == b.ctypes.data
    assert np.array_equal(r.peeked[0][0].reshape(12, 16, 3), a) and np.array_equal(r.peeked[0][1].reshape(12, 16, 3), b)


def test_gsw_host_arrays(rec, pair):
    import simplestereo_amd as ss
    a, b = pair
    out = ss.passive.StereoGSW(device=3, **GSW).compute(a, b)
    assert rec.names() == ["ssamd_gsw"]
    # int ssamd_gsw(img1, img2, height, width, winSize, maxDisparity, minDisparity, gamma, fMax, iterations, bins, disparity, device)
    p = _expect(rec.calls[0], "ssamd_gsw", (PTR, PTR, 12, 16) + GSW_SCALARS + (PTR, 3))
    assert p[0] == a.ctypes.data and p[1] == b.ctypes.data
    _is_result(p[2], out, np.int16, (12, 16))
    del rec.calls[:]
    out = ss.passive.StereoGSW(**GSW).compute(a, b, devices=[1, 0])
    assert rec.names() == ["ssamd_gsw_multi"]
    args = rec.calls[0][1]
    p = _expect(("ssamd_gsw_multi", args[:12] + args[13:]), "ssamd_gsw_multi", (PTR, PTR, 12, 16) + GSW_SCALARS + (PTR, 2))
    assert p[0] == a.ctypes.data and p[1] == b.ctypes.data
    _is_result(p[2], out, np.int16, (12, 16))
    assert isinstance(args[12], ctypes.Array) and args[12]._type_ is ctypes.c_int and list(args[12]) == [1, 0]


def test_iir_unwrap_host_arrays(rec, phase):
    import simplestereo_amd as ss
    out = ss.unwrapping.infiniteImpulseResponse(phase, tau=0.75)
    assert rec.names() == ["ssamd_iir_unwrap"]
    # int ssamd_iir_unwrap(const double *phase, int n, int h, int w, double tau, double *out, int device)
    p = _expect(rec.calls[0], "ssamd_iir_unwrap", (PTR, 1, 6, 8, 0.75, PTR, -1))
    assert p[0] == phase.ctypes.data
    _is_result(p[1], out, np.float64, (6, 8))
    del rec.calls[:]
    batch = np.stack([phase, -phase])
    out = ss.unwrapping.infiniteImpulseResponseBatch(batch, tau=1)          # an int tau arrives as a double
    assert rec.names() == ["ssamd_iir_unwrap"]
    p = _expect(rec.calls[0], "ssamd_iir_unwrap", (PTR, 2, 6, 8, 1.0, PTR, -1))
    assert p[0] == batch.ctypes.data
    _is_result(p[1], out, np.float64, (2, 6, 8))


def test_np_unwrap_host_arrays(monkeypatch, rec, phase):
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    p3 = np.random.default_rng(14).uniform(-9, 9, (2, 3, 4))
    out = ss.unwrapping.unwrap(p3, axis=1)
    assert rec.names() == ["ssamd_np_unwrap"]
    # int ssamd_np_unwrap(const double *p, long long outer, long long len, long long inner, double discont, double period, double *out, int device)
    p = _expect(rec.calls[0], "ssamd_np_unwrap", (PTR, 2, 3, 4, PI, 2 * PI, PTR, -1))
    assert p[0] == p3.ctypes.data
    _is_result(p[1], out, np.float64, (2, 3, 4))
    del rec.calls[:]
    out = ss.unwrapping.unwrap(p3, 1.5, 0, period=4)
    p = _expect(rec.calls[0], "ssamd_np_unwrap", (PTR, 1, 2, 12, 1.5, 4.0, PTR, -1))
    assert p[0] == p3.ctypes.data
    _is_result(p[1], out, np.float64, (2, 3, 4))
    del rec.calls[:]
    out = ss.unwrapping.unwrap2D(phase)
    assert rec.names() == ["ssamd_np_unwrap_xy"]
    # int ssamd_np_unwrap_xy(const double *p, int n, int h, int w, double *out, int device)
    p = _expect(rec.calls[0], "ssamd_np_unwrap_xy", (PTR, 1, 6, 8, PTR, -1))
    assert p[0] == phase.ctypes.data
    _is_result(p[1], out, np.float64, (6, 8))
    # a transposed view is copied first: 4 * 3 * 2 contiguous doubles with the view's contents
    r = Recorder({"ssamd_np_unwrap": {0: (np.float64, 24)}})
    monkeypatch.setattr(_native, "lib", lambda: r)
    view = p3.transpose(2, 1, 0)
    out = ss.unwrapping.unwrap(view, axis=-1)
    p = _expect(r.calls[0], "ssamd_np_unwrap", (PTR, 12, 2, 1, PI, 2 * PI, PTR, -1))
    assert np.array_equal(r.peeked[0][0].reshape(4, 3, 2), view)
    _is_result(p[1], out, np.float64, (4, 3, 2))


def test_empty_inputs_make_no_native_call(rec):
    import simplestereo_amd as ss
    assert ss.unwrapping.infiniteImpulseResponse(np.zeros((0, 8))).shape == (0, 8)
    assert ss.unwrapping.unwrap(np.zeros((2, 0, 4)), axis=1).shape == (2, 0, 4)
    assert ss.unwrapping.unwrap2D(np.zeros((3, 6, 0))).shape == (3, 6, 0)
    assert ss.active.ftpPhase(np.zeros((0, 16), np.uint8), np.zeros((0, 16, 3), np.uint8), 0.1).shape == (0, 16)
    assert rec.calls == []


@pytest.mark.parametrize("unwrap, tau, uw, t", [(None, 0.5, 0, 1.0), ("iir", 0.5, 1, 0.5), ("numpy", 0.5, 2, 1.0)])
def test_ftp_phase_host_arrays(monkeypatch, pair, unwrap, tau, uw, t):
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    r = Recorder({"ssamd_ftp_phase": {6: (np.float64, 12), 7: (np.float64, 12)}})
    monkeypatch.setattr(_native, "lib", lambda: r)
    obj = pair[0]
    ref = np.ascontiguousarray(pair[1][:, :, 0])
    fc = np.linspace(0.1, 0.2, 12)
    out = ss.active.ftpPhase(obj, ref, fc, radius_factor=0.25, unwrap=unwrap, tau=tau)
    assert r.names() == ["ssamd_ftp_phase"]
    # int ssamd_ftp_phase(img_obj, int ch_obj, img_ref, int ch_ref, int h, int w, const double *fmin, const double *fmax,
    #                     int unwrap, double tau, double *out, int device)
    p = _expect(r.calls[0], "ssamd_ftp_phase", (PTR, 3, PTR, 1, 12, 16, PTR, PTR, uw, t, PTR, -1))
    assert p[0] == obj.ctypes.data and p[1] == ref.ctypes.data
    assert np.array_equal(r.peeked[0][6], fc - 0.25 * fc) and np.array_equal(r.peeked[0][7], fc + 0.25 * fc)
    _is_result(p[4], out, np.float64, (12, 16))


def test_ftp_cloud_host_arrays(monkeypatch, phase):
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    r = Recorder({"ssamd_ftp_cloud": {5: (np.float64, 68)}})          # SSAMD_FTP_CLOUD_NGEOM
    monkeypatch.setattr(_native, "lib", lambda: r)
    rig = ss.StereoRig.fromFile(os.path.join(GOLDEN, "rig_example1_rig.json"))
    G = ss.active.ftpGeometry(rig, 500.0, 12.0, roi=(3, 2, 8, 6))
    out = ss.active.ftpCloud(phase, G, k=2)
    assert r.names() == ["ssamd_ftp_cloud"]
    # int ssamd_ftp_cloud(const double *phase, int h, int w, int x0, int y0, const double *geom, double k, double *out, int device)
    p = _expect(r.calls[0], "ssamd_ftp_cloud", (PTR, 6, 8, 3, 2, PTR, 2.0, PTR, -1))
    assert p[0] == phase.ctypes.data and p[1] == G.geom.ctypes.data
    assert G.geom.dtype == np.float64 and G.geom.shape == (68,) and np.array_equal(r.peeked[0][5], G.geom)
    _is_result(p[2], out, np.float64, (6, 8, 3))
    del r.calls[:]
    out = ss.active.ftpCloud(phase, rig, 500.0, 12.0, roi=(3, 2, 8, 6))      # the geometry packed inside the call, k = 0
    p = _expect(r.calls[0], "ssamd_ftp_cloud", (PTR, 6, 8, 3, 2, PTR, 0.0, PTR, -1))
    assert np.array_equal(r.peeked[1][5], G.geom)
