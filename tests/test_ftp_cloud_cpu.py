"""CPU: the host side of ss.active.ftpCloud / ftpFringeOrder / ftpGeometry, the triangulation of the reference's
StereoFTP.getCloud (active.py:776-841) -- the numpy restatement (tests/_ftp_cloud_ref.py) against the extended-precision truth
of tests/golden/ftp_cloud_cases, the packed geometry against the restatement's own, the fringe order against the reference
formula, every exception before any native call, and the C ABI's declarations and argument checks (which need no device)."""
import ctypes
import os

import numpy as np
import pytest

import _ftp_cloud_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1


# ---------------------------------------------------------------------------------------------- the arithmetic contract
@pytest.mark.parametrize("name", R.case_names())
def test_restatement_within_tol_of_the_truth(name):
    c = R.load_case(name)
    err = R.check_cloud(c, R.cloud_from_geometry(c["g"], c["phase"], c["k"], c["roi"][0], c["roi"][1]))
    print("%s: numpy restatement %.3e, tol %.3e" % (name, err, c["tol"]))
    assert err <= c["tol"]
    assert c["tol"] == 16 * max(c["numpy_err"], 2.0 ** -52)


def test_cases_cover_what_they_must():
    names = set(R.case_names())
    shapes = {tuple(R.load_case(n)["shape"]) for n in names if n != "tall_65537x3"}
    assert {(1, 1), (1, 5), (3, 64), (3, 130), (5, 257)} <= shapes
    assert R.load_case("p5x257_roi")["roi"][:2] == [37, 11]
    assert {len(R.load_case(n)["rig"]["distCoeffs2"]) for n in names} >= {0, 4, 5, 8, 12}
    assert R.load_case("k_minus3")["k"] == -3
    ramp = R.load_case("steep_ramp")["phase"]
    assert ramp.max() - ramp.min() > 200
    c = R.load_case("nonfinite")
    (ny, nx), (zy, zx) = c["special"]
    assert np.isnan(c["phase"][ny, nx]) and np.isfinite(c["phase"][zy, zx])
    _, det = R.cloud_from_geometry(c["g"], c["phase"], c["k"], c["roi"][0], c["roi"][1], details=True)
    assert det["disparity"][zy, zx] == 0.0 and np.count_nonzero(det["disparity"] == 0.0) == 1


def test_tolerance_tells_the_mistakes_apart():
    """Four undistortion iterations, or pixel corners for centres, miss the tolerance by orders of magnitude."""
    c = R.load_case("dist_d12")
    x0, y0 = c["roi"][:2]
    four = R.cloud_from_geometry(c["g"], c["phase"], c["k"], x0, y0, iterations=4)
    corner = R.cloud_from_geometry(c["g"], c["phase"], c["k"], x0 - 0.5, y0 - 0.5)
    assert R.rel_err(four, c["truth"]).max() > 1e3 * c["tol"] and R.rel_err(corner, c["truth"]).max() > 1e6 * c["tol"]


# ---------------------------------------------------------------------------------------------- geometry and fringe order
@pytest.mark.parametrize("name", ["p5x257_roi", "dist_d12", "tall_65537x3"])
def test_packed_geometry_is_the_restatements(name):
    import simplestereo_amd as ss
    c = R.load_case(name)
    G = ss.active.ftpGeometry(R.make_rig(ss, c["rig"]), c["z_plane"], c["period"], tuple(c["roi"]))
    assert G.geom.dtype == np.float64 and G.geom.shape == (ss.active.NGEOM,) == (R.NGEOM,)
    here, fp = R.geometry(c["rig"], c["z_plane"], c["period"])            # matrix products and inverses of THIS machine's BLAS
    assert np.array_equal(G.geom, here) and G.roi == tuple(c["roi"]) and G.fp == fp == c["fp"]
    assert np.allclose(here, c["g"], rtol=1e-12, atol=1e-12)             # ... which the generator's agree with to rounding
    whole = ss.active.ftpGeometry(R.make_rig(ss, c["rig"]), c["z_plane"], c["period"])
    assert whole.roi == (0, 0) + tuple(c["rig"]["res1"])


def _half_theta(base, want):
    """theta with base - theta / (2 pi) == want exactly"""
    lo = (base - want) * (2 * np.pi)
    for _ in range(2000):
        lo = np.nextafter(lo, -np.inf)
    for _ in range(4000):
        if base - lo / (2 * np.pi) == want:
            return lo
        lo = np.nextafter(lo, np.inf)
    raise AssertionError("no theta lands on %r" % want)


def test_fringe_order_equals_the_reference_formula(monkeypatch):
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _NoNative())
    c = R.load_case("p5x257_roi")
    rig, roi = R.make_rig(ss, c["rig"]), tuple(c["roi"])
    x0, y0 = roi[:2]
    G = ss.active.FtpGeometry(np.array(c["g"]), roi, c["fp"])            # the generator's geometry, bit for bit
    stripe = np.array([[100, 0], [101, 1], [101, 2], [102, 3], [103, 4]])
    for peak in (640.0, 611.3, 700.25):
        for shift in (0.0, 2 * np.pi * 5, -2 * np.pi * 3):
            phase = c["phase"] + shift
            want = R.fringe_order(c["g"], c["fp"], phase, stripe, peak, x0, y0)
            assert ss.active.ftpFringeOrder(phase, stripe, G, stripeCentralPeak=peak) == want
            assert want == np.round(want)
    k0 = R.fringe_order(c["g"], c["fp"], c["phase"], stripe, 640.0, x0, y0)
    assert R.fringe_order(c["g"], c["fp"], c["phase"] + 2 * np.pi * 5, stripe, 640.0, x0, y0) == k0 - 5
    # from the rig: this machine's geometry, the same formula
    here = R.geometry(c["rig"], c["z_plane"], c["period"])[0]
    assert ss.active.ftpFringeOrder(c["phase"], stripe, rig, c["z_plane"], c["period"], 640.0, roi) == \
        R.fringe_order(here, c["fp"], c["phase"], stripe, 640.0, x0, y0)
    # a mean that lands on .5 is rounded DOWN: ceil(k - 0.5)
    one = np.array([[100, 2]])
    u_A = R.project_points(c["g"], (100 + x0) + 0.5, (2 + y0) + 0.5)[0]
    peak = float(u_A) + 3.1 * c["period"]
    base = (peak - u_A) * c["fp"]
    phase = np.array(c["phase"])
    for want_mean, k in ((2.5, 2.0), (-1.5, -2.0), (3.5, 3.0)):
        phase[2, 100] = _half_theta(base, want_mean)
        assert base - phase[2, 100] / (2 * np.pi) == want_mean
        assert R.fringe_order(c["g"], c["fp"], phase, one, peak, x0, y0) == k
        assert ss.active.ftpFringeOrder(phase, one, G, stripeCentralPeak=peak) == k
        assert isinstance(ss.active.ftpFringeOrder(phase, one, G, stripeCentralPeak=peak), float)


# ---------------------------------------------------------------------------------------------- Python-level checks
class _NoNative:
    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were checked" % name)


@pytest.fixture
def ss_no_native(monkeypatch):
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _NoNative())
    return ss


def _rig(ss, **changes):
    p = dict(R.rig_params(res1=(64, 48)))
    p.update(changes)
    return R.make_rig(ss, p)


def test_exceptions_before_any_native_call(ss_no_native):
    ss = ss_no_native
    cloud, order, geometry = ss.active.ftpCloud, ss.active.ftpFringeOrder, ss.active.ftpGeometry
    rig = _rig(ss)
    p = np.zeros((48, 64))
    stripe = np.array([[3, 4]])
    # the phase: type, dtype, dimensions, agreement with the roi
    for bad in (p.tolist(), None, 1.0):
        with pytest.raises(TypeError):
            cloud(bad, rig, 1000.0, 12.0)
        with pytest.raises(TypeError):
            order(bad, stripe, rig, 1000.0, 12.0, 640.0)
    for dtype in (np.float32, np.int64, np.complex128):
        with pytest.raises(TypeError):
            cloud(p.astype(dtype), rig, 1000.0, 12.0)
    for bad in (np.zeros(64), np.zeros((1, 48, 64)), np.zeros(())):
        with pytest.raises(ValueError):
            cloud(bad, rig, 1000.0, 12.0)
    for bad in (np.zeros((64, 48)), np.zeros((47, 64)), np.zeros((48, 63))):
        with pytest.raises(ValueError):
            cloud(bad, rig, 1000.0, 12.0)
    with pytest.raises(ValueError):
        cloud(p, rig, 1000.0, 12.0, roi=(0, 0, 32, 48))
    with pytest.raises(ValueError):
        cloud(np.zeros((8, 16)), rig, 1000.0, 12.0, roi=(0, 0, 8, 16))            # (w, h) swapped
    # the roi
    small = np.zeros((8, 16))
    for bad in ((0, 0, 16), (0, 0, 16, 8, 1), (-1, 0, 16, 8), (0, -1, 16, 8), (0.0, 0, 16, 8), (0, 0, 16.0, 8), "abcd", 5,
                (True, 0, 16, 8), (49, 0, 16, 8), (0, 41, 16, 8), (0, 0, 65, 8), (0, 0, 16, 49)):
        with pytest.raises(ValueError):
            cloud(small, rig, 1000.0, 12.0, roi=bad)
        with pytest.raises(ValueError):
            geometry(rig, 1000.0, 12.0, bad)
    # z_plane, period, k
    for bad in (np.nan, np.inf, -np.inf, "1", None, 1j, [1.0], True):
        with pytest.raises(ValueError):
            cloud(p, rig, bad, 12.0)
        with pytest.raises(ValueError):
            cloud(p, rig, 1000.0, bad)
        with pytest.raises(ValueError):
            cloud(p, rig, 1000.0, 12.0, k=bad)
        with pytest.raises(ValueError):
            order(p, stripe, rig, 1000.0, 12.0, bad)
    for zero in (0, 0.0, -0.0):
        with pytest.raises(ValueError):
            cloud(p, rig, 1000.0, zero)
    # a tilted sensor; an epipole at infinity
    with pytest.raises(NotImplementedError):
        cloud(p, _rig(ss, distCoeffs2=[0.0] * 12 + [0.01, 0.0]), 1000.0, 12.0)
    with pytest.raises(NotImplementedError):
        geometry(_rig(ss, distCoeffs2=[0.0] * 13 + [0.01]), 1000.0, 12.0)
    with pytest.raises(ValueError) as ei:
        cloud(p, _rig(ss, T=[-250.0, 10.0, 0.0]), 1000.0, 12.0)
    assert "epipole" in str(ei.value)
    # the stripe
    for bad in (np.zeros((0, 2), dtype=np.int64), np.array([3, 4]), np.array([[3.0, 4.0]]), np.array([[3, 4, 5]]),
                np.array([[64, 4]]), np.array([[3, 48]]), np.array([[-1, 4]]), np.array([[True, False]]), None):
        with pytest.raises(ValueError):
            order(p, bad, rig, 1000.0, 12.0, 640.0)
    # a packed geometry takes no second z_plane, period or roi
    G = geometry(rig, 1000.0, 12.0)
    for kw in ({"z_plane": 1000.0}, {"period": 12.0}, {"roi": (0, 0, 64, 48)}):
        with pytest.raises(ValueError):
            cloud(p, G, **kw)


def test_empty_maps_give_empty_clouds(ss_no_native):
    ss = ss_no_native
    rig = _rig(ss)
    for roi in ((0, 0, 0, 48), (0, 0, 64, 0), (5, 5, 0, 0), (64, 48, 0, 0)):
        out = ss.active.ftpCloud(np.zeros((roi[3], roi[2])), rig, 1000.0, 12.0, roi=roi)
        assert out.shape == (roi[3], roi[2], 3) and out.dtype == np.float64


def test_what_reaches_the_library(monkeypatch):
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    calls = []

    class Lib:
        def ssamd_ftp_cloud(self, src, h, w, x0, y0, geom, k, out, dev):
            g = np.ctypeslib.as_array(ctypes.cast(geom, ctypes.POINTER(ctypes.c_double)), (R.NGEOM,)).copy()
            p = np.ctypeslib.as_array(ctypes.cast(src, ctypes.POINTER(ctypes.c_double)), (h * w,)).copy().reshape(h, w)
            calls.append((p, h, w, x0, y0, g, k, dev))
            return 0
    monkeypatch.setattr(_native, "lib", lambda: Lib())
    c = R.load_case("p5x257_roi")
    rig = R.make_rig(ss, c["rig"])
    out = ss.active.ftpCloud(c["phase"], rig, c["z_plane"], c["period"], c["k"], tuple(c["roi"]))
    p, h, w, x0, y0, g, k, dev = calls[-1]
    assert out.shape == (5, 257, 3) and (h, w, x0, y0, k, dev) == (5, 257, 37, 11, 1.0, -1)
    assert np.array_equal(g, R.geometry(c["rig"], c["z_plane"], c["period"])[0]) and np.array_equal(p, c["phase"])
    big = np.zeros((10, 600))
    big[::2, 1:258] = c["phase"]
    view = big[::2, 1:258]
    assert not view.flags["C_CONTIGUOUS"]
    ss.active.ftpCloud(view, rig, c["z_plane"], c["period"], np.int64(-3), tuple(c["roi"]))
    assert np.array_equal(calls[-1][0], c["phase"]) and calls[-1][6] == -3.0


# ---------------------------------------------------------------------------------------------- exports and the C ABI
def test_exported_and_documented():
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    a = ss.active
    assert {"ftpPhase", "ftpCloud", "ftpFringeOrder", "ftpGeometry", "FtpGeometry"} <= set(a.__all__)
    for text in ("active.py:776-841", "``ftpCloud``", "``ftpFringeOrder``", "``ftpGeometry``", "ssamd_ftp_cloud",
                 "``NotImplementedError``", "epipole"):
        assert text in a.__doc__, text
    assert "active.py:776-841" in a.ftpCloud.__doc__ and "active.py:779-788" in a.ftpFringeOrder.__doc__
    assert "StereoFTP" in a.ftpFringeOrder.__doc__ and "rectification.py:271-302" in a.ftpGeometry.__doc__
    header = open(os.path.join(ROOT, "include", "ssamd.h")).read()
    for decl in ("int ssamd_ftp_cloud(const double *phase, int h, int w, int x0, int y0, const double *geom, double k, double *out, int device);",
                 "int ssamd_ftp_cloud_device(const double *d_phase, int h, int w, int x0, int y0, const double *geom, double k, double *d_out,",
                 "#define SSAMD_FTP_CLOUD_NGEOM %d" % a.NGEOM, "active.py:776-841"):
        assert decl in header, decl
    lib = _native.lib()
    assert hasattr(lib, "ssamd_ftp_cloud") and hasattr(lib, "ssamd_ftp_cloud_device")
    name = lib.ssamd_kernel_name(_native.K_REPROJECT)
    assert b"reproject_kernel" in name and b"ftp_cloud_kernel" in name


def test_abi_version_and_slot_count_are_unchanged():
    from simplestereo_amd import _native
    header = open(os.path.join(ROOT, "include", "ssamd.h")).read()
    assert "#define SSAMD_ABI_VERSION 8 " in header and _native.ABI_VERSION == 8 and _native.lib().ssamd_abi_version() == 8
    assert "#define SSAMD_K_COUNT 12\n" in header and _native.K_COUNT == 12
    assert "#define SSAMD_K_REPROJECT %d " % _native.K_REPROJECT in header


def test_library_refuses_bad_arguments_without_a_device():
    """The argument checks of ssamd_ftp_cloud* come before the device is touched: they answer on a machine without one."""
    from simplestereo_amd import _native
    lib = _native.lib()
    c = R.load_case("p1x5")
    g = np.array(c["g"])
    p, out = np.array(c["phase"]), np.zeros((1, 5, 3))
    P, O, GP = p.ctypes.data, out.ctypes.data, g.ctypes.data
    for host in (True, False):
        f = lib.ssamd_ftp_cloud if host else lib.ssamd_ftp_cloud_device
        last = -1 if host else None
        assert f(None, 1, 5, 0, 0, GP, 0.0, O, last) == EINVAL and b"NULL" in lib.ssamd_last_error()
        assert f(P, 1, 5, 0, 0, GP, 0.0, None, last) == EINVAL
        assert f(P, 1, 5, 0, 0, None, 0.0, O, last) == EINVAL
        for h, w, x0, y0 in ((-1, 5, 0, 0), (1, -5, 0, 0), (1, 5, -1, 0), (1, 5, 0, -1)):
            assert f(P, h, w, x0, y0, GP, 0.0, O, last) == EINVAL
        assert f(P, 2 ** 16, 2 ** 15, 0, 0, GP, 0.0, O, last) == EINVAL and b"2^31" in lib.ssamd_last_error()
        assert f(P, 2 ** 30, 2, 0, 0, GP, 0.0, O, last) == EINVAL
        for k in (np.nan, np.inf, -np.inf):
            assert f(P, 1, 5, 0, 0, GP, k, O, last) == EINVAL
        for i in (0, 16, 39, R.NGEOM - 1):
            bad = g.copy()
            bad[i] = np.nan if i % 2 else np.inf
            assert f(P, 1, 5, 0, 0, bad.ctypes.data, 0.0, O, last) == EINVAL and b"geom[%d]" % i in lib.ssamd_last_error()
        assert f(None, 0, 5, 0, 0, GP, 0.0, None, last) == 0 and f(None, 5, 0, 3, 4, GP, 0.0, None, last) == 0      # an empty map
