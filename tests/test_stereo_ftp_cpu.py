"""CPU tier of ss.active.StereoFTP's front end: the bicubic weight table and ``_rigs._remap(INTER_CUBIC)``, the fill of
``findCentralStripe`` against scipy, ``buildFringe`` / ``_getCentralPeak``, the host steps ``_triangulate`` and
``_calculateCameraFrequency`` against tests/_stereo_ftp_ref.py, the second public header include/ssamd_active.h against its
ctypes rows (with include/ssamd.h unchanged), and the exceptions.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _ftp_cloud_ref as C
import _stereo_ftp_ref as S
from test_native_signatures_cpu import SCALARS, _is_pointer_class, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ the table, the remap
def test_cubic_table_properties(ss):
    from simplestereo_amd import _rigs
    t = _rigs._cubic_table()
    assert t.shape == (32, 32, 4, 4) and t.dtype == np.int16 and not t.flags.writeable
    assert np.array_equal(t, S.cubic_table())                                   # the two statements agree
    t = t.astype(np.int64)
    assert (t.reshape(1024, 16).sum(axis=1) == 32768).all()                     # every 16-tap set sums to exactly 32768
    # fraction (0, 0) is the identity tap: 1.0 saturates to 32767 in a short and the correction puts the 1 on tap (2, 2),
    # which no 8-bit neighbourhood can see: (32767 a + b + 16384) >> 15 == a for a, b in 0 .. 255
    want = np.zeros((4, 4), np.int64)
    want[1, 1], want[2, 2] = 32767, 1
    assert np.array_equal(t[0, 0], want)
    a, b = np.meshgrid(np.arange(256), np.arange(256))
    assert np.array_equal((32767 * a + b + 16384) >> 15, a)
    # x / y symmetry: swapping the fractions transposes the taps -- of the weights as rounded; the ONE corrected tap of an entry
    # is found by a scan that is not symmetric ((2, 3) comes before (3, 2)), so an entry and its mirror may differ on those two taps
    d = t - t.transpose(1, 0, 3, 2)
    free = np.ones((4, 4), bool)
    free[2, 3] = free[3, 2] = False
    assert not d[:, :, free].any()
    assert np.abs(d).max() <= 2 and np.count_nonzero(d.any(axis=(2, 3))) <= 32
    # the rows and columns of an entry are the 1-D cubic weights: along x at fy = 0, along y at fx = 0, up to the correction
    assert np.abs(t[0, :, 1, :] - t[:, 0, :, 1]).max() <= 1


def test_cubic_coefficients_are_exact_in_float32():
    """interpolateCubic at i / 32 with A = -0.75 is exact in float32 (multiples of 2^-17): the table does not depend on the
    order of its operations or on fused multiply-adds"""
    from fractions import Fraction as F
    A = F(-3, 4)
    f = np.float32
    for i in range(32):
        x = F(i, 32)
        c = [((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A, ((A + 2) * x - (A + 3)) * x * x + 1,
             ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1]
        c.append(1 - sum(c))
        row = S.cubic_table()[i, 0, :, 1]                  # fx = 0: the x weights are (0, 32767 | 32768, 0, 0)
        for k in range(4):
            assert F(float(f(float(c[k])))) == c[k]
            assert abs(int(row[k]) - round(float(c[k]) * 32767)) <= 2


def test_remap_cubic_integer_maps_are_the_identity(ss):
    from simplestereo_amd import _rigs
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (13, 17), dtype=np.uint8)
    yy, xx = np.mgrid[0:13, 0:17].astype(np.float32)
    assert np.array_equal(_rigs._remap(img, xx, yy, _rigs.INTER_CUBIC), img)
    bgr = rng.integers(0, 256, (13, 17, 3), dtype=np.uint8)
    assert np.array_equal(_rigs._remap(bgr, xx, yy, _rigs.INTER_CUBIC), bgr)
    # shifted by whole pixels: the border is 0
    got = _rigs._remap(img, xx + 3, yy - 2, _rigs.INTER_CUBIC)
    want = np.zeros_like(img)
    want[2:, :14] = img[:11, 3:]
    assert np.array_equal(got, want)


def test_remap_cubic_equals_the_restatement_with_borders_and_non_finite_maps(ss):
    from simplestereo_amd import _rigs
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (7, 64), dtype=np.uint8)
    mx = rng.uniform(-6, 70, (40, 90)).astype(np.float32)
    my = rng.uniform(-6, 13, (40, 90)).astype(np.float32)
    mx[0, :6] = [np.nan, np.inf, -np.inf, 2.0 ** 26, -2.0 ** 27, 3e38]
    my[1, :3] = [np.nan, np.inf, -1e30]
    got = _rigs._remap(img, mx, my, _rigs.INTER_CUBIC)
    assert got.dtype == np.uint8 and np.array_equal(got, S.remap_cubic(img, mx, my))
    assert not got[0, :6].any() and not got[1, :3].any() and got.any()
    for dtype in (np.uint16, np.float32):
        with pytest.raises(NotImplementedError):
            _rigs._remap(img.astype(dtype), mx, my, _rigs.INTER_CUBIC)
    with pytest.raises(NotImplementedError):
        _rigs._remap(img, mx, my, 4)


# ------------------------------------------------------------------------------------------------ the stripe's fill
@pytest.mark.parametrize("rows", ["all_valid", "gaps_inside", "gaps_at_both_ends"])
def test_fill_equals_scipy_bit_for_bit(ss, rows):
    interp1d = pytest.importorskip("scipy.interpolate").interp1d
    rng = np.random.default_rng(7)
    x = 80 + np.cumsum(rng.normal(0, 0.7, 48))
    if rows != "all_valid":
        x[[5, 6, 7, 20, 33, 34]] = np.nan
    if rows == "gaps_at_both_ends":
        x[:3] = np.nan
        x[-2:] = np.nan
    y = np.arange(0.5, 48, 1)
    valid = ~np.isnan(x)
    want = interp1d(y[valid], x[valid], kind="linear", fill_value="extrapolate")(y)
    got = ss.active._fill_linear(y, x)
    assert _same(got, want) and _same(got, S.fill_linear(y, x))
    assert np.isfinite(got).all() and np.abs(got[valid] - x[valid]).max() < 1e-12        # the knots, to the last bit or so


# ------------------------------------------------------------------------------------------------ fringes
@pytest.mark.parametrize("period,shift,dims", [(12.0, 0, (1280, 720)), (10.5, 2.5, (333, 5)), (17.3, -4.0, (64, 3))])
def test_build_fringe_and_central_peak_equal_the_restated_formulas(ss, period, shift, dims):
    assert ss.active._getCentralPeak(dims[0], period, shift) == S.central_peak(dims[0], period, shift)
    for color in (None, "r", "green", "b"):
        got = ss.active.buildFringe(period, shift, dims, stripeColor=color)
        assert _same(got, S.build_fringe(period, shift, dims, color))
    f = ss.active.buildFringe(period, shift, dims, stripeColor="red")
    assert f.shape == (dims[1], dims[0], 3) and f.dtype == np.uint8
    left = int(S.central_peak(dims[0], period, shift) - period / 2)
    assert not f[:, left:int(left + period), :2].any() and f[:, left:int(left + period), 2].any()
    v = ss.active.buildFringe(period, shift, dims, vertical=True)
    assert v.shape == (dims[1], dims[0]) and np.array_equal(v[:, 0], v[:, -1])
    assert ss.active.buildFringe(period, dims=dims, dtype=np.float64).max() <= 1.0
    with pytest.raises(ValueError):
        ss.active.buildFringe(period, dims=dims, stripeColor="yellow")


# ------------------------------------------------------------------------------------------------ the host steps
@pytest.mark.parametrize("name", ["full", "roi", "roi_camera_dist"])
def test_host_steps_equal_the_restatement(ss, name):
    """StereoFTP's attributes, _undistort of a host frame, _triangulate and _calculateCameraFrequency, bit for bit"""
    c = S.load_cases("cloud")[name]
    fringe = S.build_fringe(c["period"], stripeColor="r")
    rg = S.Rig(c["rig"], c["period"], fringe.shape[1])
    sf = ss.active.StereoFTP(C.make_rig(ss, c["rig"]), fringe, c["period"])
    assert sf.fringeDims == (1280, 720) and sf.fp == rg.fp and sf.stripeCentralPeak == rg.peak
    assert _same(sf.fringe, np.max(fringe, axis=2))
    assert _same(sf.F, rg.F) and _same(sf.Rectify1, rg.Rectify1) and _same(sf.Rectify2, rg.Rectify2)
    assert sf.R_inv.shape == (4, 4) and _same(sf.R_inv[:3, :3], rg.R_inv) and sf.R_inv[3].tolist() == [0, 0, 0, 1]
    assert sf.ep.shape == (3, 1) and sf.ep[2, 0] == 1
    x0, y0, w, h = c["roi"] or (0, 0) + tuple(c["rig"]["res1"])
    want = S.pipeline(c["rig"], fringe, c["period"], np.array(c["frame"]), c["roi"])
    und = sf._undistort(np.array(c["frame"]))[y0:y0 + h, x0:x0 + w]
    assert _same(und, want["undistorted"])
    stripe = np.array(want["stripe"])
    world = sf._triangulate(stripe, sf.stripeCentralPeak, (x0, y0, w, h))
    assert _same(stripe, want["stripe"])                                        # not modified in place
    assert _same(world, S.triangulate(rg, stripe, rg.peak, (x0, y0, w, h))) and np.mean(world[:, 2]) == want["z_plane"]
    assert _same(sf._calculateCameraFrequency(world), want["fc"])
    assert abs(want["z_plane"] - 1000) < 40 and np.abs(1 / want["fc"] - 12).max() < 1          # a sensible scene
    g = ss.active.ftpGeometry(sf.stereoRig, want["z_plane"], c["period"], c["roi"])
    assert _same(g.geom, want["geom"])


# ------------------------------------------------------------------------------------------------ the second header
@pytest.fixture(scope="module")
def active_header():
    with open(os.path.join(ROOT, "include", "ssamd_active.h")) as f:
        return f.read()


def test_active_header_parses_and_matches_its_ctypes_rows(active_header):
    from simplestereo_amd import _native
    protos = _prototypes(active_header)
    assert sorted(protos) == ["ssamd_ftp_reference", "ssamd_ftp_reference_device", "ssamd_stripe_centroids", "ssamd_stripe_centroids_device"]
    assert set(protos) == set(re.findall(r"\b(ssamd_[a-z0-9_]+)\s*\(", active_header))
    assert int(re.search(r"#define SSAMD_ACTIVE_VERSION (\d+)", active_header).group(1)) == _native.ACTIVE_VERSION == 1
    assert protos["ssamd_ftp_reference"] == ("int", ["ptr"] + ["int"] * 6 + ["ptr", "ptr", "int"])
    assert protos["ssamd_stripe_centroids_device"] == ("int", ["ptr", "int", "int", "int", "int", "ptr", "ptr"])
    lib = _native.lib()
    for name, (ret, kinds) in protos.items():
        fn = getattr(lib, name)                                                 # exported from the same library
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(fn.argtypes, kinds)):
            assert _is_pointer_class(t) if kind == "ptr" else t is SCALARS[kind], (name, i, t, kind)


def test_the_first_header_is_unchanged():
    with open(os.path.join(ROOT, "include", "ssamd.h")) as f:
        header = f.read()
    from simplestereo_amd import _native
    assert len(_prototypes(header)) == 54
    assert "#define SSAMD_ABI_VERSION 8" in header and _native.ABI_VERSION == 8
    assert "#define SSAMD_K_COUNT 12" in header and _native.K_COUNT == 12
    assert "ssamd_ftp_reference" not in header and "ssamd_stripe" not in header


def test_native_run_takes_a_dtype(ss):
    from simplestereo_amd import _native
    import inspect
    assert inspect.signature(_native.run).parameters["dtype"].default is np.float64
    out = _native.run("ssamd_ftp_reference", (np.zeros((1, 1), np.uint8),), (0, 5), None, dtype=np.uint8)      # empty: no native call
    assert out.shape == (0, 5) and out.dtype == np.uint8


# ------------------------------------------------------------------------------------------------ exceptions
def test_exceptions(ss):
    a = ss.active
    assert {"ftpReference", "findCentralStripe", "buildFringe", "StereoFTP"} <= set(a.__all__)
    rig = C.make_rig(ss, C.rig_params(res1=(160, 48)))
    fringe = S.build_fringe(12.0, stripeColor="r")
    img = np.zeros((48, 160, 3), np.uint8)
    # findCentralStripe: the reference's checks and messages
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="Threshold must be in the interval"):
            a.findCentralStripe(img, sensitivity=bad)
    with pytest.raises(ValueError, match="Color value not permitted"):
        a.findCentralStripe(img, color="yellow")
    with pytest.raises(TypeError):
        a.findCentralStripe(img.astype(np.uint16))
    with pytest.raises(TypeError):
        a.findCentralStripe([[1, 2, 3]])
    with pytest.raises(ValueError):
        a.findCentralStripe(img[:, :, 0])
    assert a.findCentralStripe(np.zeros((0, 5, 3), np.uint8)) is None and a.findCentralStripe(np.zeros((5, 0, 3), np.uint8)) is None
    # ftpReference
    with pytest.raises(TypeError):
        a.ftpReference(fringe.astype(np.float32), rig, 1000.0)
    with pytest.raises(ValueError):
        a.ftpReference(fringe[:, :, :2], rig, 1000.0)
    with pytest.raises(ValueError, match="at least one pixel"):
        a.ftpReference(np.zeros((0, 4), np.uint8), rig, 1000.0)
    with pytest.raises(ValueError):
        a.ftpReference(fringe, rig, float("inf"))
    with pytest.raises(ValueError):
        a.ftpReference(fringe, rig, 1000.0, roi=(100, 0, 100, 10))
    packed = a.ftpGeometry(rig, 1000.0, 12.0)
    with pytest.raises(ValueError, match="pass None"):
        a.ftpReference(fringe, packed, 1000.0)
    tilted = C.rig_params(res1=(160, 48))
    tilted["distCoeffs2"] = [0.0] * 12 + [0.01, 0.0]
    with pytest.raises(NotImplementedError):
        a.ftpReference(fringe, C.make_rig(ss, tilted), 1000.0)
    assert a.ftpReference(fringe, rig, 1000.0, roi=(0, 0, 0, 0)).shape == (0, 0)
    # StereoFTP.getCloud
    sf = a.StereoFTP(rig, fringe, 12.0)
    with pytest.raises(ValueError, match="image must be a BGR color image!"):
        sf.getCloud(img[:, :, 0])
    with pytest.raises(NotImplementedError):
        sf.getCloud(img, plot=True)
    with pytest.raises(TypeError):
        sf.getCloud([[[0, 0, 0]]])
    with pytest.raises(ValueError, match="camera resolution"):
        sf.getCloud(np.zeros((40, 160, 3), np.uint8))
    with pytest.raises(ValueError):
        sf.getCloud(img, roi=(0, 0, 161, 48))


def test_interpolation_kinds_other_than_linear_need_scipy(ss, monkeypatch):
    """no scipy at import time; another kind without scipy is NotImplementedError"""
    import subprocess
    import sys
    code = "import sys; import simplestereo_amd; assert not any(m == 'scipy' or m.startswith('scipy.') for m in sys.modules)"
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0
    monkeypatch.setitem(sys.modules, "scipy.interpolate", None)                 # `from scipy.interpolate import ...` raises ImportError
    monkeypatch.setattr(ss.active._native, "run", lambda *a, **k: np.array([1.0, np.nan, 2.0, 4.0]))
    img = np.zeros((4, 8, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="scipy"):
        ss.active.findCentralStripe(img, interpolation="cubic")
    assert ss.active.findCentralStripe(img)[:, 0].tolist() == [1.0, 1.5, 2.0, 4.0]
