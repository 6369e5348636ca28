"""CPU tier of FTP without a reference plane (ss.active.ftpCarrierPhase, ftpStripePhase, ftpMappingCloud, StereoFTP_Mapping,
StereoFTP_PhaseOnly): the fourth public header include/ssamd_ftp_mapping.h against its ctypes rows (the three older headers
unchanged), the argument errors of its entry points, the exceptions, tests/_ftp_mapping_ref.py against scipy and against the
BLAS restatement of _triangulate, the conditioning of the golden cases, and the two classes on a library stub.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import _ftp_cloud_ref as C
import _ftp_mapping_ref as M
import _ftp_ref as P
import _stereo_ftp_ref as S
from test_native_signatures_cpu import SCALARS, _is_pointer_class, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ELIMIT = -1, -5
NAMES = ["ssamd_ftp_carrier_phase", "ssamd_ftp_carrier_phase_device", "ssamd_ftp_mapping_cloud", "ssamd_ftp_mapping_cloud_device"]


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


# ------------------------------------------------------------------------------------------------ the fourth header
def test_mapping_header_parses_and_matches_its_ctypes_rows():
    from simplestereo_amd import _native
    with open(os.path.join(ROOT, "include", "ssamd_ftp_mapping.h")) as f:
        header = f.read()
    protos = _prototypes(header)
    assert sorted(protos) == NAMES
    assert set(protos) == set(re.findall(r"\b(ssamd_[a-z0-9_]+)\s*\(", header))
    assert int(re.search(r"#define SSAMD_FTP_MAPPING_VERSION (\d+)", header).group(1)) == _native.FTP_MAPPING_VERSION == 1
    assert protos["ssamd_ftp_carrier_phase"] == ("int", ["ptr", "int", "int", "int", "ptr", "ptr", "int", "double", "ptr", "int"])
    assert protos["ssamd_ftp_carrier_phase_device"][1][-1] == "ptr"
    assert protos["ssamd_ftp_mapping_cloud"] == ("int", ["ptr", "int", "int", "int", "int", "ptr", "ptr", "double", "double", "ptr", "int"])
    assert protos["ssamd_ftp_mapping_cloud_device"][1][-1] == "ptr"
    lib = _native.lib()
    for name, (ret, kinds) in protos.items():
        fn = getattr(lib, name)                                                 # exported from the same library
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(kinds), name
        for i, (t, kind) in enumerate(zip(fn.argtypes, kinds)):
            assert _is_pointer_class(t) if kind == "ptr" else t is SCALARS[kind], (name, i, t, kind)


def test_the_older_headers_are_unchanged():
    from simplestereo_amd import _native
    for name, count in (("ssamd.h", 54), ("ssamd_active.h", 4), ("ssamd_graycode.h", 6)):
        with open(os.path.join(ROOT, "include", name)) as f:
            header = f.read()
        assert len(_prototypes(header)) == count
        assert "ftp_carrier" not in header and "ftp_mapping" not in header
    assert _native.ABI_VERSION == 8 and _native.K_COUNT == 12 and _native.lib().ssamd_abi_version() == 8
    assert _native.lib().ssamd_kernel_name(_native.K_FTP) == b"ftp_phase_kernel"


def test_abi_argument_errors_need_no_device():
    """SSAMD_EINVAL / SSAMD_ELIMIT for what include/ssamd_ftp_mapping.h lists, decided before any device is looked for"""
    from simplestereo_amd import _native
    lib = _native.lib()
    img, f, out = np.zeros((2, 8), np.uint8), np.full(2, 0.25), np.zeros((2, 8))
    I, F, O = img.ctypes.data, f.ctypes.data, out.ctypes.data
    for host in (True, False):
        fn = lib.ssamd_ftp_carrier_phase if host else lib.ssamd_ftp_carrier_phase_device
        last = -1 if host else None
        assert fn(None, 1, 2, 8, F, F, 0, 1.0, O, last) == EINVAL and b"NULL" in lib.ssamd_last_error()
        assert fn(I, 1, 2, 8, F, F, 0, 1.0, None, last) == EINVAL
        assert fn(I, 1, 2, 8, None, F, 0, 1.0, O, last) == EINVAL and fn(I, 1, 2, 8, F, None, 0, 1.0, O, last) == EINVAL
        for ch in (0, 2, 4):
            assert fn(I, ch, 2, 8, F, F, 0, 1.0, O, last) == EINVAL
        for h, w in ((0, 8), (2, 0), (-1, 8), (2, -8)):
            assert fn(I, 1, h, w, F, F, 0, 1.0, O, last) == EINVAL
        for uw in (-1, 3):
            assert fn(I, 1, 2, 8, F, F, uw, 1.0, O, last) == EINVAL
        assert fn(I, 1, 2, 8, F, F, 1, 1.5, O, last) == EINVAL and lib.ssamd_last_error() == b"Wrong tau value!"
        assert fn(I, 1, 2, 8193, F, F, 0, 1.0, O, last) == ELIMIT and b"8192" in lib.ssamd_last_error()

    g, Fm = np.ones(68), np.arange(1.0, 10.0)
    p, pts = np.zeros((1, 5)), np.zeros((1, 5, 3))
    Pp, Op = p.ctypes.data, pts.ctypes.data
    for host in (True, False):
        fn = lib.ssamd_ftp_mapping_cloud if host else lib.ssamd_ftp_mapping_cloud_device
        last = -1 if host else None
        assert fn(None, 1, 5, 0, 0, _dp(g), _dp(Fm), 0.0, 0.0, Op, last) == EINVAL and b"NULL" in lib.ssamd_last_error()
        assert fn(Pp, 1, 5, 0, 0, _dp(g), _dp(Fm), 0.0, 0.0, None, last) == EINVAL
        assert fn(Pp, 1, 5, 0, 0, None, _dp(Fm), 0.0, 0.0, Op, last) == EINVAL
        assert fn(Pp, 1, 5, 0, 0, _dp(g), None, 0.0, 0.0, Op, last) == EINVAL
        for h, w, x0, y0 in ((-1, 5, 0, 0), (1, -5, 0, 0), (1, 5, -1, 0), (1, 5, 0, -1)):
            assert fn(Pp, h, w, x0, y0, _dp(g), _dp(Fm), 0.0, 0.0, Op, last) == EINVAL
        assert fn(Pp, 2 ** 16, 2 ** 15, 0, 0, _dp(g), _dp(Fm), 0.0, 0.0, Op, last) == EINVAL and b"2^31" in lib.ssamd_last_error()
        for bad in (np.nan, np.inf, -np.inf):
            assert fn(Pp, 1, 5, 0, 0, _dp(g), _dp(Fm), bad, 0.0, Op, last) == EINVAL
            assert fn(Pp, 1, 5, 0, 0, _dp(g), _dp(Fm), 0.0, bad, Op, last) == EINVAL
        for i in (12, 36, 39, 40, 67):                                          # read: must be finite
            b = g.copy()
            b[i] = np.inf
            assert fn(Pp, 1, 5, 0, 0, _dp(b), _dp(Fm), 0.0, 0.0, Op, last) == EINVAL and b"geom[%d]" % i in lib.ssamd_last_error()
        b = Fm.copy()
        b[4] = np.nan
        assert fn(Pp, 1, 5, 0, 0, _dp(g), _dp(b), 0.0, 0.0, Op, last) == EINVAL and b"F[4]" in lib.ssamd_last_error()
        b = g.copy()
        b[[0, 11, 37, 38]] = np.nan                                             # not read: M, T, the epipole
        assert fn(None, 0, 5, 0, 0, _dp(b), _dp(Fm), 0.0, 0.0, None, last) == 0  # ... and an empty map does nothing
        assert fn(None, 5, 0, 3, 4, _dp(g), _dp(Fm), 0.0, 0.0, None, last) == 0


# ------------------------------------------------------------------------------------------------ exceptions
def test_exported_and_documented(ss):
    a = ss.active
    assert {"ftpCarrierPhase", "ftpStripePhase", "ftpMappingCloud", "StereoFTP_Mapping", "StereoFTP_PhaseOnly"} <= set(a.__all__)
    assert issubclass(a.StereoFTP_Mapping, a.StereoFTP) and issubclass(a.StereoFTP_PhaseOnly, a.StereoFTP)
    assert "are not here" not in a.__doc__ and "StereoFTPAnaglyph`` stays out" in a.__doc__
    for text in ("active.py:1266-1450", "ssamd_ftp_mapping.h", "``ftpCarrierPhase``", "``ftpStripePhase``", "``ftpMappingCloud``"):
        assert text in a.__doc__, text
    for cls in (a.StereoFTP_Mapping, a.StereoFTP_PhaseOnly):                    # inherited, not copied
        for name in ("_triangulate", "_calculateCameraFrequency", "_frame", "convertGrayscale"):
            assert getattr(cls, name) is getattr(a.StereoFTP, name)


def test_exceptions(ss):
    a = ss.active
    img = np.zeros((4, 16), np.uint8)
    with pytest.raises(TypeError):
        a.ftpCarrierPhase(img.astype(np.float32), 0.1)
    with pytest.raises(TypeError):
        a.ftpCarrierPhase([[1, 2]], 0.1)
    with pytest.raises(ValueError):
        a.ftpCarrierPhase(np.zeros((4, 16, 2), np.uint8), 0.1)
    for fc in ("0.1", [0.1, 0.2], None):
        with pytest.raises(ValueError):
            a.ftpCarrierPhase(img, fc)
    with pytest.raises(ValueError):
        a.ftpCarrierPhase(img, 0.1, radius_factor="x")
    with pytest.raises(ValueError, match="unwrap must be"):
        a.ftpCarrierPhase(img, 0.1, unwrap="scipy")
    with pytest.raises(ValueError, match="Wrong tau value"):
        a.ftpCarrierPhase(img, 0.1, unwrap="iir", tau=1.5)
    with pytest.raises(ValueError, match="8192"):
        a.ftpCarrierPhase(np.zeros((2, a.MAX_WIDTH + 1), np.uint8), 0.05)
    assert a.ftpCarrierPhase(np.zeros((0, 7), np.uint8), 0.1).shape == (0, 7)   # empty: no native call

    ph = np.zeros((4, 6))
    with pytest.raises(TypeError):
        a.ftpStripePhase(ph.astype(np.float32), [[1.0, 1.0]])
    with pytest.raises(TypeError):
        a.ftpStripePhase(ph.tolist(), [[1.0, 1.0]])
    with pytest.raises(ValueError):
        a.ftpStripePhase(ph[0], [[1.0, 1.0]])
    for bad in ([1.0, 1.0], np.zeros((0, 2)), [[1.0, np.nan]], [[1.0, 2.0, 3.0]], "xy"):
        with pytest.raises(ValueError, match="stripe"):
            a.ftpStripePhase(ph, bad)
    with pytest.raises(ValueError):
        a.ftpStripePhase(np.zeros((0, 6)), [[1.0, 1.0]])

    rig = C.make_rig(ss, C.rig_params(res1=(160, 48)))
    ph = np.zeros((48, 160))
    with pytest.raises(TypeError):
        a.ftpMappingCloud(ph.astype(np.float32), rig, 12.0, 640.0)
    with pytest.raises(ValueError):
        a.ftpMappingCloud(ph[:40], rig, 12.0, 640.0)
    with pytest.raises(ValueError):
        a.ftpMappingCloud(ph, rig, 12.0, 640.0, roi=(100, 0, 100, 10))
    for period in (0, float("inf"), "12", None):
        with pytest.raises(ValueError):
            a.ftpMappingCloud(ph, rig, period, 640.0)
    for peak, theta in ((float("nan"), 0.0), (None, 0.0), (640.0, float("inf")), (640.0, "0")):
        with pytest.raises(ValueError):
            a.ftpMappingCloud(ph, rig, 12.0, peak, theta)
    packed = a.ftpMappingGeometry(rig, 12.0)
    assert packed.geom.shape == (68,) and packed.F.shape == (9,) and packed.roi == (0, 0, 160, 48) and not packed.geom[:12].any()
    with pytest.raises(ValueError, match="pass None"):
        a.ftpMappingCloud(ph, packed, 12.0, 640.0)
    with pytest.raises(ValueError, match="ftpMappingGeometry"):
        a.ftpMappingCloud(ph, a.ftpGeometry(rig, 1000.0, 12.0), None, 640.0)
    tilted = C.rig_params(res1=(160, 48))
    tilted["distCoeffs2"] = [0.0] * 12 + [0.01, 0.0]
    with pytest.raises(NotImplementedError):
        a.ftpMappingCloud(ph, C.make_rig(ss, tilted), 12.0, 640.0)
    assert a.ftpMappingCloud(np.zeros((0, 0)), rig, 12.0, 640.0, roi=(0, 0, 0, 0)).shape == (0, 0, 3)

    fringe = S.build_fringe(12.0, stripeColor="r")
    frame = np.zeros((48, 160, 3), np.uint8)
    for obj, call in ((a.StereoFTP_Mapping(rig, fringe, 12.0), "getCloud"), (a.StereoFTP_PhaseOnly(rig, fringe, 12.0), "getPhase")):
        f = getattr(obj, call)
        with pytest.raises(ValueError, match="image must be a BGR color image!"):
            f(frame[:, :, 0])
        with pytest.raises(NotImplementedError):
            f(frame, plot=True)
        with pytest.raises(TypeError):
            f([[[0, 0, 0]]])
        with pytest.raises(ValueError, match="camera resolution"):
            f(np.zeros((40, 160, 3), np.uint8))
        with pytest.raises(ValueError):
            f(frame, roi=(0, 0, 161, 48))


# ------------------------------------------------------------------------------------------------ the restatement itself
def _stripe_points(h, w):
    rng = np.random.default_rng(11)
    inside = np.stack([rng.uniform(0, w - 1, 40), rng.uniform(0, h - 1, 40)], axis=1)
    edges = [[0.0, 0.0], [w - 1.0, h - 1.0], [w - 1.0, 2.5], [3.25, h - 1.0], [0.0, h - 1.0], [w - 1.0, 0.0], [5.0, 3.0], [0.5, 0.5]]
    outside = [[-1e-9, 3.0], [w - 1 + 1e-9, 3.0], [4.0, -0.5], [4.0, h - 0.5], [-3.0, -3.0], [w + 5.0, 2.0]]
    return inside, np.array(edges), np.array(outside)


def test_stripe_phase_equals_scipy(ss):
    """within 16 * 2^-52 * max|phase|: a bilinear sample is under eight roundings, each at most one ulp of the largest operand,
    doubled for scipy's own order of operations; points on the last row and column, and outside (0.0)"""
    map_coordinates = pytest.importorskip("scipy.ndimage").map_coordinates
    rng = np.random.default_rng(3)
    h, w = 9, 13
    phase = np.cumsum(rng.normal(0.6, 0.2, (h, w)), axis=1) * 40 + rng.normal(0, 1, (h, 1))
    tol = 16 * 2.0 ** -52 * np.abs(phase).max()
    inside, edges, outside = _stripe_points(h, w)
    for pts in (inside, edges, outside, np.vstack([inside, edges, outside])):
        want = map_coordinates(phase, (pts[:, 1], pts[:, 0]), order=1)
        each = np.array([M.stripe_phase(phase, pts[i:i + 1]) for i in range(len(pts))])
        assert np.abs(each - want).max() <= tol
        assert abs(M.stripe_phase(phase, pts) - np.mean(want)) <= tol
        assert ss.active.ftpStripePhase(phase, pts) == M.stripe_phase(phase, pts)                # the package: the same formula
    assert all(M.stripe_phase(phase, outside[i:i + 1]) == 0.0 for i in range(len(outside)))
    assert M.stripe_phase(phase, edges[1:2]) == phase[-1, -1] and M.stripe_phase(phase, edges[:1]) == phase[0, 0]
    # findCentralStripe's rows: y = row + 0.5, so the last row (h - 0.5) is outside, as in the reference
    stripe = np.stack([np.full(h, 4.25), np.arange(0.5, h, 1)], axis=1)
    want = map_coordinates(phase, (stripe[:, 1], stripe[:, 0]), order=1)
    assert want[-1] == 0.0 and abs(M.stripe_phase(phase, stripe) - np.mean(want)) <= tol
    view = np.zeros((h, 2 * w))[:, ::2]
    view[:] = phase
    assert ss.active.ftpStripePhase(view, stripe) == M.stripe_phase(phase, stripe)


@pytest.mark.parametrize("dist", ["none", "d5", "d8", "d12"])
def test_mapping_cloud_equals_the_blas_triangulate(dist):
    """1e-12 relative: _stereo_ftp_ref.triangulate goes through BLAS .dot; a wrong row of F or a lost + 0.5 is off by far more"""
    rig = C.rig_params(res1=(160, 48), dist=dist)
    rig["T"] = [150.0, 10.0, 60.0]
    rg = S.Rig(rig, 12.0, 1280)
    g, F = M.mapping_geometry(rig, 12.0)
    h, w, x0, y0 = 7, 11, 30, 9
    yy, xx = np.mgrid[0:h, 0:w]
    phase = 0.31 * xx - 0.02 * yy + 35.0 + 0.2 * np.sin(xx * 0.7 + yy)
    theta = 33.5
    got = M.mapping_cloud(g, F, phase, theta, rg.peak, x0, y0)
    cam = np.mgrid[0:w, 0:h].T.reshape(-1, 2).astype(np.float64) + 0.5                           # active.py:1444-1445
    p_x = ((phase - theta).reshape(-1, 1)) / (2 * np.pi * rg.fp) + rg.peak + 0.5
    want = _triangulate_px(rg, cam, p_x.ravel(), (x0, y0, w, h)).reshape(h, w, 3)
    assert np.isfinite(want).all() and 500 < want[..., 2].min() and want[..., 2].max() < 2000
    assert float(C.rel_err(got, want).max()) <= 1e-12
    for wrong in (M.mapping_cloud(g, F, phase, theta, rg.peak - 0.5, x0, y0), M.mapping_cloud(g, np.roll(F, 3), phase, theta, rg.peak, x0, y0)):
        assert not float(C.rel_err(wrong, want).max()) <= 1e-6                                       # far off, or NaN


def _triangulate_px(rg, cam, p_x, roi):
    """_stereo_ftp_ref.triangulate with one projector column per point (it broadcasts a scalar)"""
    out = np.empty((cam.shape[0], 3))
    for i in range(cam.shape[0]):
        out[i] = S.triangulate(rg, cam[i:i + 1], float(p_x[i]), roi)[0]
    return out


def test_golden_cases_are_what_the_generator_makes():
    """the inputs' condition, checked here on the CPU: |ghat| >= 0.01 of its row maximum everywhere, numpy's error as recorded"""
    import sys
    sys.path.insert(0, M.GOLDEN)
    import make_golden_ftp_mapping as gen
    meta, z = M.load()
    assert sorted(meta["carrier"]) == sorted(gen.CARRIER) and sorted(meta["cloud"]) == sorted(gen.SCENES)
    for name, c in meta["carrier"].items():
        img, fc, rf = gen.make_carrier(name)
        assert _same(img, z[name + "__img"]) and _same(fc, z[name + "__fc"]) and rf == c["radius_factor"]
        truth, ratio = M.carrier_truth_longdouble(img, fc, rf)
        assert ratio.min() >= meta["min_ratio"] == 0.01 and ratio.min() == c["min_ratio"]
        if c["stored"]:
            assert _same(truth, z[name + "__truth"])
        numpy_err = float(P.wrap_err(M.carrier_phase_numpy(img, fc, rf), truth).max())
        assert c["tol"] == 16 * max(c["numpy_err"], np.pi * 2.0 ** -52) and numpy_err <= c["tol"]
    bins = {n: [b - a + 1 for a, b in zip(c["slo"], c["shi"])] for n, c in meta["carrier"].items()}
    assert bins["bins_128"] == [128, 128] and bins["bins_129"] == [129, 129] and bins["w257_all_bins"] == [257, 257]
    assert bins["empty_middle_row"][1] == 0 and bins["w2_both_bins"] == [2] and meta["carrier"]["w2_both_bins"]["slo"] == [-1]
    assert meta["carrier"]["w64_edges_on_bins"]["slo"] == [4] * 4 and meta["carrier"]["w64_edges_on_bins"]["shi"] == [12] * 4
    for name, c in meta["cloud"].items():
        assert c["unwrap_diff"] < 1e-9 and c["tol"] == 16 * max(c["numpy_err"], 2.0 ** -52)
    assert meta["cloud"]["roi"]["roi"][:2] != [0, 0] and any(meta["cloud"]["roi_camera_dist"]["rig"]["distCoeffs1"])


# ------------------------------------------------------------------------------------------------ the classes on a library stub
class Stub:
    """stands in for _native.run: records (name, scalar arguments), checks the sources against the numpy pipeline's stages and
    answers with that pipeline's next stage"""

    def __init__(self, want):
        self.want, self.calls = want, []

    def __call__(self, name, sources, shape, args, invalid=(), dtype=np.float64):
        ptrs = [0] * (len(sources) + 1)
        a = args(*ptrs)
        self.calls.append((name, a))
        w = self.want
        if name == "ssamd_stripe_centroids":
            assert np.array_equal(sources[0], w["undistorted"])
            return S.stripe_centroids(sources[0], "r", 0.5)
        if name == "ssamd_ftp_reference":
            g = np.ctypeslib.as_array((ctypes.c_double * 68).from_address(a[7]))
            assert _same(g, w["geom"])
            return w["ref"].copy()
        fmin = np.ctypeslib.as_array((ctypes.c_double * shape[0]).from_address(a[-5]))
        fmax = np.ctypeslib.as_array((ctypes.c_double * shape[0]).from_address(a[-4]))
        lo, hi = P.band(w["fc"], 0.5, shape[0])
        assert _same(fmin, lo) and _same(fmax, hi)
        if name == "ssamd_ftp_phase":
            assert np.array_equal(sources[0], w["undistorted"]) and np.array_equal(sources[1], w["ref"]) and a[-3] == 0
            return w["phase"].copy()
        if name == "ssamd_ftp_carrier_phase":
            out = M.carrier_phase_numpy(sources[0], w["fc"], 0.5)
            return M.unwrap2d(out) if a[-3] == 2 else out
        if name == "ssamd_ftp_mapping_cloud":
            raise AssertionError("handled by MappingStub")
        raise AssertionError(name)


class MappingStub(Stub):
    def __call__(self, name, sources, shape, args, invalid=(), dtype=np.float64):
        if name != "ssamd_ftp_mapping_cloud":
            return super().__call__(name, sources, shape, args, invalid, dtype)
        a = args(0, 0)
        self.calls.append((name, a))
        g = np.ctypeslib.as_array(a[5], (68,)).copy()
        F = np.ctypeslib.as_array(a[6], (9,)).copy()
        return M.mapping_cloud(g, F, sources[0], a[7], a[8], a[3], a[4])


@pytest.mark.parametrize("name", ["full", "roi", "roi_camera_dist"])
def test_get_cloud_on_a_stub_is_the_numpy_pipeline(ss, monkeypatch, name):
    meta, z = M.load()
    c = meta["cloud"][name]
    fringe = S.build_fringe(meta["period"], stripeColor="r")
    frame = np.array(z["cloud_" + name + "__frame"])
    roi = None if c["roi"] is None else tuple(c["roi"])
    want = M.pipeline_mapping(c["rig"], fringe, meta["period"], frame, roi)
    assert want["theta_shift"] == c["theta_shift"]
    stub = MappingStub(want)
    monkeypatch.setattr(ss.active._native, "run", stub)
    sf = ss.active.StereoFTP_Mapping(C.make_rig(ss, c["rig"]), fringe, meta["period"])
    got = sf.getCloud(frame, 0.5, roi)
    assert [n for n, _ in stub.calls] == ["ssamd_stripe_centroids", "ssamd_ftp_carrier_phase", "ssamd_ftp_mapping_cloud"]
    x0, y0, w, h = roi or (0, 0) + tuple(c["rig"]["res1"])
    carrier, cloud = stub.calls[1][1], stub.calls[2][1]
    assert carrier[1:4] == (3, h, w) and carrier[-3:-1] == (2, 1.0)                              # BGR cut, unwrap="numpy"
    assert cloud[1:5] == (h, w, x0, y0) and cloud[7] == want["theta_shift"] and cloud[8] == want["peak"] == sf.stripeCentralPeak
    assert _same(np.ctypeslib.as_array(cloud[5], (68,)), want["geom"]) and _same(np.ctypeslib.as_array(cloud[6], (9,)), want["F"])
    assert _same(got, want["cloud"])
    # an unwrapping method receives the wrapped map
    stub.calls.clear()
    seen = []
    sf.getCloud(frame, 0.5, roi, unwrappingMethod=lambda p: (seen.append(p), M.unwrap2d(p))[1])
    assert stub.calls[1][1][-3] == 0 and len(seen) == 1 and _same(seen[0], want["wrapped"])


@pytest.mark.parametrize("name", ["full", "roi_camera_dist"])
def test_get_phase_on_a_stub_is_the_numpy_pipeline(ss, monkeypatch, name):
    meta, z = M.load()
    c = meta["cloud"][name]
    fringe = S.build_fringe(meta["period"], stripeColor="r")
    frame = np.array(z["cloud_" + name + "__frame"])
    roi = None if c["roi"] is None else tuple(c["roi"])
    want = M.pipeline_phase_only(c["rig"], fringe, meta["period"], frame, roi)
    stub = Stub(want)
    monkeypatch.setattr(ss.active._native, "run", stub)
    sf = ss.active.StereoFTP_PhaseOnly(C.make_rig(ss, c["rig"]), fringe, meta["period"])
    got = sf.getPhase(frame, 0.5, roi)                                                           # roi=None works
    assert [n for n, _ in stub.calls] == ["ssamd_stripe_centroids", "ssamd_ftp_reference", "ssamd_ftp_phase", "ssamd_ftp_carrier_phase",
                                          "ssamd_ftp_carrier_phase"]
    assert stub.calls[3][1][1] == 3 and stub.calls[4][1][1] == 1 and stub.calls[3][1][-3] == stub.calls[4][1][-3] == 0
    assert len(got) == 3 and _same(got[0], want["phase"]) and _same(got[1], want["phase_obj"]) and _same(got[2], want["phase_ref"])
    assert want["z_plane"] == np.min(want["world"][:, 2]) and np.abs(got[0]).max() <= np.pi
    if any(c["rig"]["distCoeffs1"]):
        assert not _same(want["stripe_cam"], want["stripe"])                                      # the second undistortion moves it


def test_no_stripe_is_a_value_error(ss, monkeypatch):
    rig = C.make_rig(ss, C.rig_params(res1=(160, 48)))
    fringe = S.build_fringe(12.0, stripeColor="r")
    monkeypatch.setattr(ss.active._native, "run", lambda *a, **k: np.full(48, np.nan))
    frame = np.zeros((48, 160, 3), np.uint8)
    with pytest.raises(ValueError, match="Central stripe not found in image!"):
        ss.active.StereoFTP_PhaseOnly(rig, fringe, 12.0).getPhase(frame)
    with pytest.raises(ValueError, match="Central stripe not found in image!"):
        ss.active.StereoFTP_Mapping(rig, fringe, 12.0).getCloud(frame)
