"""GPU: FTP without a reference plane.  ss.active.ftpCarrierPhase (ftp_carrier_kernel) against the extended-precision truth of
tests/golden/ftp_mapping_cases.* within the case's recorded tolerance 16 * max(numpy's own error, pi 2^-52);
ss.active.ftpMappingCloud (ftp_mapping_cloud_kernel) bit for bit against tests/_ftp_mapping_ref.mapping_cloud;
StereoFTP_Mapping.getCloud and StereoFTP_PhaseOnly.getPhase against the chain of the public calls (bit for bit) and the numpy
pipeline (within the recorded tolerance) -- on host arrays and on device tensors."""
import numpy as np
import pytest

import _ftp_cloud_ref as C
import _ftp_mapping_ref as M
import _ftp_ref as P
import _stereo_ftp_ref as S

pytestmark = pytest.mark.gpu

META, DATA = M.load()
CARRIER = META["carrier"]


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available()
    import simplestereo_amd
    return simplestereo_amd


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ ftpCarrierPhase
_TRUTH = {}


def _carrier(name):
    """-> (img, fc, radius_factor, truth); the truth of the wide cases is computed here, once"""
    if name not in _TRUTH:
        img, fc, rf = DATA[name + "__img"], DATA[name + "__fc"], CARRIER[name]["radius_factor"]
        if CARRIER[name]["stored"]:
            truth = DATA[name + "__truth"]
        else:
            truth, ratio = M.carrier_truth_longdouble(img, fc, rf)
            assert ratio.min() >= META["min_ratio"]
            truth.setflags(write=False)
        _TRUTH[name] = (img, fc, rf, truth)
    return _TRUTH[name]


def _check(name, got, truth):
    assert got.dtype == np.float64 and got.shape == truth.shape
    err = P.wrap_err(got, truth)
    worst = float(err.max())
    print("%s: worst angle error %.3e (numpy %.3e, tolerance %.3e)" % (name, worst, CARRIER[name]["numpy_err"], CARRIER[name]["tol"]))
    assert np.isfinite(got).all()
    assert worst <= CARRIER[name]["tol"], (name, worst, CARRIER[name]["tol"], np.unravel_index(int(err.argmax()), err.shape))


@pytest.mark.parametrize("name", sorted(CARRIER))
def test_carrier_phase_against_truth_host_and_device(ss, name):
    import torch
    img, fc, rf, truth = _carrier(name)
    assert list(img.shape[:2]) == CARRIER[name]["shape"] and (img.ndim == 3) == (CARRIER[name]["channels"] == 3)
    host = ss.active.ftpCarrierPhase(img, fc, rf)
    _check(name, host, truth)
    dev = ss.active.ftpCarrierPhase(torch.from_numpy(img).cuda(), fc, rf)
    assert dev.is_cuda and dev.dtype == torch.float64
    assert _same(dev.cpu().numpy(), host)


def test_carrier_bgr_is_the_channel_maximum(ss):
    img, fc, rf, _ = _carrier("bgr")
    assert (img.argmax(axis=2) != 0).any()
    assert _same(ss.active.ftpCarrierPhase(img, fc, rf), ss.active.ftpCarrierPhase(P.gray(img), fc, rf))


def test_carrier_empty_band_row_is_zero_and_leaves_its_neighbours(ss):
    img, fc, rf, _ = _carrier("empty_middle_row")
    c = CARRIER["empty_middle_row"]
    assert c["slo"][1] > c["shi"][1] and c["slo"][0] <= c["shi"][0]
    got = ss.active.ftpCarrierPhase(img, fc, rf)
    assert np.array_equal(got[1], np.zeros(got.shape[1])) and not np.signbit(got[1]).any()
    for y in (0, 2):                                   # each neighbour alone gives the same row, bit for bit
        alone = ss.active.ftpCarrierPhase(img[y:y + 1], fc[y:y + 1], rf)
        assert _same(alone[0], got[y]) and np.abs(got[y]).max() > 1e-3
    z = ss.active.ftpCarrierPhase(img, 0.0019, rf)     # every row empty
    assert np.array_equal(z, np.zeros_like(z))


def test_carrier_is_half_of_the_pair_kernel(ss):
    """angle(ghat) - angle(g0hat) is angle(ghat * conj(g0hat)) up to rounding: the one-image kernel and the pair kernel agree"""
    img, fc, rf, _ = _carrier("w257")
    other = np.ascontiguousarray(np.roll(img, 3, axis=1))
    pair = ss.active.ftpPhase(img, other, fc, rf)
    diff = ss.active.ftpCarrierPhase(img, fc, rf) - ss.active.ftpCarrierPhase(other, fc, rf)
    assert P.wrap_err(pair, diff).max() < 1e-12


def test_carrier_width_limit(ss):
    from simplestereo_amd import _native
    w = ss.active.MAX_WIDTH + 1
    img = np.zeros((2, w), dtype=np.uint8)
    with pytest.raises(ValueError):
        ss.active.ftpCarrierPhase(img, 0.05)
    f, out = np.full(2, 0.05), np.zeros((2, w))
    rc = _native.lib().ssamd_ftp_carrier_phase(img.ctypes.data, 1, 2, w, f.ctypes.data, f.ctypes.data, 0, 1.0, out.ctypes.data, -1)
    assert rc == -5 and b"8192" in _native.lib().ssamd_last_error()


@pytest.mark.parametrize("name", ["w257", "w63_fc_per_row", "empty_middle_row", "w1", "cpt2_w1025"])
def test_carrier_unwrap_is_the_unwrapper_on_the_wrapped_map(ss, name):
    import torch
    u = ss.unwrapping
    img, fc, rf, _ = _carrier(name)
    wrapped = ss.active.ftpCarrierPhase(img, fc, rf)
    t = torch.from_numpy(img).cuda()
    want = u.unwrap2D(wrapped)
    assert _same(want, np.unwrap(np.unwrap(wrapped, axis=1), axis=0))
    assert _same(ss.active.ftpCarrierPhase(img, fc, rf, unwrap="numpy"), want)
    assert _same(ss.active.ftpCarrierPhase(t, fc, rf, unwrap="numpy").cpu().numpy(), want)
    for tau in (1, 0.8):
        want = u.infiniteImpulseResponse(wrapped, tau)
        assert _same(ss.active.ftpCarrierPhase(img, fc, rf, unwrap="iir", tau=tau), want)
        assert _same(ss.active.ftpCarrierPhase(t, fc, rf, unwrap="iir", tau=tau).cpu().numpy(), want)
    assert _same(ss.active.ftpCarrierPhase(img, fc, rf), wrapped)              # unchanged by the calls that share its scratch


def test_carrier_non_contiguous_view_and_non_default_stream(ss):
    import torch
    img, fc, rf, _ = _carrier("bgr")
    want = ss.active.ftpCarrierPhase(img, fc, rf)
    wide = np.zeros((img.shape[0], img.shape[1] + 5, 3), dtype=np.uint8)
    wide[:, 2:-3] = img
    assert _same(ss.active.ftpCarrierPhase(wide[:, 2:-3], fc, rf), want)
    t = torch.from_numpy(wide).cuda()[:, 2:-3]
    assert not t.is_contiguous()
    assert _same(ss.active.ftpCarrierPhase(t, fc, rf).cpu().numpy(), want)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        t2 = (t.to(torch.int32) + 0).to(torch.uint8)    # produced on s just before the call: the call must be ordered behind it
        out = ss.active.ftpCarrierPhase(t2, fc, rf)
        unw = ss.active.ftpCarrierPhase(t2, fc, rf, unwrap="numpy")
        total = out.sum()                              # consumed on s without a synchronisation in between
    s.synchronize()
    assert _same(out.cpu().numpy(), want) and float(total.cpu()) == float(out.sum().cpu())
    assert _same(unw.cpu().numpy(), ss.unwrapping.unwrap2D(want))


def test_carrier_profile_slot(ss):
    from simplestereo_amd import _native
    lib = _native.lib()
    img, fc, rf, _ = _carrier("w257")
    lib.ssamd_profile_enable(1)
    lib.ssamd_profile_reset()
    try:
        ss.active.ftpCarrierPhase(img, fc, rf)
        ms, n = _native.profile_read()
        assert n[_native.K_FTP] == 1 and n[_native.K_REPROJECT] == 0
        ss.active.ftpMappingCloud(np.zeros((3, 5)), _rig(ss, "d5"), 12.0, 640.0, roi=(0, 0, 5, 3))
        ms, n = _native.profile_read()
        assert n[_native.K_FTP] == 1 and n[_native.K_REPROJECT] == 1
    finally:
        lib.ssamd_profile_enable(0)


# ------------------------------------------------------------------------------------------------ ftpMappingCloud
def _rig_params(dist, res1=(1280, 720), **kw):
    rig = C.rig_params(res1=res1, dist=dist, **kw)
    rig["T"] = [150.0, 10.0, 60.0]
    return rig


def _rig(ss, dist, res1=(1280, 720)):
    return C.make_rig(ss, _rig_params(dist, res1))


def _map_phase(h, w, seed=0):
    """an unwrapped one-image phase: the carrier's ramp (about 2 pi / 3.3 per pixel), a smooth hill and some noise"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return 1.9 * x + 0.01 * y + C.smooth_phase(h, w, 6.0, seed)


def _mapping_case(ss, params, phase, roi, theta, peak=636.0):
    """host and device results of ftpMappingCloud, checked bit for bit against the restatement; -> the restatement"""
    import torch
    g, F = M.mapping_geometry(params, 12.0)
    want = M.mapping_cloud(g, F, phase, theta, peak, roi[0], roi[1])
    rig = C.make_rig(ss, params)
    packed = ss.active.ftpMappingGeometry(rig, 12.0, roi)
    assert _same(packed.geom, g) and _same(packed.F, F)
    host = ss.active.ftpMappingCloud(phase, rig, 12.0, peak, theta, roi)
    assert host.shape == phase.shape + (3,) and host.dtype == np.float64
    assert _same(host, want)
    dev = ss.active.ftpMappingCloud(torch.from_numpy(phase).cuda(), packed, stripeCentralPeak=peak, theta_shift=theta)
    assert dev.is_cuda and _same(dev.cpu().numpy(), want)
    return want


@pytest.mark.parametrize("h,w,roi_xy", [(3, 130, (575, 300)), (5, 257, (501, 333)), (1, 1, (640, 360)), (3, 3, (0, 0))])
def test_mapping_cloud_equals_the_restatement(ss, h, w, roi_xy):
    phase = _map_phase(h, w, seed=h * w) + 1200.0
    want = _mapping_case(ss, _rig_params("d8"), phase, roi_xy + (w, h), theta=1210.5)
    assert np.isfinite(want).all()


@pytest.mark.parametrize("h,w", [(1, 1), (5, 1), (2, 64), (1, 129), (3, 43)])
def test_shared_frame_through_both_cloud_kernels(ss, h, w):
    """ftp_cloud_frame, the frame ftp_mapping_cloud_kernel and ftp_cloud_kernel share, on the same shapes and a roi origin that is
    not 0: a single pixel; every pair wrapping a row, with an odd tail; exactly one full round of a wave and no tail; a full round
    plus a round of one pixel; 129 pixels with wraps in the middle of a pair.  Host and device results equal the two numpy
    restatements bit for bit."""
    import torch
    params, roi = _rig_params("d8"), (571, 303, w, h)
    want = _mapping_case(ss, params, _map_phase(h, w, seed=h * w) + 1200.0, roi, theta=1210.5)
    assert np.isfinite(want).all()
    G = ss.active.ftpGeometry(C.make_rig(ss, params), 1000.0, 12.0, roi)
    phase = C.smooth_phase(h, w, 12.0, seed=h * w)
    want = C.cloud_from_geometry(G.geom, phase, 2.0, roi[0], roi[1])
    assert want.shape == (h, w, 3) and np.isfinite(want).all()
    assert _same(ss.active.ftpCloud(phase, G, k=2.0), want)
    dev = ss.active.ftpCloud(torch.from_numpy(phase).cuda(), G, k=2.0)
    assert dev.is_cuda and _same(dev.cpu().numpy(), want)


@pytest.mark.parametrize("dist", ["none", "d4", "d5", "d8", "d12"])
def test_mapping_cloud_distortion_models(ss, dist):
    phase = _map_phase(4, 66, seed=3) + 1100.0
    want = _mapping_case(ss, _rig_params(dist), phase, (560, 320, 66, 4), theta=1105.25)
    assert np.isfinite(want).all()
    if dist != "none":
        plain = M.mapping_cloud(*M.mapping_geometry(_rig_params("none"), 12.0), phase, 1105.25, 636.0, 560, 320)
        assert not _same(plain, want)


def test_mapping_cloud_tall_map(ss):
    """65537 rows of 2 pixels: rows are not a grid dimension"""
    params = C.rig_params(res1=(2, 65537), dist="d8", k1_fy=150000.0)
    params["T"] = [150.0, 10.0, 60.0]
    phase = C.tall_phase(65537, 2)
    want = _mapping_case(ss, params, phase, (0, 0, 2, 65537), theta=0.25)
    assert np.isfinite(want).all()


def test_mapping_cloud_rig_without_depth_offset(ss):
    """T[2] == 0: the epipole on the projector image is at infinity; ftpGeometry refuses such a rig, the mapping needs no epipole"""
    params = _rig_params("d5")
    params["T"] = [-200.0, 5.0, 0.0]
    with pytest.raises(ValueError, match="epipole"):
        ss.active.ftpGeometry(C.make_rig(ss, params), 1000.0, 12.0)
    phase = _map_phase(3, 130, seed=9) + 1200.0
    want = _mapping_case(ss, params, phase, (575, 300, 130, 3), theta=1201.0)
    assert np.isfinite(want).all()


def test_mapping_cloud_non_finite_phase(ss):
    import torch
    params, roi = _rig_params("d5"), (575, 300, 130, 3)
    phase = _map_phase(3, 130, seed=4) + 1200.0
    clean = M.mapping_cloud(*M.mapping_geometry(params, 12.0), phase, 1201.0, 636.0, roi[0], roi[1])
    phase[1, 64] = np.nan
    want = M.mapping_cloud(*M.mapping_geometry(params, 12.0), phase, 1201.0, 636.0, roi[0], roi[1])
    assert np.isnan(want[1, 64]).all()
    rig = C.make_rig(ss, params)
    for got in (ss.active.ftpMappingCloud(phase, rig, 12.0, 636.0, 1201.0, roi),
                ss.active.ftpMappingCloud(torch.from_numpy(phase).cuda(), rig, 12.0, 636.0, 1201.0, roi).cpu().numpy()):
        assert np.isnan(got[1, 64]).all()                                       # the NaN the formulas give (sign and payload apart)
        keep = np.ones((3, 130), bool)
        keep[1, 64] = False
        assert _same(got[keep], clean[keep])                                    # the neighbours untouched


def test_mapping_cloud_view_at_an_odd_offset_and_stream(ss):
    import torch
    params, roi = _rig_params("d5"), (575, 300, 129, 3)
    phase = _map_phase(3, 129, seed=5) + 1200.0
    g, F = M.mapping_geometry(params, 12.0)
    want = M.mapping_cloud(g, F, phase, 1201.0, 636.0, roi[0], roi[1])
    rig = C.make_rig(ss, params)
    flat = torch.zeros(3 * 129 + 1, dtype=torch.float64, device="cuda")
    flat[1:] = torch.from_numpy(phase).cuda().reshape(-1)
    view = flat[1:].reshape(3, 129)
    assert view.data_ptr() % 16 == 8 and view.is_contiguous()
    assert _same(ss.active.ftpMappingCloud(view, rig, 12.0, 636.0, 1201.0, roi).cpu().numpy(), want)
    cols = torch.from_numpy(np.ascontiguousarray(phase.T)).cuda().T
    assert not cols.is_contiguous()
    assert _same(ss.active.ftpMappingCloud(cols, rig, 12.0, 636.0, 1201.0, roi).cpu().numpy(), want)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        p2 = view + 0.0
        out = ss.active.ftpMappingCloud(p2, rig, 12.0, 636.0, 1201.0, roi)
    s.synchronize()
    assert _same(out.cpu().numpy(), want)
    # the library itself refuses a misaligned device buffer
    from simplestereo_amd import _native
    import ctypes
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))            # noqa: E731
    out = torch.empty((3, 129, 3), dtype=torch.float64, device="cuda")
    rc = _native.lib().ssamd_ftp_mapping_cloud_device(view.data_ptr(), 3, 129, 0, 0, dp(g), dp(F), 0.0, 0.0, out.data_ptr(), None)
    assert rc == -1 and b"16-byte" in _native.lib().ssamd_last_error()


def test_stripe_phase_of_a_device_map(ss):
    import torch
    rng = np.random.default_rng(8)
    phase = np.cumsum(rng.normal(0.6, 0.1, (9, 40)), axis=1)
    stripe = np.stack([rng.uniform(-1, 41, 9), np.arange(0.5, 9, 1)], axis=1)
    want = M.stripe_phase(phase, stripe)
    assert ss.active.ftpStripePhase(phase, stripe) == want
    assert ss.active.ftpStripePhase(torch.from_numpy(phase).cuda(), stripe) == want


# ------------------------------------------------------------------------------------------------ the classes
_SCENE = {}


def _scene(ss, name):
    """-> (case, fringe, frame, roi, numpy pipeline, StereoFTP_Mapping, its getCloud of the host frame); computed once"""
    if name not in _SCENE:
        c = META["cloud"][name]
        fringe = S.build_fringe(META["period"], stripeColor="r")
        frame = np.array(DATA["cloud_" + name + "__frame"])
        roi = None if c["roi"] is None else tuple(c["roi"])
        want = M.pipeline_mapping(c["rig"], fringe, META["period"], frame, roi, c["radius_factor"])
        sf = ss.active.StereoFTP_Mapping(C.make_rig(ss, c["rig"]), fringe, META["period"])
        host = sf.getCloud(frame, c["radius_factor"], roi)
        host.setflags(write=False)
        _SCENE[name] = (c, fringe, frame, roi, want, sf, host)
    return _SCENE[name]


@pytest.mark.parametrize("name", ["full", "roi", "roi_camera_dist"])
def test_get_cloud_host_device_chain_and_numpy_pipeline(ss, name):
    import torch
    a = ss.active
    c, fringe, frame, roi, want, sf, host = _scene(ss, name)
    x0, y0, w, h = roi or (0, 0) + tuple(c["rig"]["res1"])
    assert host.shape == (h, w, 3) and host.dtype == np.float64 and isinstance(host, np.ndarray)
    t = torch.from_numpy(frame).cuda()
    dev = sf.getCloud(t, c["radius_factor"], roi)
    assert dev.is_cuda and dev.dtype == torch.float64 and _same(dev.cpu().numpy(), host)        # host and device frame: the same bits
    # the chain of the public calls, on device tensors; its host inputs equal the numpy pipeline's bit for bit
    cut, box, stripe, _ = sf._frame(t, roi)
    assert box == (x0, y0, w, h) and np.array_equal(cut.cpu().numpy(), want["undistorted"]) and _same(stripe, want["stripe"])
    fc = sf._calculateCameraFrequency(sf._triangulate(stripe, sf.stripeCentralPeak, box))
    assert _same(fc, want["fc"]) and sf.stripeCentralPeak == want["peak"]
    phase = a.ftpCarrierPhase(cut, fc, c["radius_factor"], unwrap="numpy")
    theta = a.ftpStripePhase(phase, stripe)
    assert theta == M.stripe_phase(phase.cpu().numpy(), stripe)                                  # theta_shift from its inputs
    chain = a.ftpMappingCloud(phase, sf.stereoRig, META["period"], sf.stripeCentralPeak, theta, roi)
    assert _same(chain.cpu().numpy(), host)
    # the numpy pipeline: no 2 pi decision differs, and the cloud is within the recorded tolerance everywhere
    assert np.abs(phase.cpu().numpy() - want["phase"]).max() < 1e-9 and abs(theta - want["theta_shift"]) < 1e-9
    err = float(C.rel_err(host, want["cloud"].astype(np.longdouble)).max())
    print("%s: getCloud vs the numpy pipeline %.3e, tol %.3e (numpy's own distance to the longdouble phase %.3e)"
          % (name, err, c["tol"], c["numpy_err"]))
    assert np.isfinite(host).all() and err <= c["tol"]


def test_get_cloud_with_an_unwrapping_method(ss):
    import torch
    a = ss.active
    c, fringe, frame, roi, want, sf, host = _scene(ss, "roi")
    iir = ss.unwrapping.infiniteImpulseResponse
    got = sf.getCloud(frame, c["radius_factor"], roi, unwrappingMethod=iir)
    t = torch.from_numpy(frame).cuda()
    assert _same(sf.getCloud(t, c["radius_factor"], roi, unwrappingMethod=iir).cpu().numpy(), got)
    cut, box, stripe, _ = sf._frame(frame, roi)
    phase = iir(a.ftpCarrierPhase(cut, want["fc"], c["radius_factor"]))
    chain = a.ftpMappingCloud(phase, sf.stereoRig, META["period"], sf.stripeCentralPeak, a.ftpStripePhase(phase, stripe), roi)
    assert _same(chain, got) and np.isfinite(got).all()


@pytest.mark.parametrize("name", ["full", "roi_camera_dist"])
def test_get_phase_equals_the_public_calls_on_the_numpy_stages(ss, name):
    import torch
    a = ss.active
    c, fringe, frame, roi, _, _, _ = _scene(ss, name)
    want = M.pipeline_phase_only(c["rig"], fringe, META["period"], frame, roi, c["radius_factor"])
    po = a.StereoFTP_PhaseOnly(C.make_rig(ss, c["rig"]), fringe, META["period"])
    got = po.getPhase(frame, c["radius_factor"], roi)                                            # roi=None: the whole frame
    x0, y0, w, h = roi or (0, 0) + tuple(c["rig"]["res1"])
    cut, ref, fc = want["undistorted"], want["ref"], want["fc"]
    expect = (a.ftpPhase(cut, ref, fc, c["radius_factor"]), a.ftpCarrierPhase(cut, fc, c["radius_factor"]),
              a.ftpCarrierPhase(ref, fc, c["radius_factor"]))
    assert len(got) == 3
    for g, e, key in zip(got, expect, ("phase", "phase_obj", "phase_ref")):
        assert g.shape == (h, w) and _same(g, e) and np.abs(g).max() <= np.pi
    dev = po.getPhase(torch.from_numpy(frame).cuda(), c["radius_factor"], roi)
    for d, g in zip(dev, got):
        assert d.is_cuda and _same(d.cpu().numpy(), g)
