"""GPU: the front end of ss.active.StereoFTP -- ftpReference (ftp_reference_kernel) and findCentralStripe
(stripe_centroid_kernel) against the numpy restatements of tests/_stereo_ftp_ref.py, every byte / bit equal, from host arrays
and device tensors; StereoFTP.getCloud against the chain of public functions it composes (bitwise) and against the numpy
pipeline (integer and host parts bitwise, the cloud within the tolerance tests/golden/make_golden_stereo_ftp.py measured on
numpy alone)."""
import numpy as np
import pytest

import _ftp_cloud_ref as C
import _stereo_ftp_ref as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available()
    import simplestereo_amd
    return simplestereo_amd


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


_REF = {}


def _reference_case(ss, name):
    """-> (case, gray fringe, packed geometry, the restatement's image); computed once and shared, read-only"""
    if name not in _REF:
        c = S.load_cases("reference")[name]
        fringe = S.case_fringe(c)
        g = np.array(c["geom"]) if "geom" in c else C.geometry(c["rig"], c["z_plane"], c["period"])[0]
        want = S.reference_image(fringe, g, *c["roi"])
        want.setflags(write=False)
        fringe.setflags(write=False)
        _REF[name] = (c, fringe, ss.active.FtpGeometry(g, tuple(c["roi"]), 1 / c["period"]), want)
    return _REF[name]


# ------------------------------------------------------------------------------------------------ ftpReference
@pytest.mark.parametrize("name", ["r3x130", "r5x257_roi", "dist_none", "dist_d5", "dist_d8", "dist_d12", "fringe_7x64", "fringe_1x1",
                                  "tall_65537x2", "nonfinite"])
def test_reference_image_equals_the_restatement_host_and_device(ss, name):
    import torch
    c, fringe, G, want = _reference_case(ss, name)
    host = ss.active.ftpReference(np.array(fringe), G)
    assert host.dtype == np.uint8 and host.shape == want.shape
    print("%s: %d of %d bytes differ; %d nonzero" % (name, np.count_nonzero(host != want), want.size, np.count_nonzero(want)))
    assert np.array_equal(host, want)
    dev = ss.active.ftpReference(torch.from_numpy(np.array(fringe)).cuda(), G)
    assert dev.is_cuda and dev.dtype == torch.uint8 and dev.is_contiguous()
    assert np.array_equal(dev.cpu().numpy(), host)
    if name == "nonfinite":
        y, x = c["pixel"]
        assert host[y, x] == 0
    else:
        assert want.any()
    if name == "fringe_7x64":                                  # taps straddle all four borders, some pixels fall wholly outside
        mx, my = S.projector_map(G.geom, *c["roi"])
        assert mx.min() < -3 and mx.max() > 66 and my.min() < -3 and my.max() > 9
        for edge in (mx < 1, mx > 62, my < 1, my > 5):
            assert want[edge].any()
        assert not want[(mx < -3) | (my < -3) | (mx > 66) | (my > 9)].any()


def test_reference_image_uses_every_entry_of_the_table(ss):
    """A geometry whose map is affine, x = u / 32 + 3, y = v / 32 + 2 (exact in fp64 and float32): 128 x 96 pixels walk through
    every pair of fractions on four by three cells of a random fringe -- the table built on the host in C++ is the numpy one"""
    g = np.ones(C.NGEOM)
    g[0:9] = [1 / 32, 0, 3, 0, 1 / 32, 2, 0, 0, 1]             # M
    g[9:12] = 0                                                # T
    g[12:16] = [1, 1, 0, 0]                                    # fx, fy, cx, cy
    g[16:28] = 0                                               # no distortion
    fringe = np.random.default_rng(3).integers(0, 256, (6, 8), dtype=np.uint8)
    mx, my = S.projector_map(g, 0, 0, 128, 96)
    q, r = np.rint(mx.astype(np.float64) * 32).astype(int), np.rint(my.astype(np.float64) * 32).astype(int)
    assert len(set(zip((r & 31).ravel().tolist(), (q & 31).ravel().tolist()))) == 1024
    want = S.remap_cubic(fringe, mx, my)
    got = ss.active.ftpReference(fringe, ss.active.FtpGeometry(g, (0, 0, 128, 96), 1 / 12.0))
    assert np.array_equal(got, want) and len(np.unique(want)) > 100


def test_reference_image_from_the_rig_and_from_bgr(ss):
    """the public path: the geometry packed from the StereoRig, a BGR fringe reduced by the channel maximum"""
    c, fringe, G, want = _reference_case(ss, "r5x257_roi")
    bgr = S.build_fringe(c["period"], stripeColor="r")
    got = ss.active.ftpReference(bgr, C.make_rig(ss, c["rig"]), c["z_plane"], tuple(c["roi"]))
    assert np.array_equal(got, want)
    assert np.array_equal(ss.active.ftpReference(bgr, C.make_rig(ss, c["rig"]), c["z_plane"], tuple(c["roi"]), period=12.0), want)


def test_reference_image_non_contiguous_fringe_and_non_default_stream(ss):
    import torch
    c, fringe, G, want = _reference_case(ss, "r3x130")
    big = torch.zeros((2 * fringe.shape[0], fringe.shape[1] + 7), dtype=torch.uint8, device="cuda")
    big[::2, 3:3 + fringe.shape[1]] = torch.from_numpy(np.array(fringe)).cuda()
    view = big[::2, 3:3 + fringe.shape[1]]
    assert not view.is_contiguous()
    assert np.array_equal(ss.active.ftpReference(view, G).cpu().numpy(), want)
    host = np.zeros((2 * fringe.shape[0], fringe.shape[1] + 7), np.uint8)
    host[::2, 3:3 + fringe.shape[1]] = fringe
    assert np.array_equal(ss.active.ftpReference(host[::2, 3:3 + fringe.shape[1]], G), want)
    src = torch.from_numpy(np.array(fringe)).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fr = torch.zeros_like(src)
        fr.copy_(src + 0)                                      # filled on s just before the call
        out = ss.active.ftpReference(fr, G)
        total = out.sum()                                      # consumed on s without a synchronisation in between
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), want) and int(total.cpu()) == int(want.sum(dtype=np.int64))


def test_profile_slots(ss):
    from simplestereo_amd import _native
    c, fringe, G, want = _reference_case(ss, "dist_d5")
    lib = _native.lib()
    assert b"ftp_reference_kernel" in lib.ssamd_kernel_name(_native.K_REMAP)
    img = np.zeros((4, 9, 3), np.uint8)
    img[:, 4, 2] = 200
    lib.ssamd_profile_enable(1)
    try:
        lib.ssamd_profile_reset()
        ss.active.ftpReference(np.array(fringe), G)
        ss.active.findCentralStripe(img)
        ms, n = _native.profile_read()
        assert n[_native.K_REMAP] == 1 and n[_native.K_FTP] == 1 and sum(n) == 2 and ms[_native.K_REMAP] > 0
    finally:
        lib.ssamd_profile_enable(0)


# ------------------------------------------------------------------------------------------------ findCentralStripe
def _stripe_image(h, w, seed):
    """random BGR bytes with a brighter red stripe that wanders over the rows; rows 1 and h - 2 (if any) hold no red at all"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for y in range(h):
        x = int((w - 1) * (0.3 + 0.4 * y / max(h - 1, 1)))
        img[y, max(x - 2, 0):x + 3, 2] = 255
    if h > 3:
        img[1, :, 2] = 0
        img[h - 2, :, 2] = 0
    return img


@pytest.mark.parametrize("w", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("color", ["r", "g", "b"])
def test_stripe_centroids_equal_numpy(ss, w, color):
    import torch
    from simplestereo_amd import _native
    img = _stripe_image(9, w, seed=w)
    ch = S.CHANNEL[color]
    if color != "r":
        img[:, :, [2, ch]] = img[:, :, [ch, 2]]
    for sensitivity in (0, 0.5, 128 / 255, 1):
        want = S.stripe_centroids(img, color, sensitivity)
        thr = int(np.ceil(255 * float(sensitivity)))
        host = _native.run("ssamd_stripe_centroids", (img,), (9,), lambda s, o: (s, 9, w, ch, thr, o))
        dev = _native.run("ssamd_stripe_centroids", (torch.from_numpy(img).cuda(),), (9,), lambda s, o: (s, 9, w, ch, thr, o)).cpu().numpy()
        for got in (host, dev):
            assert np.array_equal(np.isnan(got), np.isnan(want)), (w, color, sensitivity)
            ok = ~np.isnan(want)
            assert _same(got[ok], want[ok]), (w, color, sensitivity)
        if sensitivity in (0.5, 1) and w > 1:
            assert np.isnan(want[[1, 7]]).all() and not np.isnan(want[[0, 4, 8]]).any()
        # the public function: the reference's result, with its fill
        stripe = ss.active.findCentralStripe(img, color, sensitivity)
        ref = S.find_central_stripe(img, color, sensitivity)
        assert stripe.shape == (9, 2) and _same(stripe, ref)
        assert _same(ss.active.findCentralStripe(torch.from_numpy(img).cuda(), color, sensitivity), ref)


def test_stripe_thresholds_that_land_on_an_integer(ss):
    """value < 255 * sensitivity with the product exactly an integer: the value equal to it is kept, one below is not"""
    for t in (1, 51, 128, 254, 255):
        sens = t / 255
        img = np.zeros((3, 40, 3), np.uint8)
        img[0, 10, 2], img[0, 30, 2] = t, t - 1                 # only column 10 survives: centroid 10
        img[1, 10, 2], img[1, 30, 2] = t, t                     # both: 20
        img[2, 5, 2] = t - 1                                    # none: NaN (filled by extrapolation)
        want = S.find_central_stripe(img, "r", sens)
        got = ss.active.findCentralStripe(img, "r", sens)
        assert _same(got, want), t
        assert np.array_equal(np.isnan(S.stripe_centroids(img, "r", sens)), [False, False, True])


def test_stripe_wide_rows_need_64_bit_sums(ss):
    import torch
    img = np.full((3, 8192, 3), 255, np.uint8)
    img[1, :, 2] = 0
    want = S.find_central_stripe(img, "r", 0.5)
    assert 255 * 8191 * 8192 // 2 > 2 ** 32 and want[0, 0] == 4095.5
    assert _same(ss.active.findCentralStripe(img, "r", 0.5), want)
    assert _same(ss.active.findCentralStripe(torch.from_numpy(img).cuda(), "r", 0.5), want)


def test_no_stripe_at_all_is_none(ss):
    import torch
    img = _stripe_image(6, 50, seed=1)
    img[:, :, 2] = 100
    assert ss.active.findCentralStripe(img, "r", 0.5) is None
    assert ss.active.findCentralStripe(torch.from_numpy(img).cuda(), "r", 0.5) is None
    assert ss.active.findCentralStripe(img, "r", 0.3) is not None


# ------------------------------------------------------------------------------------------------ StereoFTP.getCloud
_CLOUD = {}


def _cloud_case(ss, name):
    """-> (case, StereoFTP, frame, the numpy pipeline's stages, getCloud of the host frame); computed once and shared"""
    if name not in _CLOUD:
        c = S.load_cases("cloud")[name]
        fringe = S.build_fringe(c["period"], stripeColor="r")
        sf = ss.active.StereoFTP(C.make_rig(ss, c["rig"]), fringe, c["period"])
        frame = np.array(c["frame"])
        roi = None if c["roi"] is None else tuple(c["roi"])
        want = S.pipeline(c["rig"], fringe, c["period"], frame, roi, c["radius_factor"])
        host = sf.getCloud(frame, c["radius_factor"], roi)
        host.setflags(write=False)
        _CLOUD[name] = (c, sf, frame, roi, want, host)
    return _CLOUD[name]


@pytest.mark.parametrize("name", ["full", "roi", "roi_camera_dist"])
def test_get_cloud_equals_the_chain_of_public_functions(ss, name):
    import torch
    a = ss.active
    c, sf, frame, roi, want, host = _cloud_case(ss, name)
    x0, y0, w, h = roi or (0, 0) + tuple(c["rig"]["res1"])
    assert host.shape == (h, w, 3) and host.dtype == np.float64 and isinstance(host, np.ndarray)
    dev = sf.getCloud(torch.from_numpy(frame).cuda(), c["radius_factor"], roi)
    assert dev.is_cuda and dev.dtype == torch.float64
    assert _same(dev.cpu().numpy(), host)                      # host frame and device frame: the same bits
    # the chain getCloud composes, on device tensors
    t = torch.from_numpy(frame).cuda()
    cut = sf._undistort(t)[y0:y0 + h, x0:x0 + w]
    assert np.array_equal(cut.cpu().numpy(), want["undistorted"])
    stripe = a.findCentralStripe(cut, sf.stripeColor, sf.stripeSensitivity)
    idx = np.ceil(stripe - 0.5).astype(np.int64)
    world = sf._triangulate(stripe, sf.stripeCentralPeak, (x0, y0, w, h))
    z_plane, fc = np.mean(world[:, 2]), sf._calculateCameraFrequency(world)
    ref = a.ftpReference(torch.from_numpy(sf.fringe).cuda(), sf.stereoRig, z_plane, roi)
    phase = a.ftpPhase(cut, ref, fc, c["radius_factor"], unwrap="numpy")
    k = a.ftpFringeOrder(phase, idx, sf.stereoRig, z_plane, c["period"], sf.stripeCentralPeak, roi)
    chain = a.ftpCloud(phase, sf.stereoRig, z_plane, c["period"], k, roi)
    assert _same(chain.cpu().numpy(), host)


def test_get_cloud_accepts_an_unwrapping_method(ss):
    import torch
    c, sf, frame, roi, want, host = _cloud_case(ss, "roi")
    got = sf.getCloud(frame, c["radius_factor"], roi, unwrappingMethod=ss.unwrapping.infiniteImpulseResponse)
    assert got.shape == host.shape and np.isfinite(got).all()
    dev = sf.getCloud(torch.from_numpy(frame).cuda(), c["radius_factor"], roi, unwrappingMethod=ss.unwrapping.infiniteImpulseResponse)
    assert _same(dev.cpu().numpy(), got)
    seen = []
    sf.getCloud(frame, c["radius_factor"], roi, unwrappingMethod=lambda p: (seen.append(p), ss.unwrapping.unwrap2D(p))[1])
    assert len(seen) == 1 and seen[0].shape == host.shape[:2] and np.abs(seen[0]).max() <= np.pi        # the wrapped phase


@pytest.mark.parametrize("name", ["full", "roi", "roi_camera_dist"])
def test_get_cloud_against_the_numpy_pipeline(ss, name):
    """The integer and host parts (reference image, stripe, z_plane, fc, band, k) are those of the numpy pipeline bit for bit;
    the cloud is within the case's tolerance of it -- 16 x the distance between that pipeline and the same pipeline fed the
    np.longdouble phase, floored at 16 x 2^-52, measured by the generator on numpy alone -- over the pixels the fixture keeps."""
    import torch
    a = ss.active
    c, sf, frame, roi, want, host = _cloud_case(ss, name)
    x0, y0, w, h = roi or (0, 0) + tuple(c["rig"]["res1"])
    cut, box, stripe, idx = sf._frame(torch.from_numpy(frame).cuda(), roi)
    assert box == (x0, y0, w, h) and np.array_equal(cut.cpu().numpy(), want["undistorted"])
    assert _same(stripe, want["stripe"]) and np.array_equal(idx, want["stripe_indexes"])
    world = sf._triangulate(stripe, sf.stripeCentralPeak, box)
    z_plane, fc = np.mean(world[:, 2]), sf._calculateCameraFrequency(world)
    assert z_plane == want["z_plane"] == c["z_plane"] and _same(fc, want["fc"])
    fmin, fmax = a._band(fc, c["radius_factor"], h)
    assert _same(fmin, want["fmin"]) and _same(fmax, want["fmax"])
    G = a.ftpGeometry(sf.stereoRig, z_plane, c["period"], roi)
    ref = a.ftpReference(sf.fringe, G)
    assert np.array_equal(ref, want["ref"])
    phase = a.ftpPhase(np.ascontiguousarray(cut.cpu().numpy()), ref, fc, c["radius_factor"], unwrap="numpy")
    assert a.ftpFringeOrder(phase, idx, G, stripeCentralPeak=sf.stripeCentralPeak) == want["k"] == c["k"]
    keep = np.unpackbits(np.array(c["keep"]))[:h * w].reshape(h, w).astype(bool)
    assert keep.mean() >= 0.9 and np.isfinite(host[keep]).all()
    err = float(C.rel_err(host, want["cloud"].astype(np.longdouble))[keep].max())
    print("%s: getCloud vs the numpy pipeline %.3e, tol %.3e (numpy's own distance to the longdouble phase %.3e), kept %.3f"
          % (name, err, c["tol"], c["numpy_err"], keep.mean()))
    assert err <= c["tol"]
