"""ss.active on the kernels against what the reference's OWN simplestereo/active.py computed: tests/golden/active_ref_cases.*,
recorded by tests/golden/make_golden_active_ref.py (the reference loaded from where it lies, cv2 answered by a stand-in made of
the numpy restatements).  Only tests/golden is read.  Every frame is at most 48 x 160 or 67 x 37.

The classes run on a host array and on a device tensor; the public chains run on the reference's recorded intermediate values.
Float results are held to the tolerance recorded per case (16 * max(numpy_err, 2^-52), numpy_err the reference's own distance
to itself on the np.longdouble phase), bytes and counts exactly.  With the fundamental matrix in float64 throughout, as before
the reference's float32 cross-product matrix was followed, the StereoFTP and StereoFTP_Mapping clouds of the classes were
1.22e-10 .. 1.30e-10 away; measured on an MI355X they are 7.9e-16 .. 1.4e-15 now (tolerances 5.4e-15 .. 1.6e-14)."""
import numpy as np
import pytest

import _active_ref as AR
import _ftp_cloud_ref as C
import _ftp_ref as P
import _graycode_ref as G

pytestmark = pytest.mark.gpu

META, DATA = AR.load()
PERIOD = META["period"]


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available()
    import simplestereo_amd
    return simplestereo_amd


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _rows(a, b, keep=None):
    e = C.rel_err(np.asarray(a), np.asarray(b).astype(np.longdouble))
    return float((e if keep is None else e[keep]).max())


def _rel(a, b):
    return float((np.abs(np.asarray(a, dtype=np.float64) - b) / np.abs(b)).max())


def _case(kind, name):
    c, d = META[kind][name], AR.fields(DATA, kind + "_" + name)
    roi = None if c["roi"] is None else tuple(c["roi"])
    x0, y0, w, h = AR.box(c["rig"], roi)
    cut = AR.frame(c["rig"], PERIOD)[y0:y0 + h, x0:x0 + w] if c["undistorted_is_the_frame"] else d["undistorted"]
    keep = np.unpackbits(d["keep"])[:h * w].reshape(h, w).astype(bool) if "keep" in d else None
    return c, d, roi, (x0, y0, w, h), np.array(cut), keep


def _device_unwrapper(f):
    import torch
    return lambda t: torch.from_numpy(f(t.cpu().numpy())).to(t.device)


# ------------------------------------------------------------------------------------------------ StereoFTP
@pytest.mark.parametrize("name", sorted(META["ftp"]))
def test_stereo_ftp_class_against_the_reference(ss, name):
    import torch
    c, d, roi, box, cut, keep = _case("ftp", name)
    frame = np.array(AR.frame(c["rig"], PERIOD))
    sf = ss.active.StereoFTP(C.make_rig(ss, c["rig"]), AR.fringe(PERIOD), PERIOD)
    method = None if c["unwrap"] is None else AR.UNWRAPPERS[c["unwrap"]]
    host = sf.getCloud(frame, c["radius_factor"], roi, unwrappingMethod=method)
    dev = sf.getCloud(torch.from_numpy(frame).cuda(), c["radius_factor"], roi, unwrappingMethod=None if method is None else _device_unwrapper(method))
    assert isinstance(host, np.ndarray) and host.dtype == np.float64 and host.shape == d["cloud"].shape == (box[3], box[2], 3)
    assert dev.is_cuda and dev.dtype == torch.float64 and tuple(dev.shape) == host.shape
    assert np.isfinite(host).all() and np.isfinite(dev.cpu().numpy()).all()
    # the stages the class goes through, against the reference's recorded ones
    got_cut, got_box, stripe, _ = sf._frame(frame, roi)
    assert got_box == box and np.array_equal(got_cut, cut) and _bits(stripe, d["stripe_cam"])
    world = sf._triangulate(stripe, sf.stripeCentralPeak, box)
    fc = sf._calculateCameraFrequency(world)
    ref = ss.active.ftpReference(sf.fringe, ss.active.ftpGeometry(sf.stereoRig, c["z_plane"], PERIOD, box))
    assert np.array_equal(ref, d["ref"]) and ref.dtype == np.uint8
    errs = {"host": _rows(host, d["cloud"], keep), "device": _rows(dev.cpu().numpy(), d["cloud"], keep),
            "stripe_world": _rows(world, d["stripe_world"]), "fc": _rel(fc, d["fc"]), "z_plane": abs(np.mean(world[:, 2]) - c["z_plane"]) / c["z_plane"]}
    print("ftp %-16s numpy_err %.3e tol %.3e  kernels vs reference: %s" % (name, c["numpy_err"], c["tol"], {k: "%.2e" % v for k, v in errs.items()}))
    assert all(v <= c["tol"] for v in errs.values()), errs


@pytest.mark.parametrize("name", ["full", "roi_17_5", "roi_camera_dist", "proj_d12", "radius_0.3"])
def test_stereo_ftp_public_chain_on_the_references_intermediates(ss, name):
    """ftpPhase(unwrap="numpy") -> ftpFringeOrder -> ftpCloud, fed the reference's undistorted cut, virtual reference image,
    fc, stripe and z_plane, on device tensors"""
    import torch
    a = ss.active
    c, d, roi, box, cut, keep = _case("ftp", name)
    rig = C.make_rig(ss, c["rig"])
    phase = a.ftpPhase(torch.from_numpy(cut).cuda(), torch.from_numpy(np.array(d["ref"])).cuda(), d["fc"], c["radius_factor"], unwrap="numpy")
    geom = a.ftpGeometry(rig, c["z_plane"], PERIOD, box)
    k = a.ftpFringeOrder(phase, np.ceil(d["stripe_cam"] - 0.5).astype(np.int64), geom, stripeCentralPeak=c["peak"])
    cloud = a.ftpCloud(phase, geom, k=k)
    assert cloud.is_cuda and tuple(cloud.shape) == d["cloud"].shape
    err = _rows(cloud.cpu().numpy(), d["cloud"], keep)
    print("ftp chain %-16s tol %.3e  kernels vs reference %.3e" % (name, c["tol"], err))
    assert err <= c["tol"]


# ------------------------------------------------------------------------------------------------ StereoFTP_Mapping
@pytest.mark.parametrize("name", sorted(META["mapping"]))
def test_mapping_class_and_chain_against_the_reference(ss, name):
    import torch
    a = ss.active
    c, d, roi, box, cut, _ = _case("mapping", name)
    x0, y0, w, h = box
    frame = np.array(AR.frame(c["rig"], PERIOD))
    sf = a.StereoFTP_Mapping(C.make_rig(ss, c["rig"]), AR.fringe(PERIOD), PERIOD)
    host = sf.getCloud(frame, c["radius_factor"], roi)
    dev = sf.getCloud(torch.from_numpy(frame).cuda(), c["radius_factor"], roi)
    assert isinstance(host, np.ndarray) and host.shape == d["cloud"].shape == (h, w, 3) and dev.is_cuda and _bits(dev.cpu().numpy(), host)
    # ftpCarrierPhase -> ftpStripePhase -> ftpMappingCloud on the reference's cut, fc and stripe; the reference samples the
    # phase at the stripe shifted by the roi origin (its in-place edit), which is where the chain is told to sample
    phase = a.ftpCarrierPhase(torch.from_numpy(cut).cuda(), d["fc"], c["radius_factor"], unwrap="numpy")
    theta = a.ftpStripePhase(phase, d["stripe_cam"] + np.array([x0, y0], dtype=np.float64))
    chain = a.ftpMappingCloud(phase, sf.stereoRig, PERIOD, c["peak"], theta, roi)
    errs = {"chain": _rows(chain.cpu().numpy(), d["cloud"])}
    if (x0, y0) == (0, 0):
        errs["host"] = _rows(host, d["cloud"])
    else:
        # the class samples the stripe where it is (README, compatibility table): per cent away from the reference here, and
        # equal to the chain told the same
        away = _rows(host, d["cloud"])
        plain = a.ftpMappingCloud(phase, sf.stereoRig, PERIOD, c["peak"], a.ftpStripePhase(phase, d["stripe_cam"]), roi)
        print("   the class, sampling the stripe where it is: %.3e from the reference" % away)
        assert 1e-3 < away < 1e-1 and _bits(plain.cpu().numpy(), host)
    print("mapping %-24s numpy_err %.3e tol %.3e  kernels vs reference: %s" % (name, c["numpy_err"], c["tol"], {k: "%.2e" % v for k, v in errs.items()}))
    assert np.isfinite(host).all() and all(v <= c["tol"] for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------ StereoFTP_PhaseOnly
def test_phase_only_class_against_the_reference(ss):
    import torch
    c, d = META["phase_only"]["roi"], AR.fields(DATA, "phase_only_roi")
    roi = tuple(c["roi"])
    frame = np.array(AR.frame(c["rig"], PERIOD))
    po = ss.active.StereoFTP_PhaseOnly(C.make_rig(ss, c["rig"]), AR.fringe(PERIOD), PERIOD)
    host = po.getPhase(frame, c["radius_factor"], roi)
    dev = po.getPhase(torch.from_numpy(frame).cuda(), c["radius_factor"], roi)
    assert isinstance(host, tuple) and len(host) == 3 and len(dev) == 3
    for i in range(3):
        keep = np.unpackbits(d["keep%d" % i])[:roi[2] * roi[3]].reshape(roi[3], roi[2]).astype(bool)
        assert host[i].shape == d["out%d" % i].shape and host[i].dtype == np.float64 and dev[i].is_cuda
        errs = [float(P.wrap_err(v, d["out%d" % i])[keep].max()) for v in (host[i], dev[i].cpu().numpy())]
        print("phase_only out%d: numpy_err %.3e tol %.3e  kernels vs reference %.3e (host) %.3e (device)" % (i, c["numpy_err"][i], c["tol"][i], *errs))
        assert max(errs) <= c["tol"][i]
    # roi=None: an UnboundLocalError in the reference (recorded), the whole frame here
    assert META["phase_only"]["roi_none"]["exception"] == "UnboundLocalError"
    whole = po.getPhase(frame, c["radius_factor"], None)
    assert len(whole) == 3 and all(v.shape == frame.shape[:2] and np.isfinite(v).all() for v in whole)


# ------------------------------------------------------------------------------------------------ GrayCode
@pytest.mark.parametrize("name", sorted(META["graycode"]))
def test_graycode_class_against_the_reference(ss, name):
    import torch
    c, d = META["graycode"][name], AR.fields(DATA, "gray_" + name)
    stack = AR.graycode_stack(c)
    roi = None if c["roi"] is None else tuple(c["roi"])
    gc = ss.active.GrayCode(G.make_rig(ss, c["rig"]), white_thr=c["white_thr"])
    assert gc.num_patterns == c["num_patterns"] == stack.shape[0]
    assert _bits(gc.Rectify1, d["Rectify1"]) and _bits(gc.Rectify2, d["Rectify2"]) and _bits(gc.R_inv, d["R_inv"]) and gc.rig.getBaseline() == c["baseline"]
    host = gc.getCloud(stack, roi)                                 # (a 1 x 1 projector has no pattern images: an empty stack)
    dense = gc.getCloud(stack, roi, dense=True)
    t = torch.from_numpy(stack).cuda()
    dev, dev_dense = gc.getCloud(t, roi), gc.getCloud(t, roi, dense=True)
    # the same count and, point by point, the same order
    assert host.shape == d["cloud"].shape == (c["n"], 1, 3) and host.dtype == np.float64 and tuple(dev.shape) == host.shape
    x0, y0, xe, ye = roi or (0, 0) + tuple(c["rig"]["res1"])
    assert dense.shape == (ye - y0, xe - x0, 3) and _bits(dev.cpu().numpy(), host) and G.same_points(dev_dense.cpu().numpy(), dense)
    valid = ~np.isnan(dense[..., 0])
    assert int(valid.sum()) == c["n"] and _bits(dense[valid].reshape(-1, 1, 3), host)
    err = _rows(host, d["cloud"])
    print("graycode %-18s %d points  numpy_err %.3e tol %.3e  kernels vs reference %.3e" % (name, c["n"], c["numpy_err"], c["tol"], err))
    assert np.isfinite(host).all() and err <= c["tol"]


# ------------------------------------------------------------------------------------------------ findCentralStripe
@pytest.mark.parametrize("name", sorted(META["stripe"]["cases"]))
def test_find_central_stripe_against_the_reference(ss, name):
    import torch
    c = META["stripe"]["cases"][name]
    img = AR.stripe_image(c, META["stripe"]["rig"], PERIOD)
    outs = [ss.active.findCentralStripe(v, c["color"], c["sensitivity"], c["interpolation"]) for v in (img, torch.from_numpy(img).cuda())]
    for out in outs:
        if c["found"]:
            assert isinstance(out, np.ndarray) and _bits(out, DATA["stripe_" + name + "__out"])
        else:
            assert out is None
