"""GPU: ss.active.ftpCloud (ftp_cloud_kernel), the triangulation of the reference's StereoFTP.getCloud (active.py:776-841),
against the extended-precision truth of tests/golden/ftp_cloud_cases within each case's own tolerance
(16 * max(numpy's own error, 2^-52), measured by tests/golden/make_golden_ftp_cloud.py), from host arrays and from device
tensors; and the chain camera frame -> phase -> unwrapped phase -> fringe order -> cloud without leaving the device."""
import json
import os

import numpy as np
import pytest

import _ftp_cloud_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available()
    import simplestereo_amd
    return simplestereo_amd


def _same(a, b):
    """identical 64-bit patterns, NaN at the same positions"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _args(ss, c):
    """ftpCloud's arguments after the phase, with the geometry the generator packed (the input the truth belongs to: a
    disparity of exactly 0 does not survive a last-bit difference in a matrix inverse)"""
    return ss.active.FtpGeometry(np.array(c["g"]), tuple(c["roi"]), c["fp"]), None, None, c["k"]


@pytest.mark.parametrize("name", R.case_names())
def test_every_case_within_tol_from_the_rig(ss, name):
    """The public path: the geometry packed from the StereoRig on this machine."""
    c = R.load_case(name)
    got = ss.active.ftpCloud(c["phase"], R.make_rig(ss, c["rig"]), c["z_plane"], c["period"], c["k"], tuple(c["roi"]))
    assert got.shape == c["truth"].shape and np.isfinite(got[c["keep"]]).all()
    err = float(R.rel_err(got, c["truth"])[c["keep"]].max())
    print("%s: kernel, geometry from the rig %.3e, tol %.3e" % (name, err, c["tol"]))
    assert err <= c["tol"]


@pytest.mark.parametrize("name", R.case_names())
def test_every_case_within_tol_host_and_device(ss, name):
    import torch
    c = R.load_case(name)
    host = ss.active.ftpCloud(c["phase"], *_args(ss, c))
    err = R.check_cloud(c, host)
    print("%s: kernel %.3e, numpy restatement %.3e, tol %.3e" % (name, err, c["numpy_err"], c["tol"]))
    assert err <= c["tol"]
    dev = ss.active.ftpCloud(torch.from_numpy(np.array(c["phase"])).cuda(), *_args(ss, c))
    assert dev.is_cuda and dev.dtype == torch.float64 and dev.is_contiguous()
    assert _same(dev.cpu().numpy(), host)                     # host and device results are bitwise equal


@pytest.mark.parametrize("name", ["p3x130", "dist_none", "dist_d5", "dist_d8", "dist_d12", "nonfinite"])
def test_kernel_evaluates_the_restatements_operations(ss, name):
    """The kernel's contract is stricter than the tolerance: the operations of tests/_ftp_cloud_ref.py in their order, each
    rounded once -- the same bits as numpy wherever the result is finite, and the same pixels non-finite."""
    c = R.load_case(name)
    got = ss.active.ftpCloud(c["phase"], *_args(ss, c))
    want = R.cloud_from_geometry(c["g"], c["phase"], c["k"], c["roi"][0], c["roi"][1])
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    keep = c["keep"]
    assert _same(got[keep], want[keep]), float(np.abs(got[keep] - want[keep]).max())


def test_non_finite_only_where_the_formulas_are(ss):
    c = R.load_case("nonfinite")
    got = ss.active.ftpCloud(c["phase"], *_args(ss, c))
    bad = ~np.isfinite(got).all(axis=-1)
    assert sorted(map(list, np.argwhere(bad))) == sorted(c["special"])
    assert not np.isfinite(got[~c["keep"]]).any()


def test_non_contiguous_view_equals_the_contiguous_map(ss):
    import torch
    c = R.load_case("p5x257_roi")
    want = ss.active.ftpCloud(c["phase"], *_args(ss, c))
    big = torch.zeros((10, 600), dtype=torch.float64, device="cuda")
    big[::2, 1:258] = torch.from_numpy(np.array(c["phase"])).cuda()
    view = big[::2, 1:258]
    assert not view.is_contiguous()
    assert _same(ss.active.ftpCloud(view, *_args(ss, c)).cpu().numpy(), want)
    # a contiguous view at a storage offset that is not a multiple of 16 bytes
    flat = torch.zeros(5 * 257 + 1, dtype=torch.float64, device="cuda")
    flat[1:] = torch.from_numpy(np.array(c["phase"])).cuda().reshape(-1)
    odd = flat[1:].view(5, 257)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 8
    assert _same(ss.active.ftpCloud(odd, *_args(ss, c)).cpu().numpy(), want)
    host = np.zeros((10, 600))
    host[::2, 1:258] = c["phase"]
    assert _same(ss.active.ftpCloud(host[::2, 1:258], *_args(ss, c)), want)


def test_non_default_stream(ss):
    """The call runs on the current stream: it is ordered behind the kernel that fills its phase on that stream, and its
    result is complete once that stream is synchronised."""
    import torch
    c = R.load_case("p3x130")
    want = ss.active.ftpCloud(c["phase"], *_args(ss, c))
    src = torch.from_numpy(np.array(c["phase"])).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        phase = torch.full_like(src, float("nan"))
        phase.copy_(src * 1.0)                               # filled on s just before the call
        out = ss.active.ftpCloud(phase, *_args(ss, c))
        total = out.sum()                                    # consumed on s without a synchronisation in between
    s.synchronize()
    assert _same(out.cpu().numpy(), want)
    assert float(total.cpu()) == float(out.sum().cpu())


def test_profile_slot_and_kernel_name(ss):
    from simplestereo_amd import _native
    import torch
    c = R.load_case("p3x64")
    lib = _native.lib()
    name = lib.ssamd_kernel_name(_native.K_REPROJECT)
    assert b"reproject_kernel" in name and b"ftp_cloud_kernel" in name
    t = torch.from_numpy(np.array(c["phase"])).cuda()
    lib.ssamd_profile_enable(1)
    try:
        for phase, calls in ((c["phase"], 1), (t, 3)):
            lib.ssamd_profile_reset()
            for _ in range(calls):
                ss.active.ftpCloud(phase, *_args(ss, c))
            ms, n = _native.profile_read()
            assert n[_native.K_REPROJECT] == calls and ms[_native.K_REPROJECT] > 0
            assert n[_native.K_FTP] == 0 and n[_native.K_NPUNWRAP] == 0
            assert sum(n) == calls
    finally:
        lib.ssamd_profile_enable(0)


def test_pipeline_on_the_device_equals_the_downloaded_map(ss):
    """ftpPhase(unwrap="numpy") -> ftpFringeOrder -> ftpCloud on device tensors equals, bit for bit, ftpCloud on the
    downloaded unwrapped map (and the fringe order taken from it)."""
    import torch
    name = "w257"
    with open(os.path.join(G, "ftp_cases.json")) as f:
        rf = json.load(f)["cases"][name]["radius_factor"]
    z = np.load(os.path.join(G, "ftp_cases.npz"))
    obj, ref, fc = z[name + "__obj"], z[name + "__ref"], z[name + "__fc"]
    h, w = obj.shape[:2]
    rig = R.make_rig(ss, R.rig_params(dist="d8"))
    roi, z_plane, period = (400, 250, w, h), 1000.0, 12.0
    stripe = np.array([[w // 2, y] for y in range(h)])
    geometry = ss.active.ftpGeometry(rig, z_plane, period, roi)
    # a central stripe about two and a half periods from where the stripe pixels fall on the reference plane
    peak = float(np.round(R.project_points(geometry.geom, roi[0] + w // 2 + 0.5, roi[1] + 0.5)[0])) + 30.0
    phase_dev = ss.active.ftpPhase(torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda(), fc, rf, unwrap="numpy")
    k_dev = ss.active.ftpFringeOrder(phase_dev, stripe, geometry, stripeCentralPeak=peak)
    cloud_dev = ss.active.ftpCloud(phase_dev, geometry, k=k_dev)
    assert phase_dev.is_cuda and cloud_dev.is_cuda and cloud_dev.shape == (h, w, 3)
    phase = phase_dev.cpu().numpy()
    k = ss.active.ftpFringeOrder(phase, stripe, rig, z_plane, period, peak, roi)
    assert k == k_dev == R.fringe_order(geometry.geom, geometry.fp, phase, stripe, peak, roi[0], roi[1]) and abs(k) >= 2
    want = ss.active.ftpCloud(phase, rig, z_plane, period, k, roi)
    assert np.isfinite(want).all() and _same(cloud_dev.cpu().numpy(), want)
    # ... and is the triangulation of that map: within 16 errors of numpy of the extended-precision truth
    truth = R.cloud_from_geometry(geometry.geom, phase, k, roi[0], roi[1], dtype=np.longdouble)
    numpy_err = float(R.rel_err(R.cloud_from_geometry(geometry.geom, phase, k, roi[0], roi[1]), truth).max())
    assert float(R.rel_err(want, truth).max()) <= 16 * max(numpy_err, 2.0 ** -52)
