"""GPU: what the Python layer hands to libssamd.so for device tensors.  A proxy around the loaded library records every call and
passes it on; each route is driven inside ``torch.cuda.stream(side)`` on the smallest shapes every route accepts.  Asserted per
route: the entry point, the arguments in the order of include/ssamd.h (written out by hand), the current stream's handle as the
last one, and a result equal bit for bit to the same operator on host arrays (which the rest of the suite holds to the oracle)."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PI = float(np.pi)
OUT = object()           # placeholder: the pointer of the tensor the call returns
HOSTPTR = object()       # placeholder: a pointer to a host temporary


class Proxy:
    """records ``(name, args)`` of every ``ssamd_*`` call, then calls the library; ctypes pointers are read while the call's
    temporaries are alive (``peek[name] = {argument index: count}``)"""

    def __init__(self, real, peek=None):
        self.real = real
        self.calls = []
        self.peek = peek or {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)
        if not name.startswith("ssamd_") or name == "ssamd_last_error":
            return fn

        def call(*args):
            seen = list(args)
            for i, count in self.peek.get(name, {}).items():
                seen[i] = tuple(args[i][k] for k in range(count))
            self.calls.append((name, tuple(seen)))
            return fn(*args)
        return call


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import simplestereo_amd as ss
    from simplestereo_amd.synth import make_pair
    before = ss.passive.set_autotune(False)          # no trial launches: these calls are about arguments, not speed
    L, R, _ = make_pair(24, 40, 4, 7)
    e = dict(ss=ss, torch=torch, side=torch.cuda.Stream(), L=L, R=R, tL=torch.from_numpy(L).cuda(), tR=torch.from_numpy(R).cuda(),
             phase=np.random.default_rng(21).uniform(-9, 9, (16, 24)))
    e["tphase"] = torch.from_numpy(e["phase"]).cuda()
    rig = ss.RectifiedStereoRig.fromFile(os.path.join(GOLDEN, "rig_example2_rigRect.json"))
    rig.computeRectificationMaps(destDims=(40, 24))
    w, h = rig.res1
    rng = np.random.default_rng(22)
    e["rig"] = rig
    e["raw"] = tuple(rng.integers(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2))
    e["traw"] = tuple(torch.from_numpy(x).cuda() for x in e["raw"])
    torch.cuda.synchronize()
    yield e
    ss.passive.set_autotune(before)


@pytest.fixture
def px(env, monkeypatch):
    from simplestereo_amd import _native
    p = Proxy(_native.lib(), {"ssamd_reproject_device": {3: 16}})
    monkeypatch.setattr(_native, "lib", lambda: p)
    return p


def _drive(env, px, fn, name, want):
    """run fn on the side stream; ONE native call, `name` with `want` followed by the side stream's handle -> (tensor, host copy)"""
    torch, side = env["torch"], env["side"]
    del px.calls[:]
    with torch.cuda.stream(side):
        out = fn()
        host = out.cpu().numpy()
    assert [c[0] for c in px.calls] == [name]
    _check_call(env, px.calls[0], name, want, out)
    return out, host


def _check_call(env, call, name, want, out):
    got_name, args = call
    assert got_name == name
    assert len(args) == len(want) + 1, (name, args)
    for i, (g, w) in enumerate(zip(args, want)):
        if w is OUT:
            assert type(g) is int and g == out.data_ptr(), (name, i)
        elif w is HOSTPTR:
            assert type(g) is int and g != 0, (name, i)
        else:
            assert type(g) is type(w) and g == w, (name, i, g, w)
    stream = args[-1]
    assert isinstance(stream, ctypes.c_void_p) and stream.value == env["side"].cuda_stream != 0


ASW = dict(winSize=5, maxDisparity=4, minDisparity=1, gammaC=4, gammaP=9.5, consistent=True)
ASW_SCALARS = (5, 4, 1, 4.0, 9.5, 1)           # winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent
GSW = dict(winSize=5, maxDisparity=4, minDisparity=1, gamma=9, fMax=100, iterations=2, bins=13)
GSW_SCALARS = (5, 4, 1, 9, 100.0, 2, 13)       # winSize, maxDisparity, minDisparity, gamma, fMax, iterations, bins


def _matchers(ss):
    """(matcher, scalars, name of the plain / rows2 / rectified entry point)"""
    return [(ss.passive.StereoASW(**ASW), ASW_SCALARS, "ssamd_asw_exact_device", "ssamd_asw_exact_device_rows2", "ssamd_asw_exact_rectified_device"),
            (ss.passive.StereoASW(exact=False, **ASW), ASW_SCALARS, "ssamd_asw_device", "ssamd_asw_device_rows2", "ssamd_asw_rectified_device"),
            (ss.passive.StereoGSW(**GSW), GSW_SCALARS, "ssamd_gsw_device", "ssamd_gsw_device_rows2", "ssamd_gsw_rectified_device")]


def test_matchers_on_device_tensors(env, px):
    """int ssamd_*_device(d_img1, d_img2, height, width, out_row0, out_rows, <parameters>, d_disparity, stream) and
    ..._device_rows2(d_img1, d_img2, height, width, out_row0, out_rows, skip_row0, skip_rows, <parameters>, d_disparity, stream)"""
    ss, torch, tL, tR = env["ss"], env["torch"], env["tL"], env["tR"]
    a, b = tL.data_ptr(), tR.data_ptr()
    for m, scalars, plain, rows2, _ in _matchers(ss):
        whole = m.compute(env["L"], env["R"])
        _, got = _drive(env, px, lambda: m.compute(tL, tR), plain, (a, b, 24, 40, 0, 24) + scalars + (OUT,))
        assert got.dtype == np.int16 and np.array_equal(got, whole)
        _, got = _drive(env, px, lambda: m._compute_device(tL, tR, out_row0=3, out_rows=7), plain, (a, b, 24, 40, 3, 7) + scalars + (OUT,))
        assert np.array_equal(got, whole[3:10])
        _, got = _drive(env, px, lambda: m._compute_device(tL, tR, out_row0=5), plain, (a, b, 24, 40, 5, 19) + scalars + (OUT,))
        assert np.array_equal(got, whole[5:])
        buf = torch.full((20, 40), -7, dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()
        out, got = _drive(env, px, lambda: m._compute_device(tL, tR, out_row0=2, out_rows=20, out=buf, skip=(6, 9)), rows2,
                          (a, b, 24, 40, 2, 20, 6, 9) + scalars + (OUT,))
        assert out is buf
        assert np.array_equal(got[:4], whole[2:6]) and np.array_equal(got[13:], whole[15:22]) and (got[4:13] == -7).all()
        # skip of no rows: the one-range entry point
        _drive(env, px, lambda: m._compute_device(tL, tR, out_row0=2, out_rows=20, skip=(6, 0)), plain, (a, b, 24, 40, 2, 20) + scalars + (OUT,))


def test_asw_alternate_on_device_tensors(env, px):
    """int ssamd_asw_alternate_rows_device(d_img1, d_img2, height, width, out_row0, out_rows, row_parity, winSize, ..., d_disparity, stream)"""
    ss, torch, tL, tR = env["ss"], env["torch"], env["tL"], env["tR"]
    m = ss.passive.StereoASW(alternate=True, **ASW)
    whole = m.compute(env["L"], env["R"])
    _, got = _drive(env, px, lambda: m.compute(tL, tR), "ssamd_asw_alternate_rows_device",
                    (tL.data_ptr(), tR.data_ptr(), 24, 40, 0, 24, 0) + ASW_SCALARS + (OUT,))
    assert np.array_equal(got, whole)
    sL, sR = tL[1:].contiguous(), tR[1:].contiguous()          # first row odd in the whole image; 5 // 2 + 1 halo rows above row 4
    torch.cuda.synchronize()
    _, got = _drive(env, px, lambda: m._compute_device(sL, sR, out_row0=3, out_rows=6, row_parity=1), "ssamd_asw_alternate_rows_device",
                    (sL.data_ptr(), sR.data_ptr(), 23, 40, 3, 6, 1) + ASW_SCALARS + (OUT,))
    assert np.array_equal(got, whole[4:10])
    _drive(env, px, lambda: m._compute_device(sL, sR, out_row0=3, out_rows=6, row_parity=3), "ssamd_asw_alternate_rows_device",
           (sL.data_ptr(), sR.data_ptr(), 23, 40, 3, 6, 1) + ASW_SCALARS + (OUT,))          # only the parity bit is passed
    del px.calls[:]
    with pytest.raises(ValueError):
        m._compute_device(tL, tR, out_row0=2, out_rows=20, skip=(6, 9))
    assert px.calls == []


def test_matchers_rectify_and_match(env, px):
    """int ssamd_*_rectified_device(d_raw1, d_raw2, src_height, src_width, d_mapx1, d_mapy1, d_mapx2, d_mapy2, height, width,
    interpolation, <parameters>, d_disparity, stream)"""
    ss, rig = env["ss"], env["rig"]
    r1, r2 = env["traw"]
    w, h = rig.res1
    maps = tuple(t.data_ptr() for t in rig._device_maps(1, r1.device) + rig._device_maps(2, r1.device))
    for interp in (1, 0):
        rect = rig.rectifyImages(*env["raw"], interp)
        for m, scalars, _, _, entry in _matchers(ss):
            _, got = _drive(env, px, lambda: m.compute(r1, r2, rectify=rig, interpolation=interp), entry,
                            (r1.data_ptr(), r2.data_ptr(), h, w) + maps + (24, 40, interp) + scalars + (OUT,))
            assert got.dtype == np.int16 and np.array_equal(got, m.compute(*rect))


def test_rig_kernels_on_device_tensors(env, px):
    """int ssamd_remap_bgr_device(d_src, src_h, src_w, d_mapx, d_mapy, dst_h, dst_w, interpolation, d_dst, stream);
    int ssamd_reproject_device(d_disparity, h, w, const double *Q, d_points, stream)"""
    ss, torch, rig, side = env["ss"], env["torch"], env["rig"], env["side"]
    r1, r2 = env["traw"]
    w, h = rig.res1
    m1, m2 = rig._device_maps(1, r1.device), rig._device_maps(2, r1.device)
    for interp in (1, 0):
        del px.calls[:]
        with torch.cuda.stream(side):
            o1, o2 = rig.rectifyImages(r1, r2, interp)
            g1, g2 = o1.cpu().numpy(), o2.cpu().numpy()
        assert [c[0] for c in px.calls] == ["ssamd_remap_bgr_device"] * 2
        for call, src, maps, out in ((px.calls[0], r1, m1, o1), (px.calls[1], r2, m2, o2)):
            _check_call(env, call, "ssamd_remap_bgr_device", (src.data_ptr(), h, w, maps[0].data_ptr(), maps[1].data_ptr(), 24, 40, interp, OUT), out)
        h1, h2 = rig.rectifyImages(*env["raw"], interp)
        assert g1.dtype == np.uint8 and np.array_equal(g1, h1) and np.array_equal(g2, h2)
    disp = np.random.default_rng(23).integers(1, 30, (24, 40)).astype(np.int16)
    td = torch.from_numpy(disp).cuda()
    torch.cuda.synchronize()
    _, got = _drive(env, px, lambda: rig.get3DPoints(td), "ssamd_reproject_device",
                    (td.data_ptr(), 24, 40, tuple(float(q) for q in rig.getQ().ravel()), OUT))
    want = rig.get3DPoints(disp)
    print("get3DPoints, tensor against host array: %d of %d values differ, largest difference %.3e"
          % (np.count_nonzero(got != want), got.size, float(np.abs(got - want).max())))
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_unwrappers_on_device_tensors(env, px):
    """int ssamd_iir_unwrap_device(d_phase, n, h, w, tau, d_out, stream);
    int ssamd_np_unwrap_device(d_p, long long outer, long long len, long long inner, discont, period, d_out, stream);
    int ssamd_np_unwrap_xy_device(d_p, n, h, w, d_out, stream)"""
    ss, torch, phase, t = env["ss"], env["torch"], env["phase"], env["tphase"]
    U = ss.unwrapping
    _, got = _drive(env, px, lambda: U.infiniteImpulseResponse(t, tau=0.75), "ssamd_iir_unwrap_device", (t.data_ptr(), 1, 16, 24, 0.75, OUT))
    assert np.array_equal(got.view(np.uint64), U.infiniteImpulseResponse(phase, tau=0.75).view(np.uint64))
    batch = np.stack([phase, -phase])
    tb = torch.from_numpy(batch).cuda()
    torch.cuda.synchronize()
    _, got = _drive(env, px, lambda: U.infiniteImpulseResponseBatch(tb, tau=1), "ssamd_iir_unwrap_device", (tb.data_ptr(), 2, 16, 24, 1.0, OUT))
    assert np.array_equal(got.view(np.uint64), U.infiniteImpulseResponseBatch(batch, tau=1).view(np.uint64))
    _, got = _drive(env, px, lambda: U.unwrap(tb, axis=1), "ssamd_np_unwrap_device", (tb.data_ptr(), 2, 16, 24, PI, 2 * PI, OUT))
    assert np.array_equal(got.view(np.uint64), U.unwrap(batch, axis=1).view(np.uint64))
    _, got = _drive(env, px, lambda: U.unwrap(tb, 1.5, 0, period=4), "ssamd_np_unwrap_device", (tb.data_ptr(), 1, 2, 384, 1.5, 4.0, OUT))
    assert np.array_equal(got.view(np.uint64), U.unwrap(batch, 1.5, 0, period=4).view(np.uint64))
    _, got = _drive(env, px, lambda: U.unwrap2D(t), "ssamd_np_unwrap_xy_device", (t.data_ptr(), 1, 16, 24, OUT))
    assert np.array_equal(got.view(np.uint64), U.unwrap2D(phase).view(np.uint64))
    _, got = _drive(env, px, lambda: U.unwrap2D(tb), "ssamd_np_unwrap_xy_device", (tb.data_ptr(), 2, 16, 24, OUT))
    assert np.array_equal(got.view(np.uint64), U.unwrap2D(batch).view(np.uint64))
    del px.calls[:]
    assert tuple(U.unwrap(tb[:, :0], axis=1).shape) == (2, 0, 24) and tuple(U.infiniteImpulseResponse(t[:0]).shape) == (0, 24)
    assert px.calls == []                                     # an empty tensor: a result, no native call


def test_ftp_on_device_tensors(env, px):
    """int ssamd_ftp_phase_device(d_img_obj, ch_obj, d_img_ref, ch_ref, h, w, const double *fmin, const double *fmax, unwrap, tau,
    d_out, stream);  int ssamd_ftp_cloud_device(d_phase, h, w, x0, y0, const double *geom, k, d_out, stream)"""
    ss, torch, L, R, tL = env["ss"], env["torch"], env["L"], env["R"], env["tL"]
    ref = np.ascontiguousarray(R[:, :, 0])
    tref = torch.from_numpy(ref).cuda()
    torch.cuda.synchronize()
    for unwrap, uw, tau in ((None, 0, 1.0), ("iir", 1, 0.5), ("numpy", 2, 1.0)):
        _, got = _drive(env, px, lambda: ss.active.ftpPhase(tL, tref, 0.15, radius_factor=0.5, unwrap=unwrap, tau=0.5), "ssamd_ftp_phase_device",
                        (tL.data_ptr(), 3, tref.data_ptr(), 1, 24, 40, HOSTPTR, HOSTPTR, uw, tau, OUT))
        want = ss.active.ftpPhase(L, ref, 0.15, radius_factor=0.5, unwrap=unwrap, tau=0.5)
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    rig = ss.StereoRig.fromFile(os.path.join(GOLDEN, "rig_example1_rig.json"))
    G = ss.active.ftpGeometry(rig, 500.0, 12.0, roi=(3, 2, 24, 16))
    t = env["tphase"]
    _, got = _drive(env, px, lambda: ss.active.ftpCloud(t, G, k=2), "ssamd_ftp_cloud_device", (t.data_ptr(), 16, 24, 3, 2, G.geom.ctypes.data, 2.0, OUT))
    want = ss.active.ftpCloud(env["phase"], G, k=2)
    assert got.shape == (16, 24, 3) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
