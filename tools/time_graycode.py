"""Timing of ss.active.GrayCode on the MI355X: its three kernels alone, getCloud for a device and a host stack, and the numpy
restatement on the host.

    python tools/time_graycode.py [--reps 20] [--out profiles/graycode_timing.txt]

For camera stacks of 1920x1080 and 4096x2160 with a 1920x1080 projector (N = 44 pattern images; 8 distortion coefficients on the
projector, 5 on the camera; tests/_graycode_ref.scene: a smooth surface, contrast 60, +-2 of noise, a tenth of the pixels with one
washed-out bit), after warm-up, the MEDIAN over --reps calls of
  graycode_decode_kernel   alone (HIP events around the launch: ssamd_profile_*), with the undistortion maps and without, each
                           beside the HBM floor of the bytes it must move (N + 8 read with maps, N without, 8 written per pixel,
                           over 8 TB/s) and as a fraction of the copy bandwidth measured in the same run (a 1 GiB device copy, the
                           measurement of tools/hbm_bw.py)
  graycode_scan_kernel     alone
  graycode_cloud_kernel    alone, compacted and dense (8 read per pixel, 24 written per valid pixel / per pixel)
  getCloud                 a device-tensor stack, compacted (torch events; the read-back of the count included) and dense, and a
                           host stack (host clock, copies included)
  numpy                    the restatement of tests/_graycode_ref.py on the host (host clock, one call)
and whether the device cloud equals the restatement's bit for bit."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12                                    # bytes per second (MI355X specification)


def main():
    import torch
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    import _graycode_ref as G
    import _stereo_ftp_ref as S
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1920x1080,4096x2160")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_graycode.py measures on a GPU"
    lib = _native.lib()
    a = ss.active
    proj = (1920, 1080)
    N = G.num_patterns(*proj)

    def median_events(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    def median_clock(fn, warm=1, reps=None):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps or args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts)

    def kernel_alone(fn, slot):
        for _ in range(3):
            fn()
        lib.ssamd_profile_enable(1)
        ts = []
        try:
            for _ in range(args.reps):
                lib.ssamd_profile_reset()
                fn()
                ms, n = _native.profile_read()
                assert n[slot] == 1
                ts.append(ms[slot])
        finally:
            lib.ssamd_profile_enable(0)
        return statistics.median(ts)

    # the copy bandwidth of this device in this run: tools/hbm_bw.py's 1 GiB copy
    n_copy = 1 << 30
    src, dst = torch.empty(n_copy, dtype=torch.uint8, device="cuda"), torch.empty(n_copy, dtype=torch.uint8, device="cuda")
    src.fill_(7)
    copy_bw = 2 * n_copy / (median_events(lambda: dst.copy_(src)) * 1e-3)
    del src, dst
    lines = ["ss.active.GrayCode timing on %s; median of %d calls after warm-up, ms per stack; %d x %d projector, N = %d"
             % (torch.cuda.get_device_name(0), args.reps, proj[0], proj[1], N),
             "HBM floor: the bytes a kernel must move over %.1f TB/s; copy: over the %.2f TB/s (read + written) a 1 GiB device copy reaches in this run"
             % (HBM_PEAK * 1e-12, copy_bw * 1e-12)]

    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        rig = G.rig((w, h), proj, "d8", dist1=[-0.08, 0.03, 0.0005, -0.0004, 0.0])
        stack = G.scene(7, (w, h), proj, noise=2)
        gc = a.GrayCode(G.make_rig(ss, rig))
        t = torch.from_numpy(stack).cuda()
        mx, my = gc._maps(t.device)
        geom = gc._geometry()
        gp = geom.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        args_dev = a._gray_decode_args(t, gc._proj, gc.white_thr, mx, my, (0, 0, w, h))
        decoded, counts = a._gray_decode_device(t, args_dev, h, w)
        nb = int(counts.shape[0])
        offsets = torch.empty((nb + 1,), dtype=torch.int32, device=t.device)
        _native.call_on_stream(t, lib.ssamd_graycode_offsets_device, counts.data_ptr(), nb, offsets.data_ptr())
        n = int(offsets[-1].item())
        out = torch.empty((h, w, 3), dtype=torch.float64, device=t.device)

        t_dec_maps = kernel_alone(lambda: a.grayCodeDecode(t, proj, maps=(mx, my)), _native.K_FTP)
        t_dec = kernel_alone(lambda: a.grayCodeDecode(t, proj), _native.K_FTP)
        t_scan = kernel_alone(lambda: _native.call_on_stream(t, lib.ssamd_graycode_offsets_device, counts.data_ptr(), nb, offsets.data_ptr()),
                              _native.K_FTP)
        t_cloud = kernel_alone(lambda: _native.call_on_stream(t, lib.ssamd_graycode_cloud_device, decoded.data_ptr(), h, w, 0, 0, gp,
                                                              offsets.data_ptr(), out.data_ptr()), _native.K_REPROJECT)
        t_cloud_dense = kernel_alone(lambda: _native.call_on_stream(t, lib.ssamd_graycode_cloud_device, decoded.data_ptr(), h, w, 0, 0, gp,
                                                                    None, out.data_ptr()), _native.K_REPROJECT)
        t_dev = median_events(lambda: gc.getCloud(t))
        t_dev_clock = median_clock(lambda: (gc.getCloud(t), torch.cuda.synchronize()))
        t_dense = median_events(lambda: gc.getCloud(t, dense=True))
        t_host = median_clock(lambda: gc.getCloud(stack), warm=1, reps=3)
        t0 = time.perf_counter()
        hx, hy = S.undistort_maps(np.array(rig["intrinsic1"]), rig["distCoeffs1"], (w, h))
        dec = G.decode(G.remap_stack_taps_once(stack, hx, hy), proj[0], proj[1], 5)
        want = G.compact(G.cloud_dense(G.geometry(rig), dec, 0, 0), dec)
        t_numpy = 1e3 * (time.perf_counter() - t0)
        same = G.same_points(gc.getCloud(t).cpu().numpy(), want)

        px = h * w
        ms = lambda nbytes, bw: nbytes / bw * 1e3      # noqa: E731
        rows = [("graycode_decode_kernel alone, with maps", t_dec_maps, (N + 16) * px),
                ("graycode_decode_kernel alone, no maps", t_dec, (N + 8) * px),
                ("graycode_cloud_kernel alone, compacted", t_cloud, 8 * px + 24 * n),
                ("graycode_cloud_kernel alone, dense", t_cloud_dense, 32 * px)]
        lines += ["", "%s  (%d pixels, %d valid = %.1f %%; %d blocks)" % (size, px, n, 100.0 * n / px, nb)]
        for name, tm, nbytes in rows:
            lines.append("  %-44s %9.4f   (HBM floor %.4f = %.0f %%; copy %.4f = %.0f %%; %.2f TB/s)"
                         % (name, tm, ms(nbytes, HBM_PEAK), 100 * ms(nbytes, HBM_PEAK) / tm, ms(nbytes, copy_bw), 100 * ms(nbytes, copy_bw) / tm,
                            nbytes / tm * 1e-9))
        lines += ["  %-44s %9.4f" % ("graycode_scan_kernel alone (%d counts)" % nb, t_scan),
                  "  %-44s %9.3f   (torch events; host clock with a final synchronisation %.3f)" % ("getCloud, device-tensor stack", t_dev, t_dev_clock),
                  "  %-44s %9.3f" % ("getCloud(dense=True), device-tensor stack", t_dense),
                  "  %-44s %9.1f" % ("getCloud, host stack (copies included)", t_host),
                  "  %-44s %9.1f" % ("numpy restatement on the host", t_numpy),
                  "  the device cloud equals the numpy restatement's bit for bit: %s" % same]
        print("\n".join(lines[-11:]), flush=True)
        del t, decoded, out
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
