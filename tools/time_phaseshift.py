"""Timing of ss.active.PhaseShift on the MI355X: its two kernels alone, getCloud for a device and a host stack, and the numpy
restatement on the host.

    python tools/time_phaseshift.py [--reps 20] [--out profiles/phaseshift_timing.txt]

For camera stacks of 1920x1080 and 4096x2160 with a 1920x1080 projector, periods x (1920, 240, 30) and y (1080, 135, 15), so
N = 24 images (8 distortion coefficients on the projector, 5 on the camera; tests/_phaseshift_ref.scene: a smooth surface,
amplitude 100, evenly lit), after warm-up, the MEDIAN over --reps calls of
  phaseshift_decode_kernel  alone (HIP events around the launch: ssamd_profile_*), with the undistortion maps and without, each
                            beside the HBM floor of the bytes it must move (N + 8 read with maps, N without, 16 written per pixel,
                            over 8 TB/s) and as a fraction of the copy bandwidth measured in the same run (a 1 GiB device copy, the
                            measurement of tools/hbm_bw.py)
  sl_triangulate_kernel     alone, on the pixel grid (16 read, 24 written per pixel) and on camera points of the caller's (32 read)
  getCloud                  a device-tensor stack (torch events) and a host stack (host clock, copies included)
  numpy                     the restatement of tests/_phaseshift_ref.py on the host (host clock, one call)
and how far the device cloud is from the restatement's (the device's atan2 is not numpy's: not bit for bit)."""
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
PROJ = (1920, 1080)
PERIODS = ([1920.0, 240.0, 30.0], [1080.0, 135.0, 15.0])


def main():
    import torch
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    import _ftp_cloud_ref as C
    import _graycode_ref as G
    import _phaseshift_ref as P
    import _stereo_ftp_ref as S
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1920x1080,4096x2160")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_phaseshift.py measures on a GPU"
    lib = _native.lib()
    a = ss.active
    N = 4 * (len(PERIODS[0]) + len(PERIODS[1]))

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
    lines = ["ss.active.PhaseShift timing on %s; median of %d calls after warm-up, ms per stack; %d x %d projector, periods x %s y %s, N = %d"
             % (torch.cuda.get_device_name(0), args.reps, PROJ[0], PROJ[1], PERIODS[0], PERIODS[1], N),
             "HBM floor: the bytes a kernel must move over %.1f TB/s; copy: over the %.2f TB/s (read + written) a 1 GiB device copy reaches in this run"
             % (HBM_PEAK * 1e-12, copy_bw * 1e-12)]

    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        rig = G.rig((w, h), PROJ, "d8", dist1=[-0.08, 0.03, 0.0005, -0.0004, 0.0])
        stack = P.scene(7, (w, h), PROJ, PERIODS, low=100, extra=0)           # (evenly lit: every k is far from a tie)
        ps = a.PhaseShift(G.make_rig(ss, rig), PERIODS)
        t = torch.from_numpy(stack).cuda()
        mx, my = a._cached_maps(ps._cache, ps.rig, t.device)
        gp = ps.rig._geometry().ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        proj = a.phaseShiftDecode(t, PERIODS, PROJ, maps=(mx, my))
        cam = torch.from_numpy(P.grid((0, 0, w, h))).cuda().reshape(-1, 2)
        out = torch.empty((h, w, 3), dtype=torch.float64, device=t.device)

        t_dec_maps = kernel_alone(lambda: a.phaseShiftDecode(t, PERIODS, PROJ, maps=(mx, my)), _native.K_FTP)
        t_dec = kernel_alone(lambda: a.phaseShiftDecode(t, PERIODS, PROJ), _native.K_FTP)
        t_tri_grid = kernel_alone(lambda: _native.call_on_stream(t, lib.ssamd_sl_triangulate_device, None, proj.data_ptr(), h * w, w, 0, 0, gp,
                                                                 out.data_ptr()), _native.K_REPROJECT)
        t_tri = kernel_alone(lambda: _native.call_on_stream(t, lib.ssamd_sl_triangulate_device, cam.data_ptr(), proj.data_ptr(), h * w, w, 0, 0, gp,
                                                            out.data_ptr()), _native.K_REPROJECT)
        t_dev = median_events(lambda: ps.getCloud(t))
        t_dev_clock = median_clock(lambda: (ps.getCloud(t), torch.cuda.synchronize()))
        t_host = median_clock(lambda: ps.getCloud(stack), warm=1, reps=3)
        t0 = time.perf_counter()
        hx, hy = S.undistort_maps(np.array(rig["intrinsic1"]), rig["distCoeffs1"], (w, h))
        want = P.triangulate(P.sl_rig(rig)["geom"], P.grid((0, 0, w, h)), P.decode(G.remap_stack_taps_once(stack, hx, hy), PERIODS, PROJ))
        t_numpy = 1e3 * (time.perf_counter() - t0)
        err = float(np.nanmax(C.rel_err(ps.getCloud(t).cpu().numpy().reshape(-1, 1, 3), want.astype(np.longdouble))))

        px = h * w
        ms = lambda nbytes, bw: nbytes / bw * 1e3      # noqa: E731
        rows = [("phaseshift_decode_kernel alone, with maps", t_dec_maps, (N + 8 + 16) * px),
                ("phaseshift_decode_kernel alone, no maps", t_dec, (N + 16) * px),
                ("sl_triangulate_kernel alone, pixel grid", t_tri_grid, 40 * px),
                ("sl_triangulate_kernel alone, camera points", t_tri, 56 * px)]
        lines += ["", "%s  (%d pixels)" % (size, px)]
        for name, tm, nbytes in rows:
            lines.append("  %-44s %9.4f   (HBM floor %.4f = %.0f %%; copy %.4f = %.0f %%; %.2f TB/s)"
                         % (name, tm, ms(nbytes, HBM_PEAK), 100 * ms(nbytes, HBM_PEAK) / tm, ms(nbytes, copy_bw), 100 * ms(nbytes, copy_bw) / tm,
                            nbytes / tm * 1e-9))
        lines += ["  %-44s %9.3f   (torch events; host clock with a final synchronisation %.3f)" % ("getCloud, device-tensor stack", t_dev, t_dev_clock),
                  "  %-44s %9.1f" % ("getCloud, host stack (copies included)", t_host),
                  "  %-44s %9.1f" % ("numpy restatement on the host", t_numpy),
                  "  worst relative distance of the device cloud to the numpy restatement's: %.2e" % err]
        print("\n".join(lines[-9:]), flush=True)
        del t, proj, cam, out
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
