"""Timing of ss.active.ftpCloud (ftp_cloud_kernel) on the MI355X, beside the same triangulation in numpy on the host and beside
the demodulation kernel (ftp_phase_kernel) that feeds it, measured in the same run.

    python tools/time_ftp_cloud.py [--reps 50] [--out profiles/ftp_cloud_timing.txt]

For 1920x1080 and 4096x2160 (a camera of that resolution, a 1280x720 projector 250 mm to its side, 8 distortion coefficients,
z_plane = 1000, period = 12, a smooth phase map), after warm-up, the MEDIAN over --reps calls of
  kernel        ftp_cloud_kernel alone (HIP events around the launch: ssamd_profile_*), with the share of the HBM roofline: the
                32 bytes per pixel it must move (8 read, 24 written) at the 8.0 TB/s peak, over the kernel time -- and the same
                for each distortion model (the kernel is instantiated per model)
  device call   ftpCloud on a float64 tensor already in HBM (torch events around the call: packing of the geometry on the host
                and the launch); and with a geometry packed once (ftpGeometry)
  host call     ftpCloud on a numpy array (upload, kernel, download of 24 bytes per pixel, synchronous; host clock)
  numpy         the same per-pixel arithmetic vectorised in numpy on the host (tests/_ftp_cloud_ref.py; host clock, few calls)
  ftp_phase     ftp_phase_kernel alone at the same size (fc = 0.05, radius_factor = 0.5, as tools/time_ftp.py)
and whether the kernel's map equals the numpy restatement's bit for bit."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12                                    # bytes per second (MI355X specification)
BYTES_PER_PIXEL = 32


def main():
    import torch
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    import _ftp_cloud_ref as R
    from time_ftp import fringes
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_ftp_cloud.py measures on a GPU"
    lib = _native.lib()
    lines = ["ss.active.ftpCloud timing on %s; median of %d calls after warm-up, ms per phase map; z_plane = 1000, period = 12"
             % (torch.cuda.get_device_name(0), args.reps)]

    def median_events(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts)

    def median_clock(fn, warm=2, reps=None):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps or args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts)

    def kernel_alone(fn, slot):
        for _ in range(5):
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
        return statistics.median(ts), min(ts)

    for name, (h, w) in (("1920x1080", (1080, 1920)), ("4096x2160", (2160, 4096))):
        phase = R.smooth_phase(h, w, seed=1)
        tphase = torch.from_numpy(phase).cuda()
        rigs = {d: R.make_rig(ss, R.rig_params(res1=(w, h), dist=d, k1_fx=1500.0 * w / 1280, k1_fy=1500.0 * w / 1280)) for d in ("none", "d5", "d8", "d12")}
        rig = rigs["d8"]
        z_plane, period, k = 1000.0, 12.0, 2.0
        packed = ss.active.ftpGeometry(rig, z_plane, period)
        got = ss.active.ftpCloud(tphase, packed, k=k).cpu().numpy()
        want = R.cloud_from_geometry(packed.geom, phase, k, 0, 0)
        same = np.array_equal(got.view(np.uint64), want.view(np.uint64))
        floor = BYTES_PER_PIXEL * h * w / HBM_PEAK * 1e3

        per_model = {d: kernel_alone(lambda d=d: ss.active.ftpCloud(tphase, rigs[d], z_plane, period, k), _native.K_REPROJECT)
                     for d in rigs}
        t_kernel, t_kernel_min = per_model["d8"]
        t_dev = median_events(lambda: ss.active.ftpCloud(tphase, rig, z_plane, period, k))
        t_dev_packed = median_events(lambda: ss.active.ftpCloud(tphase, packed, k=k))
        t_host = median_clock(lambda: ss.active.ftpCloud(phase, packed, k=k))
        t_numpy = median_clock(lambda: R.cloud_from_geometry(packed.geom, phase, k, 0, 0), warm=1, reps=3)
        obj, ref = fringes(h, w, 0.05, 1)
        tobj, tref = torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda()
        t_ftp, _ = kernel_alone(lambda: ss.active.ftpPhase(tobj, tref, 0.05, 0.5), _native.K_FTP)

        lines += ["", "%s  (%d pixels; the 32 bytes per pixel take %.4f ms at the 8.0 TB/s HBM peak)" % (name, h * w, floor),
                  "  kernel alone (ftp_cloud_kernel, 8 coeff.) %9.4f   (fastest %.4f; %.0f %% of the HBM roofline, %.2f TB/s)"
                  % (t_kernel, t_kernel_min, 100 * floor / t_kernel, BYTES_PER_PIXEL * h * w / t_kernel * 1e-9)]
        lines += ["  kernel alone, %-28s %9.4f   (%.0f %% of the HBM roofline)" % (label, per_model[d][0], 100 * floor / per_model[d][0])
                  for d, label in (("none", "no distortion"), ("d5", "5 coefficients"), ("d12", "12 coefficients (thin prism)"))]
        lines += ["  device-tensor call                        %9.4f   (geometry packed on the host in every call)" % t_dev,
                  "  device-tensor call, ftpGeometry once      %9.4f" % t_dev_packed,
                  "  host-array call (copies included)         %9.3f" % t_host,
                  "  numpy restatement on the host             %9.1f" % t_numpy,
                  "  ftp_phase_kernel alone, same size         %9.4f   (the cloud kernel takes %.2f of it)" % (t_ftp, t_kernel / t_ftp),
                  "  kernel's cloud equals the numpy restatement's bit for bit: %s" % same]
        print("\n".join(lines[-12:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
