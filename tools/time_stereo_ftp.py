"""Timing of ss.active.StereoFTP on the MI355X: the two kernels of its front end alone, the whole getCloud for a device and a
host frame, the same pipeline in numpy on the host, and ftp_cloud_kernel / ftp_phase_kernel in the same run for scale.

    python tools/time_stereo_ftp.py [--reps 20] [--out profiles/stereo_ftp_timing.txt]

For camera frames of 1920x1080 and 4096x2160 (a 1280x720 projector 160 mm to the camera's side, 8 distortion coefficients on the
projector, a rendered plane at 1000 with a smooth bump, fringe period 12), after warm-up, the MEDIAN over --reps calls of
  ftp_reference_kernel    alone (HIP events around the launch: ssamd_profile_*), with its share of the HBM floor of the bytes it
                          must move (1 written per pixel + the fringe once) and the taps it gathers per second
  stripe_centroid_kernel  alone, with its share of the HBM floor of the 3 bytes per pixel it reads
  ftp_cloud_kernel, ftp_phase_kernel   alone, at the same size, on the maps of the same frame
  getCloud                a device-tensor frame (torch events; host arithmetic of the stripe included) and a host frame (host clock)
  numpy                   the pipeline of tests/_stereo_ftp_ref.py on the host (host clock, one call)
and whether getCloud's reference image equals the restatement's byte for byte."""
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


def main():
    import torch
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    import _ftp_cloud_ref as C
    import _stereo_ftp_ref as S
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1920x1080,4096x2160")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_stereo_ftp.py measures on a GPU"
    lib = _native.lib()
    a = ss.active
    period = 12.0
    fringe = S.build_fringe(period, stripeColor="r")
    lines = ["ss.active.StereoFTP timing on %s; median of %d calls after warm-up, ms per frame; 1280x720 fringe, period 12"
             % (torch.cuda.get_device_name(0), args.reps)]

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
        return statistics.median(ts), min(ts)

    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        rig = C.rig_params(res1=(w, h), dist="d8", k1_fx=1500.0 * w / 640, k1_fy=1500.0 * w / 640)      # the projector lights the whole view
        rig["T"] = [150.0, 10.0, 60.0]
        frame = S.render(rig, period)
        sf = a.StereoFTP(C.make_rig(ss, rig), fringe, period)
        tframe = torch.from_numpy(frame).cuda()
        cut, box, stripe, idx = sf._frame(tframe, None)
        world = sf._triangulate(stripe, sf.stripeCentralPeak, box)
        z_plane, fc = float(np.mean(world[:, 2])), sf._calculateCameraFrequency(world)
        G = a.ftpGeometry(sf.stereoRig, z_plane, period)
        tfringe = torch.from_numpy(sf.fringe).cuda()
        ref = a.ftpReference(tfringe, G)
        phase = a.ftpPhase(cut, ref, fc, 0.5, unwrap="numpy")
        k = a.ftpFringeOrder(phase, idx, G, stripeCentralPeak=sf.stripeCentralPeak)

        t_ref, t_ref_min = kernel_alone(lambda: a.ftpReference(tfringe, G), _native.K_REMAP)
        t_stripe, _ = kernel_alone(lambda: a.findCentralStripe(cut, "r", 0.5), _native.K_FTP)
        t_cloud, _ = kernel_alone(lambda: a.ftpCloud(phase, G, k=k), _native.K_REPROJECT)
        t_phase, _ = kernel_alone(lambda: a.ftpPhase(cut, ref, fc, 0.5), _native.K_FTP)
        t_ref_call = median_events(lambda: a.ftpReference(tfringe, G))
        t_stripe_call = median_clock(lambda: a.findCentralStripe(cut, "r", 0.5))
        t_dev = median_events(lambda: sf.getCloud(tframe))
        t_dev_clock = median_clock(lambda: (sf.getCloud(tframe), torch.cuda.synchronize()))
        t_host = median_clock(lambda: sf.getCloud(frame), warm=1, reps=3)
        t0 = time.perf_counter()
        want = S.pipeline(rig, fringe, period, frame)
        t_numpy = 1e3 * (time.perf_counter() - t0)
        same = np.array_equal(ref.cpu().numpy(), want["ref"]) and z_plane == want["z_plane"]

        ref_floor = (h * w + fringe.shape[0] * fringe.shape[1]) / HBM_PEAK * 1e3
        stripe_floor = 3 * h * w / HBM_PEAK * 1e3
        lines += ["", "%s  (%d pixels; z_plane %.1f, k %g)" % (size, h * w, z_plane, k),
                  "  ftp_reference_kernel alone (8 coeff.)      %9.4f   (fastest %.4f; %.1f %% of its HBM floor %.4f; %.0f G taps/s; %.2f x ftp_cloud_kernel)"
                  % (t_ref, t_ref_min, 100 * ref_floor / t_ref, ref_floor, 16 * h * w / t_ref * 1e-6, t_ref / t_cloud),
                  "  stripe_centroid_kernel alone               %9.4f   (%.0f %% of its HBM floor %.4f, %.2f TB/s)"
                  % (t_stripe, 100 * stripe_floor / t_stripe, stripe_floor, 3 * h * w / t_stripe * 1e-9),
                  "  ftp_cloud_kernel alone, same size          %9.4f" % t_cloud,
                  "  ftp_phase_kernel alone, same size          %9.4f" % t_phase,
                  "  ftpReference, device-tensor call           %9.4f" % t_ref_call,
                  "  findCentralStripe, device frame (host clock, fill included) %9.4f" % t_stripe_call,
                  "  getCloud, device-tensor frame              %9.3f   (torch events; host clock with a final synchronisation %.3f)" % (t_dev, t_dev_clock),
                  "  getCloud, host frame (numpy undistort, copies included) %9.1f" % t_host,
                  "  numpy pipeline on the host                 %9.1f" % t_numpy,
                  "  reference image and z_plane equal the numpy pipeline's bit for bit: %s" % same]
        print("\n".join(lines[-12:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
