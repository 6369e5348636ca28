"""Timing of FTP without a reference plane on the MI355X: ftp_carrier_kernel against ftp_phase_kernel, ftp_mapping_cloud_kernel
against ftp_cloud_kernel, and StereoFTP_Mapping.getCloud against StereoFTP.getCloud and against the numpy pipeline.

    python tools/time_ftp_mapping.py [--reps 20] [--out profiles/ftp_mapping_timing.txt]

For camera frames of 1920x1080 and 4096x2160 (the scene of tools/time_stereo_ftp.py: a 1280x720 projector 160 mm to the camera's
side, 8 distortion coefficients on the projector, a rendered plane at 1000 with a smooth bump, fringe period 12), after warm-up,
the MEDIAN over --reps calls of
  ftp_carrier_kernel, ftp_phase_kernel              alone (HIP events around the launch: ssamd_profile_*), fc 0.05 in every row,
                                                    radius_factor 0.5, in the same run, in turns, twice (the lower of the two
                                                    medians of each); the ratio of the two
  ftp_mapping_cloud_kernel, ftp_cloud_kernel        alone, in the same run; the ratio and the share of the HBM floor of the 32 bytes
                                                    per pixel either must move (8 read, 24 written)
  StereoFTP_Mapping.getCloud, StereoFTP.getCloud    a device-tensor frame (torch events; host arithmetic of the stripe included)
                                                    and a host frame (host clock)
  numpy                                             pipeline_mapping of tests/_ftp_mapping_ref.py on the host (host clock, one call)
and whether getCloud's host inputs (stripe, fc) equal the numpy pipeline's bit for bit and its cloud agrees with it."""
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
    import _ftp_mapping_ref as M
    import _stereo_ftp_ref as S
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1920x1080,4096x2160")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_ftp_mapping.py measures on a GPU"
    lib = _native.lib()
    a = ss.active
    period = 12.0
    fringe = S.build_fringe(period, stripeColor="r")
    lines = ["ss.active.StereoFTP_Mapping timing on %s; median of %d calls after warm-up, ms per frame; 1280x720 fringe, period 12"
             % (torch.cuda.get_device_name(0), args.reps),
             "(the four kernels alone at fc 0.05: measured in turns, twice; the lower of each kernel's two medians)"]

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
        srig = C.make_rig(ss, rig)
        sf, sm = a.StereoFTP(srig, fringe, period), a.StereoFTP_Mapping(srig, fringe, period)
        tframe = torch.from_numpy(frame).cuda()
        cut, box, stripe, idx = sf._frame(tframe, None)
        world = sf._triangulate(stripe, sf.stripeCentralPeak, box)
        z_plane, fc = float(np.mean(world[:, 2])), sf._calculateCameraFrequency(world)
        G = a.ftpGeometry(srig, z_plane, period)
        ref = a.ftpReference(torch.from_numpy(sf.fringe).cuda(), G)
        pair = a.ftpPhase(cut, ref, fc, 0.5, unwrap="numpy")
        k = a.ftpFringeOrder(pair, idx, G, stripeCentralPeak=sf.stripeCentralPeak)
        GM = a.ftpMappingGeometry(srig, period)
        one = a.ftpCarrierPhase(cut, fc, 0.5, unwrap="numpy")
        theta = a.ftpStripePhase(one, stripe)

        # in turns, twice: the order of the two does not favour either
        t_car, t_pha, t_map, t_clo = [], [], [], []
        for _ in range(2):
            t_car.append(kernel_alone(lambda: a.ftpCarrierPhase(cut, 0.05, 0.5), _native.K_FTP))
            t_pha.append(kernel_alone(lambda: a.ftpPhase(cut, ref, 0.05, 0.5), _native.K_FTP))
            t_map.append(kernel_alone(lambda: a.ftpMappingCloud(one, GM, stripeCentralPeak=sf.stripeCentralPeak, theta_shift=theta), _native.K_REPROJECT))
            t_clo.append(kernel_alone(lambda: a.ftpCloud(pair, G, k=k), _native.K_REPROJECT))
        (t_car, m_car), (t_pha, m_pha), (t_map, m_map), (t_clo, m_clo) = (min(t) for t in (t_car, t_pha, t_map, t_clo))
        t_car_scene, _ = kernel_alone(lambda: a.ftpCarrierPhase(cut, fc, 0.5), _native.K_FTP)
        t_pha_scene, _ = kernel_alone(lambda: a.ftpPhase(cut, ref, fc, 0.5), _native.K_FTP)
        t_dev = median_events(lambda: sm.getCloud(tframe))
        t_dev_clock = median_clock(lambda: (sm.getCloud(tframe), torch.cuda.synchronize()))
        t_dev_ftp = median_events(lambda: sf.getCloud(tframe))
        t_host = median_clock(lambda: sm.getCloud(frame), warm=1, reps=3)
        t_host_ftp = median_clock(lambda: sf.getCloud(frame), warm=1, reps=3)
        t0 = time.perf_counter()
        want = M.pipeline_mapping(rig, fringe, period, frame)
        t_numpy = 1e3 * (time.perf_counter() - t0)
        got = sm.getCloud(tframe).cpu().numpy()
        same = np.array_equal(stripe, want["stripe"]) and np.array_equal(fc, want["fc"])
        err = float(np.nanmax(C.rel_err(got, want["cloud"].astype(np.longdouble))))
        unwrap_diff = float(np.abs(one.cpu().numpy() - want["phase"]).max())

        floor = 32 * h * w / HBM_PEAK * 1e3
        bins = int(np.floor(0.075 * w) - np.ceil(0.025 * w) + 1)
        lines += ["", "%s  (%d pixels; %d bins of %d at fc 0.05; scene: fc %.4f .. %.4f, theta_shift %.3f)" % (size, h * w, bins, w, fc.min(), fc.max(), theta),
                  "  ftp_carrier_kernel alone, fc 0.05          %9.4f   (fastest %.4f)" % (t_car, m_car),
                  "  ftp_phase_kernel alone, fc 0.05            %9.4f   (fastest %.4f)   carrier / pair = %.3f" % (t_pha, m_pha, t_car / t_pha),
                  "  ... on the scene's own fc                  %9.4f against %.4f       carrier / pair = %.3f" % (t_car_scene, t_pha_scene, t_car_scene / t_pha_scene),
                  "  ftp_mapping_cloud_kernel alone (8 coeff.)  %9.4f   (fastest %.4f; %.1f %% of the HBM floor %.4f of 32 B/pixel, %.2f TB/s)"
                  % (t_map, m_map, 100 * floor / t_map, floor, 32 * h * w / t_map * 1e-9),
                  "  ftp_cloud_kernel alone (8 coeff.)          %9.4f   (fastest %.4f; %.1f %% of that floor)   mapping / cloud = %.3f"
                  % (t_clo, m_clo, 100 * floor / t_clo, t_map / t_clo),
                  "  StereoFTP_Mapping.getCloud, device frame   %9.3f   (torch events; host clock with a final synchronisation %.3f)" % (t_dev, t_dev_clock),
                  "  StereoFTP.getCloud, device frame           %9.3f   mapping / ftp = %.3f" % (t_dev_ftp, t_dev / t_dev_ftp),
                  "  StereoFTP_Mapping.getCloud, host frame (numpy undistort, copies included) %9.1f" % t_host,
                  "  StereoFTP.getCloud, host frame             %9.1f" % t_host_ftp,
                  "  numpy pipeline_mapping on the host         %9.1f   (%.0f x the device frame, %.1f x the host frame)" % (t_numpy, t_numpy / t_dev, t_numpy / t_host),
                  "  stripe and fc equal the numpy pipeline's bit for bit: %s; unwrapped maps differ by %.2e; cloud within %.2e (relative)"
                  % (same, unwrap_diff, err)]
        print("\n".join(lines[-13:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
