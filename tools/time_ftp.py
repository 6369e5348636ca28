"""Timing of ss.active.ftpPhase (ftp_phase_kernel) on the MI355X, beside the same demodulation in numpy on the host (the
reference's way) and as a torch.fft composition on the device.

    python tools/time_ftp.py [--reps 20] [--out profiles/ftp_phase_timing.txt]

For 1920x1080 and 4096x2160 (fc = 0.05, radius_factor = 0.5, synthetic fringes), after warm-up, the MEDIAN over --reps calls of
  kernel        ftp_phase_kernel alone (HIP events around the launch: ssamd_profile_*)
  device call   ftpPhase on uint8 tensors already in HBM (torch events around the call: band planning, band upload, kernel)
  device+iir    the same with unwrap="iir" (the unwrap kernel on top, same stream)
  device+numpy  the same with unwrap="numpy" (np.unwrap along x, then along y: two scan launches on top, same stream)
  unwrap        ss.unwrapping.unwrap of the wrapped map along axis 1 (row form) and along axis 0 (column form), and unwrap2D
                (both), on a tensor in HBM (torch events around the call; the scan kernel alone by ssamd_profile_*), each equal
                to numpy's result bit for bit; unwrap2D also on a steep noisy ramp, where every other sample jumps
  host unwrap   the composition unwrap="numpy" replaces: download of the fp64 map, two np.unwrap calls, upload (host clock
                around work that ends in a synchronise)
  host call     ftpPhase on numpy arrays (uploads, kernel, download, synchronous; host clock)
  numpy         fft / mask / ifft / angle in numpy on the host (host clock)
  torch.fft     max over channels, torch.fft.fft, mask, ifft, angle on the device (torch events), fp64 like the kernel
and the largest angle between the kernel's map and each of the other two."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fringes(h, w, fc, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    bump = 1.5 * np.exp(-(((x - w / 2) / (w / 4)) ** 2 + ((y - h / 2) / (h / 2)) ** 2))
    obj = 128 + 70 * np.cos(2 * np.pi * fc * x + bump) + rng.integers(-3, 4, (h, w))
    ref = 128 + 70 * np.cos(2 * np.pi * fc * x)
    return np.clip(np.rint(obj), 0, 255).astype(np.uint8), np.clip(np.rint(ref), 0, 255).astype(np.uint8)


def numpy_way(obj, ref, fc, rf):
    h, w = obj.shape
    freqs = np.fft.fftfreq(w)
    f = np.full(h, fc)
    radius = rf * f
    low = (freqs.reshape(1, -1) - (f - radius).reshape(-1, 1)) < 0
    high = (freqs.reshape(1, -1) - (f + radius).reshape(-1, 1)) > 0
    G0, G = np.fft.fft(ref, axis=1), np.fft.fft(obj, axis=1)
    for a in (G, G0):
        a[low] = 0
        a[high] = 0
    return np.angle(np.fft.ifft(G, axis=1) * np.conjugate(np.fft.ifft(G0, axis=1)))


def angle_between(a, b):
    d = a - b
    return float(np.abs(np.arctan2(np.sin(d), np.cos(d))).max())


def main():
    import torch
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_ftp.py measures on a GPU"
    lib = _native.lib()
    lines = ["ss.active.ftpPhase timing on %s; median of %d calls after warm-up, ms per frame pair; fc = 0.05, radius_factor = 0.5"
             % (torch.cuda.get_device_name(0), args.reps)]

    def median_events(fn):
        for _ in range(3):
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

    def median_clock(fn, warm=2):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ts)

    for name, (h, w) in (("1920x1080", (1080, 1920)), ("4096x2160", (2160, 4096))):
        fc, rf = 0.05, 0.5
        obj, ref = fringes(h, w, fc, 1)
        tobj, tref = torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda()
        got = ss.active.ftpPhase(tobj, tref, fc, rf)
        torch.cuda.synchronize()

        lib.ssamd_profile_enable(1)
        kern = []
        for _ in range(args.reps):
            lib.ssamd_profile_reset()
            ss.active.ftpPhase(tobj, tref, fc, rf)
            ms, n = _native.profile_read()
            assert n[_native.K_FTP] == 1
            kern.append(ms[_native.K_FTP])
        lib.ssamd_profile_enable(0)
        t_kernel = statistics.median(kern)
        t_dev = median_events(lambda: ss.active.ftpPhase(tobj, tref, fc, rf))
        t_iir = median_events(lambda: ss.active.ftpPhase(tobj, tref, fc, rf, unwrap="iir", tau=0.8))
        t_np = median_events(lambda: ss.active.ftpPhase(tobj, tref, fc, rf, unwrap="numpy"))
        t_ux = median_events(lambda: ss.unwrapping.unwrap(got, axis=1))
        t_uy = median_events(lambda: ss.unwrapping.unwrap(got, axis=0))
        t_uxy = median_events(lambda: ss.unwrapping.unwrap2D(got))
        lib.ssamd_profile_enable(1)
        scan = {0: [], 1: []}
        for _ in range(args.reps):
            for axis in (0, 1):
                lib.ssamd_profile_reset()
                ss.unwrapping.unwrap(got, axis=axis)
                ms, n = _native.profile_read()
                assert n[_native.K_NPUNWRAP] == 1
                scan[axis].append(ms[_native.K_NPUNWRAP])
        lib.ssamd_profile_enable(0)
        k_ux, k_uy = statistics.median(scan[1]), statistics.median(scan[0])
        yy, xx = np.mgrid[0:h, 0:w]
        steep = torch.from_numpy(np.angle(np.exp(1j * (2.9 * (xx + yy) + np.random.default_rng(2).normal(0, 0.1, (h, w)))))).cuda()
        t_steep = median_events(lambda: ss.unwrapping.unwrap2D(steep))
        assert np.array_equal(ss.unwrapping.unwrap2D(steep).cpu().numpy().view(np.uint64),
                              np.unwrap(np.unwrap(steep.cpu().numpy(), axis=1), axis=0).view(np.uint64))

        def host_composition():
            wrapped = got.cpu().numpy()
            unwrapped = np.unwrap(np.unwrap(wrapped, discont=np.pi, axis=1), discont=np.pi, axis=0)
            up = torch.from_numpy(unwrapped).cuda()
            torch.cuda.synchronize()
            return unwrapped, up
        t_hostuw = median_clock(host_composition, warm=1)
        want = host_composition()[0]
        same = all(np.array_equal(a.cpu().numpy().view(np.uint64), b.view(np.uint64)) for a, b in (
            (ss.unwrapping.unwrap2D(got), want), (ss.active.ftpPhase(tobj, tref, fc, rf, unwrap="numpy"), want),
            (ss.unwrapping.unwrap(got, axis=1), np.unwrap(got.cpu().numpy(), axis=1)),
            (ss.unwrapping.unwrap(got, axis=0), np.unwrap(got.cpu().numpy(), axis=0))))
        assert same, "the device unwrap differs from np.unwrap"
        t_host = median_clock(lambda: ss.active.ftpPhase(obj, ref, fc, rf))
        t_numpy = median_clock(lambda: numpy_way(obj, ref, fc, rf), warm=1)

        freqs = torch.fft.fftfreq(w, dtype=torch.float64, device="cuda")
        cut = ((freqs - (fc - rf * fc)) < 0) | ((freqs - (fc + rf * fc)) > 0)

        def torch_way():
            G = torch.fft.fft(tobj.to(torch.float64), dim=1)
            G0 = torch.fft.fft(tref.to(torch.float64), dim=1)
            G[:, cut] = 0
            G0[:, cut] = 0
            return torch.angle(torch.fft.ifft(G, dim=1) * torch.conj(torch.fft.ifft(G0, dim=1)))
        t_torch = median_events(torch_way)

        k = int((~cut).sum().item())
        fma = h * w * k * (4 + 8)                      # forward 2 per term and image, backward 4 per term and image
        lines += ["", "%s  (%d kept bins of %d per row)" % (name, k, w),
                  "  kernel alone (ftp_phase_kernel)        %9.3f   (%.2f fp64 TFMA/s of the %.2e FMAs the two passes need)"
                  % (t_kernel, fma / t_kernel * 1e-9, fma),
                  "  device-tensor call                     %9.3f" % t_dev,
                  "  device-tensor call, unwrap=\"iir\"       %9.3f   (the unwrapper adds %.3f)" % (t_iir, t_iir - t_dev),
                  "  device-tensor call, unwrap=\"numpy\"     %9.3f   (the unwrapper adds %.3f)" % (t_np, t_np - t_dev),
                  "  unwrapping.unwrap axis=1 (row form)    %9.3f   (kernel alone %.3f: %.2f TB/s of the 16 bytes per sample it moves)"
                  % (t_ux, k_ux, 16.0 * h * w / k_ux * 1e-9),
                  "  unwrapping.unwrap axis=0 (column form) %9.3f   (kernel alone %.3f: %.2f TB/s)" % (t_uy, k_uy, 16.0 * h * w / k_uy * 1e-9),
                  "  unwrapping.unwrap2D (both)             %9.3f" % t_uxy,
                  "  unwrapping.unwrap2D, steep noisy ramp  %9.3f   (a jump at about every other sample: the worst case)" % t_steep,
                  "  download + 2 np.unwrap + upload (host) %9.3f   (what unwrap=\"numpy\" replaces; results equal bit for bit)" % t_hostuw,
                  "  host-array call (copies included)      %9.3f" % t_host,
                  "  numpy on the host (the reference's way)%9.3f" % t_numpy,
                  "  torch.fft composition on the device    %9.3f" % t_torch,
                  "  largest angle between the kernel's map and numpy's %.2e, torch.fft's %.2e"
                  % (angle_between(got.cpu().numpy(), numpy_way(obj, ref, fc, rf)),
                     angle_between(got.cpu().numpy(), torch_way().cpu().numpy()))]
        print("\n".join(lines[-15:]), flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
