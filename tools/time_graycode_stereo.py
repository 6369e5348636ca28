"""Timing of ss.active.GrayCodeStereo on the MI355X: its kernels alone, getCloud for device and host stacks in both reduce modes,
and the numpy restatement on the host.

    python tools/time_graycode_stereo.py [--reps 20] [--out profiles/graycode_stereo_timing.txt]

For two camera stacks of 1920x1080 and two of 4096x2160 with a 1920x1080 projector (N = 44 pattern images; 5 distortion
coefficients per camera; tests/_graycode_ref.scene: a smooth surface, contrast 60, +-2 of noise, a tenth of the pixels with one
washed-out bit), after warm-up, the MEDIAN over --reps calls of
  graycode_decode_kernel        camera 1 alone, with its maps: the yardstick, re-measured in this run (tools/time_graycode.py)
  clear + graycode_scatter      HIP events around the memset of both tables and the scatter kernels (ssamd_profile_*): with both
                                cameras, with one camera's region left empty, and with both empty (the memset alone); a camera's
                                scatter is its run less the memset.  Beside it the updates the kernel issues after the per-thread
                                merge (counted on the host from the decoded map) and the rate they amount to
  graycode_match_kernel         alone (reads both tables, writes 32 B per projector pixel)
  graycode_scan_kernel          alone
  graycode_stereo_cloud_kernel  alone, compacted and dense, and on caller-supplied couples (stereoTriangulate)
  getCloud                      device-tensor stacks, compacted (torch events; the read-back of the count included) and dense, and
                                host stacks (host clock, copies included)
  numpy                         the restatement of tests/_graycode_stereo_ref.py on the host (host clock, one call)
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


def merged_updates(decoded, proj):
    """The updates graycode_scatter_kernel issues for a decoded map: one per run of equal cells inside a thread's four pixels"""
    pw, ph = proj
    d = decoded.reshape(-1, 2).astype(np.int64)
    ok = (d[:, 0] >= 0) & (d[:, 0] < pw) & (d[:, 1] >= 0) & (d[:, 1] < ph)
    cell = np.where(ok, d[:, 1] * pw + d[:, 0], -1)
    cell = np.concatenate([cell, np.full((-cell.size) % 4, -1, np.int64)]).reshape(-1, 4)
    nxt = np.concatenate([cell[:, 1:], np.full((cell.shape[0], 1), -2, np.int64)], axis=1)
    return int(((cell >= 0) & (cell != nxt)).sum()), int(ok.sum())


def main():
    import torch
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    import _graycode_ref as G
    import _graycode_stereo_ref as S
    import _stereo_ftp_ref as F
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="1920x1080,4096x2160")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "time_graycode_stereo.py measures on a GPU"
    lib = _native.lib()
    a = ss.active
    proj = (1920, 1080)
    cells = proj[0] * proj[1]
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

    def kernels_alone(fn, *slots):
        """median time of each profile slot over the calls of fn, which launches once into each"""
        for _ in range(3):
            fn()
        lib.ssamd_profile_enable(1)
        ts = [[] for _ in slots]
        try:
            for _ in range(args.reps):
                lib.ssamd_profile_reset()
                fn()
                ms, n = _native.profile_read()
                for k, slot in enumerate(slots):
                    assert n[slot] == 1, (slot, n)
                    ts[k].append(ms[slot])
        finally:
            lib.ssamd_profile_enable(0)
        return [statistics.median(t) for t in ts]

    n_copy = 1 << 30
    src, dst = torch.empty(n_copy, dtype=torch.uint8, device="cuda"), torch.empty(n_copy, dtype=torch.uint8, device="cuda")
    src.fill_(7)
    copy_bw = 2 * n_copy / (median_events(lambda: dst.copy_(src)) * 1e-3)
    del src, dst
    lines = ["ss.active.GrayCodeStereo timing on %s; median of %d calls after warm-up, ms; two cameras, %d x %d projector, N = %d"
             % (torch.cuda.get_device_name(0), args.reps, proj[0], proj[1], N),
             "HBM floor: the bytes a kernel must move over %.1f TB/s; a 1 GiB device copy reaches %.2f TB/s (read + written) in this run"
             % (HBM_PEAK * 1e-12, copy_bw * 1e-12)]
    ms_of = lambda nbytes, bw: nbytes / bw * 1e3      # noqa: E731

    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        px = h * w
        r = S.two_camera_rig((w, h), (w, h), dist1=[-0.08, 0.03, 0.0005, -0.0004, 0.0], dist2=[-0.06, 0.02, -0.0003, 0.0006, 0.0])
        stacks = (G.scene(7, (w, h), proj, noise=2), G.scene(8, (w, h), proj, noise=2))
        rig = G.make_rig(ss, r)
        tens = tuple(torch.from_numpy(s).cuda() for s in stacks)
        dev = tens[0].device
        gs = {reduce: a.GrayCodeStereo(rig, proj, reduce=reduce) for reduce in ("last", "mean")}
        maps = [ss._rigs._cached_maps(gs["last"]._cache, rig, dev, which=i + 1) for i in range(2)]
        dargs = [a._gray_decode_args(tens[i], gs["last"]._proj, 5, maps[i][0], maps[i][1], (0, 0, w, h)) for i in range(2)]
        decoded = [a._gray_decode_device(tens[i], dargs[i], h, w)[0] for i in range(2)]
        gp = gs["last"]._geometry().ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        nb = a._gray_blocks(proj[1], proj[0])
        matches = torch.empty((proj[1], proj[0], 4), dtype=torch.float64, device=dev)
        counts = torch.empty((nb,), dtype=torch.int32, device=dev)
        offsets = torch.empty((nb + 1,), dtype=torch.int32, device=dev)
        out = torch.empty((cells, 3), dtype=torch.float64, device=dev)
        scratch = torch.empty((2 * ((20 * cells + 7) // 8),), dtype=torch.int64, device=dev)
        host_dec = [d.cpu().numpy() for d in decoded]
        updates = [merged_updates(d, proj) for d in host_dec]

        t_dec = kernels_alone(lambda: a.grayCodeDecode(tens[0], proj, maps=maps[0]), _native.K_FTP)[0]
        lines += ["", "%s per camera  (%d pixels, %.1f %% / %.1f %% valid; %.2f camera pixels per projector pixel)"
                  % (size, px, 100.0 * updates[0][1] / px, 100.0 * updates[1][1] / px, px / cells),
                  "  %-52s %9.4f   (HBM floor %.4f = %.0f %%; %.2f TB/s)"
                  % ("graycode_decode_kernel alone, with maps, camera 1", t_dec, ms_of((N + 16) * px, HBM_PEAK), 100 * ms_of((N + 16) * px, HBM_PEAK) / t_dec,
                     (N + 16) * px / t_dec * 1e-9)]

        def match_call(mode, h1, h2):
            _native.call_on_stream(tens[0], lambda *x: lib.ssamd_graycode_stereo_match_device(*x[:-1], scratch.data_ptr(), x[-1]),
                                   decoded[0].data_ptr(), h1, w, 0, 0, decoded[1].data_ptr(), h2, w, 0, 0, proj[0], proj[1], mode,
                                   matches.data_ptr(), counts.data_ptr())

        n_points = {}
        for reduce, mode in (("last", _native.STEREO_LAST), ("mean", _native.STEREO_MEAN)):
            per_update = 4 if mode == _native.STEREO_LAST else 20
            table = 2 * ((per_update * cells + 7) // 8 * 8)
            t_none, t_match = kernels_alone(lambda: match_call(mode, 0, 0), _native.K_FTP, _native.K_REMAP)
            t_one = [kernels_alone(lambda: match_call(mode, h if i == 0 else 0, h if i == 1 else 0), _native.K_FTP, _native.K_REMAP)[0] for i in range(2)]
            t_both, t_match = kernels_alone(lambda: match_call(mode, h, h), _native.K_FTP, _native.K_REMAP)
            t_scan = kernels_alone(lambda: _native.call_on_stream(tens[0], lib.ssamd_graycode_offsets_device, counts.data_ptr(), nb, offsets.data_ptr()),
                                   _native.K_FTP)[0]
            n = n_points[reduce] = int(offsets[-1].item())
            t_cloud = kernels_alone(lambda: _native.call_on_stream(tens[0], lib.ssamd_graycode_stereo_cloud_device, matches.data_ptr(), proj[0], proj[1], gp,
                                                                   offsets.data_ptr(), out.data_ptr()), _native.K_REPROJECT)[0]
            t_cloud_dense = kernels_alone(lambda: _native.call_on_stream(tens[0], lib.ssamd_graycode_stereo_cloud_device, matches.data_ptr(), proj[0], proj[1],
                                                                         gp, None, out.data_ptr()), _native.K_REPROJECT)[0]
            flat = matches.reshape(-1, 4)
            p1, p2 = flat[:, :2].contiguous(), flat[:, 2:].contiguous()
            t_pairs = kernels_alone(lambda: a.stereoTriangulate(rig, p1, p2), _native.K_REPROJECT)[0]
            t_dev = median_events(lambda: gs[reduce].getCloud(tens))
            t_dev_clock = median_clock(lambda: (gs[reduce].getCloud(tens), torch.cuda.synchronize()))
            t_dense = median_events(lambda: gs[reduce].getCloud(tens, dense=True))
            t_host = median_clock(lambda: gs[reduce].getCloud(stacks), warm=1, reps=3)
            lines += ["  reduce=%s: %d of %d projector pixels matched; the scatter issues %d + %d updates of %d B after the per-thread merge (%.2f / %.2f per valid pixel)"
                      % (reduce, n, cells, updates[0][0], updates[1][0], per_update, updates[0][0] / updates[0][1], updates[1][0] / updates[1][1]),
                      "    %-50s %9.4f   (%d B of tables: %.2f TB/s)" % ("memset of both tables alone", t_none, table, table / t_none * 1e-9)]
            for i in range(2):
                ts = t_one[i] - t_none
                lines.append("    %-50s %9.4f   less the memset %.4f: %.1f G updates/s, %.3f TB/s of atomic bytes; reading its map %.4f at the HBM floor"
                             % ("memset + graycode_scatter_kernel, camera %d" % (i + 1), t_one[i], ts, updates[i][0] / ts * 1e-6,
                                updates[i][0] * per_update / ts * 1e-9, ms_of(8 * px, HBM_PEAK)))
            lines += ["    %-50s %9.4f" % ("memset + both scatters (as getCloud runs them)", t_both),
                      "    %-50s %9.4f   (HBM floor %.4f = %.0f %%: %d B of tables read, 32 B per cell written)"
                      % ("graycode_match_kernel alone", t_match, ms_of(table + 32 * cells, HBM_PEAK), 100 * ms_of(table + 32 * cells, HBM_PEAK) / t_match, table),
                      "    %-50s %9.4f" % ("graycode_scan_kernel alone (%d counts)" % nb, t_scan),
                      "    %-50s %9.4f   (HBM floor %.4f = %.0f %%)" % ("graycode_stereo_cloud_kernel alone, compacted", t_cloud, ms_of(32 * cells + 24 * n, HBM_PEAK),
                                                                      100 * ms_of(32 * cells + 24 * n, HBM_PEAK) / t_cloud),
                      "    %-50s %9.4f   (HBM floor %.4f = %.0f %%)" % ("graycode_stereo_cloud_kernel alone, dense", t_cloud_dense, ms_of(56 * cells, HBM_PEAK),
                                                                      100 * ms_of(56 * cells, HBM_PEAK) / t_cloud_dense),
                      "    %-50s %9.4f   (HBM floor %.4f = %.0f %%)" % ("the same kernel on %d couples (stereoTriangulate)" % cells, t_pairs, ms_of(56 * cells, HBM_PEAK),
                                                                      100 * ms_of(56 * cells, HBM_PEAK) / t_pairs),
                      "    %-50s %9.3f   (torch events; host clock with a final synchronisation %.3f)" % ("getCloud, device-tensor stacks", t_dev, t_dev_clock),
                      "    %-50s %9.3f" % ("getCloud(dense=True), device-tensor stacks", t_dense),
                      "    %-50s %9.1f" % ("getCloud, host stacks (copies included)", t_host),
                      "    scatter of both cameras against the two decodes (2 x the yardstick): %.1f %%" % (100 * (t_both - t_none) / (2 * t_dec))]
            print("\n".join(lines[-14:]), flush=True)

        t0 = time.perf_counter()
        dec = []
        for i, (K, d) in enumerate(((r["intrinsic1"], r["distCoeffs1"]), (r["intrinsic2"], r["distCoeffs2"]))):
            hx, hy = F.undistort_maps(np.array(K), d, (w, h))
            dec.append(G.decode(G.remap_stack_taps_once(stacks[i], hx, hy), proj[0], proj[1], 5))
        t_decode_np = 1e3 * (time.perf_counter() - t0)
        assert np.array_equal(dec[0], host_dec[0]) and np.array_equal(dec[1], host_dec[1])
        for reduce in ("last", "mean"):
            t0 = time.perf_counter()
            want = S.cloud(S.geometry(r), S.match(dec[0], dec[1], proj, reduce))
            t_np = 1e3 * (time.perf_counter() - t0)
            same = G.same_points(gs[reduce].getCloud(tens).cpu().numpy(), want) and want.shape[0] == n_points[reduce]
            lines.append("  numpy restatement on the host, reduce=%s: decode of both stacks %.0f + tables, match and triangulation %.0f; "
                         "the device cloud equals it bit for bit: %s" % (reduce, t_decode_np, t_np, same))
            print(lines[-1], flush=True)
        del tens, decoded, matches, out, scratch
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
