"""Timing of ss.unwrapping.infiniteImpulseResponse (iir_unwrap_kernel) on the MI355X.

    python tools/time_unwrap.py [--out profiles/unwrap_times.json]

Reports ms per map for one 1920x1080 and one 4096x2160 map on the device path (torch tensors, CUDA-event timed, kernel only
plus launch) and the host path (numpy in / out: copies included), maps per second of infiniteImpulseResponseBatch for n = 64 and
256 at 1080p, and the single-map device time at other band caps (SSAMD_UNWRAP_ROWS).  Inputs are random wrapped ramps."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def phase(rng, n, h, w):
    y, x = np.mgrid[0:h, 0:w]
    base = np.fmod(0.09 * x + 0.03 * y, 2 * np.pi)
    return np.ascontiguousarray(base[None] + rng.normal(0, 0.2, (n, h, w)))


def main():
    import torch
    from simplestereo_amd import _native
    from simplestereo_amd import unwrapping as uw
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    res = {"device": torch.cuda.get_device_name(0)}

    def dev_ms(t, fn, reps):
        fn(t)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn(t)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    for name, (h, w) in (("1080p", (1080, 1920)), ("2160p", (2160, 4096))):
        ph = phase(rng, 1, h, w)[0]
        t = torch.from_numpy(ph).cuda()
        res[name + "_device_ms_per_map"] = round(dev_ms(t, lambda x: uw.infiniteImpulseResponse(x, 0.8), args.reps), 3)
        uw.infiniteImpulseResponse(ph, 0.8)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            uw.infiniteImpulseResponse(ph, 0.8)
        res[name + "_host_ms_per_map"] = round(1e3 * (time.perf_counter() - t0) / args.reps, 3)
        print(name, res[name + "_device_ms_per_map"], res[name + "_host_ms_per_map"], flush=True)
    for n in (64, 256):
        t = torch.from_numpy(phase(rng, 4, 1080, 1920)).cuda().repeat(n // 4, 1, 1).contiguous()
        ms = dev_ms(t, lambda x: uw.infiniteImpulseResponseBatch(x, 0.8), 2)
        res["1080p_batch%d_ms" % n] = round(ms, 3)
        res["1080p_batch%d_maps_per_s" % n] = round(n / ms * 1e3, 1)
        print("batch", n, ms, flush=True)
        del t
    t = torch.from_numpy(phase(rng, 1, 1080, 1920)[0]).cuda()
    res["1080p_device_ms_by_band_cap"] = {}
    for cap in (64, 128, 256, 512, 1024):
        with _native.options(SSAMD_UNWRAP_ROWS=cap):
            res["1080p_device_ms_by_band_cap"][cap] = round(dev_ms(t, lambda x: uw.infiniteImpulseResponse(x, 0.8), 3), 3)
    print(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
