"""Fourier-transform profilometry on a synthetic fringe pair: ss.active.ftpPhase demodulates the object image against the
reference image and unwraps the phase -- with the IIR unwrapper, or with --unwrap numpy as the reference does by default
(np.unwrap along x, then along y) -- all on the GPU.

    python examples/ftp_phase.py [--size 480 640] [--fc 0.08] [--device] [--unwrap iir|numpy]

The object image carries a smooth hill of 4 rad on its fringes; the recovered unwrapped phase is compared with it."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplestereo_amd as ss      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--fc", type=float, default=0.08, help="carrier, cycles per pixel")
    ap.add_argument("--device", action="store_true", help="keep the images and the phase in HBM (torch tensors)")
    ap.add_argument("--unwrap", choices=["iir", "numpy"], default="iir",
                    help="iir: unwrapping.infiniteImpulseResponse (tau 0.8); numpy: the reference's default, unwrapping.unwrap2D")
    args = ap.parse_args()
    h, w = args.size
    rng = np.random.default_rng(0)
    y, x = np.mgrid[0:h, 0:w]
    hill = 4.0 * np.exp(-(((x - w / 2) / (w / 5)) ** 2 + ((y - h / 2) / (h / 5)) ** 2))
    obj = np.clip(np.rint(128 + 70 * np.cos(2 * np.pi * args.fc * x + hill) + rng.normal(0, 2, (h, w))), 0, 255).astype(np.uint8)
    ref = np.clip(np.rint(128 + 70 * np.cos(2 * np.pi * args.fc * x)), 0, 255).astype(np.uint8)
    obj = np.stack([obj // 2, obj, obj // 3], axis=2)          # a BGR camera frame: gray is the channel maximum

    if args.device:
        import torch
        wrapped = ss.active.ftpPhase(torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda(), args.fc).cpu().numpy()
        phase = ss.active.ftpPhase(torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda(), args.fc, unwrap=args.unwrap, tau=0.8)
        phase = phase.cpu().numpy()
    else:
        wrapped = ss.active.ftpPhase(obj, ref, args.fc)
        phase = ss.active.ftpPhase(obj, ref, args.fc, unwrap=args.unwrap, tau=0.8)
    m = w // 10                                                # the band-pass rings at the row ends
    err = np.abs(phase - hill)[:, m:-m]
    print("wrapped phase in [%.3f, %.3f]; unwrapped phase peaks at %.3f rad (hill: %.3f)" %
          (wrapped.min(), wrapped.max(), phase.max(), hill.max()))
    print("unwrapped phase against the hill, away from the row ends: mean |error| %.4f rad, worst %.4f rad" % (err.mean(), err.max()))
    assert err.mean() < 0.1, "the recovered phase does not follow the hill"


if __name__ == "__main__":
    main()
