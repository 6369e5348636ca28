"""Classic Fourier-transform profilometry, without a reference plane, with ss.active.StereoFTP_Mapping, the reference's class:
the phase of the camera frame alone is unwrapped, anchored at the central stripe, mapped to a projector column and triangulated
per pixel through the fundamental matrix.  StereoFTP_PhaseOnly returns the wrapped maps of the demodulation on their own.

    python examples/ftp_mapping.py [--size 480 640] [--device]

The scene is the one of examples/stereo_ftp.py: a plane at 1000 in front of the camera with a smooth bump of 12 towards the
camera, lit by ss.active.buildFringe(12, stripeColor='r') from a projector 160 to the camera's side.  The recovered depth is
compared with the scene and with StereoFTP's on the same frame: the classic method anchors the absolute phase at the stripe's
centroid itself, with no rounding to an integer fringe order, so an error in locating the stripe shifts every point (some 17
off at 1000 here, where the method with a virtual reference plane is 0.05 off)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplestereo_amd as ss      # noqa: E402
from stereo_ftp import render      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--device", action="store_true", help="hand the frame over as a torch tensor in HBM; the cloud stays there")
    args = ap.parse_args()
    h, w = args.size
    period, dims = 12.0, (1280, 720)
    a = np.deg2rad(-9.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    f = 1500.0 * w / 640
    K1 = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]])
    K2 = np.array([[1480.0, 0, 650.5], [0, 1490.0, 355.25], [0, 0, 1]])
    rig = ss.StereoRig((w, h), dims, K1, K2, np.zeros(5), np.zeros(5), R, [150.0, 10.0, 60.0])

    fringe = ss.active.buildFringe(period, dims=dims, stripeColor="r")
    ftp = ss.active.StereoFTP_Mapping(rig, fringe, period, stripeColor="r")
    surface = lambda X, Y: 1000.0 - 12.0 * np.exp(-((X / 60.0) ** 2 + (Y / 45.0) ** 2))      # noqa: E731
    frame, depth = render(rig, dims, period, ftp.stripeCentralPeak, surface)

    if args.device:
        import torch
        frame = torch.from_numpy(frame).cuda()
    cloud = ftp.getCloud(frame)
    phase, phase_obj, phase_ref = ss.active.StereoFTP_PhaseOnly(rig, fringe, period, stripeColor="r").getPhase(frame)
    other = ss.active.StereoFTP(rig, fringe, period, stripeColor="r").getCloud(frame)
    if args.device:
        cloud, other, phase, phase_obj, phase_ref = (t.cpu().numpy() for t in (cloud, other, phase, phase_obj, phase_ref))

    m = w // 8                                                       # the band-pass rings at the row ends
    err = np.abs(cloud[:, m:-m, 2] - depth[:, m:-m])
    print("cloud %s; depth from %.1f to %.1f (plane 1000, top of the bump 988)" % (cloud.shape, cloud[:, m:-m, 2].min(), cloud[:, m:-m, 2].max()))
    print("depth against the scene, away from the row ends: mean |error| %.3f, worst %.3f" % (err.mean(), err.max()))
    print("StereoFTP on the same frame: mean |error| %.3f" % np.abs(other[:, m:-m, 2] - depth[:, m:-m]).mean())
    d = phase - (phase_obj - phase_ref)
    print("getPhase: angle(ghat conj(g0hat)) against angle(ghat) - angle(g0hat), worst difference on the circle %.2e"
          % np.abs(np.arctan2(np.sin(d), np.cos(d))).max())
    assert np.isfinite(cloud).all() and err.mean() < 0.05 * 1000.0, "the cloud does not follow the scene"


if __name__ == "__main__":
    main()
