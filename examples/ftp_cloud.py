"""Fourier-transform profilometry from a synthetic fringe pair to a point cloud, all on the GPU:
ss.active.ftpPhase(unwrap="numpy") demodulates and unwraps, ss.active.ftpFringeOrder finds the fringe order from the central
stripe, ss.active.ftpCloud triangulates the phase.

    python examples/ftp_cloud.py [--size 480 640] [--device]

The scene is the reference plane at z_plane = 1000 with a smooth bump of 30 towards the camera on it.  The fringe images are
synthesised from the geometry itself: the object image shows, at every camera pixel, the projector column that lights the
surface point seen there.  The recovered depth is compared with the bump."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplestereo_amd as ss      # noqa: E402


def projector_column(rig, points):
    """Projector column of 3-D points in the camera's coordinate system (no projector lens distortion in this example)."""
    p = points.dot(np.asarray(rig.R).T) + np.asarray(rig.T).reshape(1, 1, 3)
    K2 = np.asarray(rig.intrinsic2)
    return K2[0, 0] * p[..., 0] / p[..., 2] + K2[0, 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--device", action="store_true", help="keep the images, the phase and the cloud in HBM (torch tensors)")
    args = ap.parse_args()
    h, w = args.size
    z_plane, period, bump_height = 1000.0, 16.0, 30.0
    a = np.deg2rad(-9.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    K1 = np.array([[1500.0, 0, w / 2], [0, 1500.0, h / 2], [0, 0, 1]])
    K2 = np.array([[1500.0, 0, 640.0], [0, 1500.0, 360.0], [0, 0, 1]])
    rig = ss.StereoRig((w, h), (1280, 720), K1, K2, np.zeros(5), np.zeros(5), R, [-250.0, 10.0, 60.0])
    geometry = ss.active.ftpGeometry(rig, z_plane, period)

    # the scene, and what the camera sees of a cosine fringe of that period whose central stripe peaks at column `peak`
    y, x = np.mgrid[0:h, 0:w]
    bump = bump_height * np.exp(-(((x - w / 2) / (w / 5)) ** 2 + ((y - h / 2) / (h / 5)) ** 2))
    rays = np.stack([(x + 0.5 - K1[0, 2]) / K1[0, 0], (y + 0.5 - K1[1, 2]) / K1[1, 1], np.ones((h, w))], axis=-1)
    u_obj = projector_column(rig, rays * (z_plane - bump)[..., None])
    u_ref = projector_column(rig, rays * z_plane)                   # the virtual reference image's columns
    peak = float(np.round(u_ref[h // 2, w // 8]))                   # a stripe away from the bump
    fringe = lambda u: np.clip(np.rint(128 + 70 * np.cos(2 * np.pi * (u - peak) / period)), 0, 255).astype(np.uint8)     # noqa: E731
    obj, ref = fringe(u_obj), fringe(u_ref)
    # the carrier of each row as the camera sees it, and the pixels of the central stripe (the caller's business: in the
    # reference findCentralStripe and _calculateCameraFrequency do this)
    fc = np.abs(np.gradient(u_ref, axis=1)).mean(axis=1) / period
    stripe = np.array([[int(np.argmin(np.abs(u_obj[r] - peak))), r] for r in range(h)])

    if args.device:
        import torch
        obj, ref = torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda()
    phase = ss.active.ftpPhase(obj, ref, fc, unwrap="numpy")
    k = ss.active.ftpFringeOrder(phase, stripe, geometry, stripeCentralPeak=peak)
    cloud = ss.active.ftpCloud(phase, geometry, k=k)
    if args.device:
        cloud = cloud.cpu().numpy()

    m = w // 8                                                       # the band-pass rings at the row ends
    depth = cloud[:, m:-m, 2]
    err = np.abs(depth - (z_plane - bump)[:, m:-m])
    print("fringe order k = %g; depth from %.1f to %.1f (plane %.0f, top of the bump %.1f)" %
          (k + 0.0, depth.min(), depth.max(), z_plane, z_plane - bump_height))
    print("depth against the scene, away from the row ends: mean |error| %.3f, worst %.3f" % (err.mean(), err.max()))
    assert err.mean() < 1.0, "the cloud does not follow the bump"


if __name__ == "__main__":
    main()
