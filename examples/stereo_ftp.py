"""Fourier-transform profilometry from one camera frame to a point cloud with ss.active.StereoFTP, the reference's class:
undistortion, central stripe, reference plane, carrier, virtual reference image, phase, fringe order and triangulation.

    python examples/stereo_ftp.py [--size 480 640] [--device]

The scene is a plane at 1000 in front of the camera with a smooth bump of 12 towards the camera on it, lit by
ss.active.buildFringe(12, stripeColor='r') from a projector 160 to the camera's side.  The frame is rendered from the
geometry itself: every camera pixel shows the fringe value at the projector point that lights the surface seen there.
The recovered depth is compared with the scene."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplestereo_amd as ss      # noqa: E402


def render(rig, fringe_dims, period, peak, surface_z):
    """uint8 BGR [h, w, 3]: the fringe with its red central stripe as the camera sees it on the surface z = surface_z(X, Y)
    (no lens distortion in this example)"""
    w, h = rig.res1
    K1, K2 = np.asarray(rig.intrinsic1), np.asarray(rig.intrinsic2)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    nx, ny = (x - K1[0, 2]) / K1[0, 0], (y - K1[1, 2]) / K1[1, 1]
    z = np.full((h, w), 1000.0)
    for _ in range(20):                                             # the ray's point on the surface, by fixed-point iteration
        z = surface_z(nx * z, ny * z)
    p = np.stack([nx * z, ny * z, z], axis=-1).dot(np.asarray(rig.R).T) + np.asarray(rig.T).reshape(1, 1, 3)
    u, v = K2[0, 0] * p[..., 0] / p[..., 2] + K2[0, 2], K2[1, 1] * p[..., 1] / p[..., 2] + K2[1, 2]
    lit = (u >= 0) & (u <= fringe_dims[0] - 1) & (v >= 0) & (v <= fringe_dims[1] - 1)
    img = np.repeat(np.rint(np.where(lit, 255 * (1 + np.cos(2 * np.pi * u / period)) / 2, 0))[..., None], 3, axis=2)
    left = int(peak - period / 2)
    img[(u >= left) & (u < int(left + period)), :2] = 0           # the central stripe keeps the red channel only
    return img.astype(np.uint8), z


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
    ftp = ss.active.StereoFTP(rig, fringe, period, stripeColor="r")
    surface = lambda X, Y: 1000.0 - 12.0 * np.exp(-((X / 60.0) ** 2 + (Y / 45.0) ** 2))      # noqa: E731
    frame, depth = render(rig, dims, period, ftp.stripeCentralPeak, surface)

    if args.device:
        import torch
        frame = torch.from_numpy(frame).cuda()
    cloud = ftp.getCloud(frame)
    if args.device:
        cloud = cloud.cpu().numpy()

    m = w // 8                                                       # the band-pass rings at the row ends
    err = np.abs(cloud[:, m:-m, 2] - depth[:, m:-m])
    print("cloud %s; depth from %.1f to %.1f (plane 1000, top of the bump 988)" % (cloud.shape, cloud[:, m:-m, 2].min(), cloud[:, m:-m, 2].max()))
    print("depth against the scene, away from the row ends: mean |error| %.3f, worst %.3f" % (err.mean(), err.max()))
    assert err.mean() < 1.0, "the cloud does not follow the scene"


if __name__ == "__main__":
    main()
