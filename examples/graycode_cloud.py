"""Gray-code structured light from a stack of camera images to a point cloud with ss.active.GrayCode, the reference's class:
undistortion and decode of every pixel, compaction of the valid ones, triangulation.

    python examples/graycode_cloud.py [--size 480 640] [--device] [--dense]

The scene is a plane at 1000 in front of the camera with a smooth bump of 12 towards the camera on it, lit by the patterns of
ss.active.grayCodePattern((1280, 720)) from a projector 160 to the camera's side.  The stack is rendered from the geometry
itself: every camera pixel shows, in every pattern image, the value of the projector pixel that lights the surface seen there;
where no projector pixel does, the pattern and its inverse are equally dark and the pixel decodes as invalid.  The recovered
depth is compared with the scene: a projector pixel is 1 / 1480 rad wide, which is about 2 in depth at this distance."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplestereo_amd as ss      # noqa: E402


def render(rig, patterns, surface_z):
    """uint8 [N, h, w]: the pattern images as the camera sees them on the surface z = surface_z(X, Y) (no lens distortion in this
    example), and the depth of every camera pixel"""
    w, h = rig.res1
    K1, K2 = np.asarray(rig.intrinsic1), np.asarray(rig.intrinsic2)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    nx, ny = (x + 0.5 - K1[0, 2]) / K1[0, 0], (y + 0.5 - K1[1, 2]) / K1[1, 1]      # the ray through the pixel's centre
    z = np.full((h, w), 1000.0)
    for _ in range(20):                                             # the ray's point on the surface, by fixed-point iteration
        z = surface_z(nx * z, ny * z)
    p = np.stack([nx * z, ny * z, z], axis=-1).dot(np.asarray(rig.R).T) + np.asarray(rig.T).reshape(1, 1, 3)
    u, v = K2[0, 0] * p[..., 0] / p[..., 2] + K2[0, 2], K2[1, 1] * p[..., 1] / p[..., 2] + K2[1, 2]
    lit = (u >= 0) & (u < rig.res2[0]) & (v >= 0) & (v < rig.res2[1])
    ui, vi = np.where(lit, np.floor(u), 0).astype(int), np.where(lit, np.floor(v), 0).astype(int)
    seen = patterns[:, vi, ui]                                       # [N, h, w]: 0 or 255
    stack = np.where(lit[None], 30 + (seen // 255) * 180, 30).astype(np.uint8)
    return stack, z, lit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--device", action="store_true", help="hand the stack over as a torch tensor in HBM; the cloud stays there")
    ap.add_argument("--dense", action="store_true", help="the cloud in the shape of the image, NaN at the invalid pixels")
    args = ap.parse_args()
    h, w = args.size
    dims = (1280, 720)
    a = np.deg2rad(-9.0)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    f = 1500.0 * w / 640
    K1 = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]])
    K2 = np.array([[1480.0, 0, 650.5], [0, 1490.0, 355.25], [0, 0, 1]])
    rig = ss.StereoRig((w, h), dims, K1, K2, np.zeros(5), np.zeros(5), R, [150.0, 10.0, 60.0])

    gc = ss.active.GrayCode(rig)
    patterns = ss.active.grayCodePattern(dims)
    assert patterns.shape[0] == gc.num_patterns == 42
    surface = lambda X, Y: 1000.0 - 12.0 * np.exp(-((X / 60.0) ** 2 + (Y / 45.0) ** 2))      # noqa: E731
    stack, depth, lit = render(rig, patterns, surface)

    images = stack
    if args.device:
        import torch
        images = torch.from_numpy(stack).cuda()
    cloud = gc.getCloud(images, dense=args.dense)
    if args.device:
        cloud = cloud.cpu().numpy()

    if args.dense:
        valid = ~np.isnan(cloud[..., 2])
        z = cloud[..., 2][valid]
    else:
        valid = ss.active.grayCodeDecode(stack, dims)[..., 0] >= 0     # (no lens distortion: the decode of the stack as it is)
        z = cloud[:, 0, 2]
    assert np.array_equal(valid, lit) and z.shape[0] == lit.sum()
    err = np.abs(z - depth[valid])
    print("cloud %s from %d images; %d of %d pixels lit; depth from %.1f to %.1f (plane 1000, top of the bump 988)"
          % (cloud.shape, stack.shape[0], lit.sum(), lit.size, z.min(), z.max()))
    print("depth against the scene: mean |error| %.3f, worst %.3f" % (err.mean(), err.max()))
    assert err.mean() < 1.5 and err.max() < 4.0, "the cloud does not follow the scene"


if __name__ == "__main__":
    main()
