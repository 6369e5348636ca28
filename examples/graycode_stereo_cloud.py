"""Conventional active stereo -- two calibrated cameras, one uncalibrated projector -- from two stacks of camera images to a point
cloud with ss.active.GrayCodeStereo: decode of both stacks, inversion of both camera -> projector maps, triangulation camera
against camera.

    python examples/graycode_stereo_cloud.py [--size 480 640] [--device]

The scene is a tilted plane about 1000 in front of two cameras 120 apart, lit by the patterns of ss.active.grayCodePattern((320, 180))
from a projector between them whose calibration nobody knows: it only paints a code on the surface.  The stacks are rendered from
the geometry itself: every camera pixel shows, in every pattern image, the value of the projector pixel that lights the surface
seen there.  The cameras out-resolve the projector (a projector pixel covers about a dozen camera pixels), so the choice of the camera
pixel that stands for a projector pixel matters: reduce="last" takes the last one in raster order, a corner of the patch, in
either camera; reduce="mean" takes the centroid of the patch.  The residual of a plane fitted to the cloud shows the difference."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import simplestereo_amd as ss      # noqa: E402

PLANE_N, PLANE_D = np.array([0.12, -0.05, 1.0]), 1000.0      # the surface: PLANE_N . X = PLANE_D in the frame of camera 1


def render(K, R, T, res, patterns, proj):
    """uint8 [N, h, w]: the pattern images as a camera with X_cam = R X + T sees them on the plane; proj = (Kp, Rp, Tp, (wp, hp))"""
    w, h = res
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    rays = np.stack([(x + 0.5 - K[0, 2]) / K[0, 0], (y + 0.5 - K[1, 2]) / K[1, 1], np.ones((h, w))], axis=-1).dot(R)      # R^T d: world directions
    centre = -R.T.dot(T)
    t = (PLANE_D - PLANE_N.dot(centre)) / rays.dot(PLANE_N)
    X = centre + rays * t[..., None]
    Kp, Rp, Tp, (wp, hp) = proj
    p = X.dot(Rp.T) + Tp
    u, v = Kp[0, 0] * p[..., 0] / p[..., 2] + Kp[0, 2], Kp[1, 1] * p[..., 1] / p[..., 2] + Kp[1, 2]
    lit = (u >= 0) & (u < wp) & (v >= 0) & (v < hp)
    ui, vi = np.where(lit, np.floor(u), 0).astype(int), np.where(lit, np.floor(v), 0).astype(int)
    return np.where(lit[None], 30 + (patterns[:, vi, ui] // 255) * 180, 30).astype(np.uint8)


def plane_residual(points):
    """RMS distance of the points from their least-squares plane"""
    p = points.reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    c = p - p.mean(axis=0)
    return float(np.sqrt(np.linalg.svd(c, compute_uv=False)[-1] ** 2 / p.shape[0]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[480, 640], metavar=("H", "W"))
    ap.add_argument("--device", action="store_true", help="hand the stacks over as torch tensors in HBM; the cloud stays there")
    args = ap.parse_args()
    h, w = args.size
    dims = (320, 180)
    rot = lambda deg: np.array([[np.cos(np.deg2rad(deg)), 0, np.sin(np.deg2rad(deg))], [0, 1, 0], [-np.sin(np.deg2rad(deg)), 0, np.cos(np.deg2rad(deg))]])      # noqa: E731
    f = 1500.0 * w / 640
    K1 = np.array([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]])
    K2 = np.array([[1.02 * f, 0, w / 2 + 3.5], [0, 1.02 * f, h / 2 - 2.25], [0, 0, 1]])
    R, T = rot(-6.0), np.array([-120.0, 4.0, 9.0])
    rig = ss.StereoRig((w, h), (w, h), K1, K2, np.zeros(5), np.zeros(5), R, T)
    projector = (np.array([[420.0, 0, 160.0], [0, 420.0, 90.0], [0, 0, 1]]), rot(-3.0), np.array([-60.0, -30.0, 5.0]), dims)

    patterns = ss.active.grayCodePattern(dims)
    stacks = (render(K1, np.eye(3), np.zeros(3), (w, h), patterns, projector), render(K2, R, T, (w, h), patterns, projector))
    images = stacks
    if args.device:
        import torch
        images = tuple(torch.from_numpy(s).cuda() for s in stacks)
    for reduce in ("last", "mean"):
        gs = ss.active.GrayCodeStereo(rig, dims, reduce=reduce)
        assert patterns.shape[0] == gs.num_patterns == 34
        cloud = gs.getCloud(images)
        if args.device:
            cloud = cloud.cpu().numpy()
        pts = cloud.reshape(-1, 3)
        off = np.abs(pts.dot(PLANE_N) - PLANE_D) / np.linalg.norm(PLANE_N)
        print("reduce=%-4s  %6d points from 2 x %d images; plane-fit residual %.3f; distance from the scene's plane: mean %.3f, worst %.3f"
              % (reduce, pts.shape[0], stacks[0].shape[0], plane_residual(pts), off.mean(), off.max()))
        assert pts.shape[0] > 1000 and off.mean() < (4.0 if reduce == "last" else 2.0), "the cloud does not follow the scene"


if __name__ == "__main__":
    main()
