"""
_rigs
=====
Stereo rig parameter containers with the API of ``simplestereo.StereoRig`` /
``simplestereo.RectifiedStereoRig`` (reference ``simplestereo/_rigs.py:22-338``,
``341-628``) and ``simplestereo.StructuredLightRig`` (``631-715``) -- the plumbing that feeds rectified pairs to ``passive.StereoASW``
(``examples/009 StereoMatchingASW.py:20-39``).

Own code, numpy only: OpenCV is not a dependency (it is absent on the MI355X
image).  Where the reference calls OpenCV, the published OpenCV camera model is
restated here:

====================================  ==========================================
reference call                         restated by
====================================  ==========================================
cv2.undistortPoints (4 corners)        :func:`_undistort_points`
cv2.initUndistortRectifyMap            :func:`_init_undistort_rectify_map`
cv2.remap (constant border)            :func:`_remap`
cv2.reprojectImageTo3D                 :meth:`RectifiedStereoRig.get3DPoints`
cv2.perspectiveTransform,              :meth:`StructuredLightRig.triangulate`
cv2.undistortPoints (every point)      (``sl_triangulate_kernel``)
cv2.undistort                          :meth:`StructuredLightRig.undistortCameraImage`
====================================  ==========================================

Parity status: JSON round trip and the 3x3 algebra are pinned by the reference's
own rig files (loaded as data in the tests); pixel values of ``rectifyImages`` can
not be pinned against cv2 in this environment ("parity unpinned"):
they are checked by self-consistency on synthetic rigs instead.
"""
import json

import numpy as np

from . import _native
from ._native import is_device_tensor as _is_device_tensor

__all__ = ["StereoRig", "RectifiedStereoRig", "StructuredLightRig"]

# OpenCV interpolation flag values, so callers can pass cv2.INTER_* or these
INTER_NEAREST = 0
INTER_LINEAR = 1
INTER_CUBIC = 2


def _dist_vector(d):
    """OpenCV order (k1,k2,p1,p2[,k3[,k4,k5,k6[,s1,s2,s3,s4[,tx,ty]]]]) padded to 14."""
    v = np.zeros(14)
    d = np.asarray(d, dtype=np.float64).ravel()
    if d.size not in (0, 4, 5, 8, 12, 14):
        raise ValueError("distortion coefficients must have 4, 5, 8, 12 or 14 elements")
    v[:d.size] = d
    if v[12] != 0 or v[13] != 0:
        raise NotImplementedError("tilted sensor model (tauX, tauY) is not supported")
    return v


def _distort(x, y, dist):
    """Apply the OpenCV radial/tangential/thin-prism model to normalised coordinates."""
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = dist[:12]
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    kr = (1 + k1 * r2 + k2 * r4 + k3 * r6) / (1 + k4 * r2 + k5 * r4 + k6 * r6)
    xd = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r4
    yd = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r4
    return xd, yd


def _undistort_points(pts, K, distCoeffs, R=None, iterations=5):
    """cv2.undistortPoints semantics: pixel -> normalised, iterative undistortion, then R.
    ``iterations`` = 5 is OpenCV's default termination (TermCriteria(MAX_ITER, 5, 0.01) in cv::undistortPoints,
    modules/calib3d/src/undistort.dispatch.cpp), which the reference's ``_getCorners`` inherits
    (reference rectification.py:125-156)."""
    K = np.asarray(K, dtype=np.float64)
    dist = _dist_vector(distCoeffs)
    pts = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    x0 = (pts[:, 0] - K[0, 2]) / K[0, 0]
    y0 = (pts[:, 1] - K[1, 2]) / K[1, 1]
    x, y = x0.copy(), y0.copy()
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = dist[:12]
    for _ in range(iterations):
        r2 = x * x + y * y
        icdist = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x) + s1 * r2 + s2 * r2 * r2
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y + s3 * r2 + s4 * r2 * r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    if R is not None:
        R = np.asarray(R, dtype=np.float64)
        X = R[0, 0] * x + R[0, 1] * y + R[0, 2]
        Y = R[1, 0] * x + R[1, 1] * y + R[1, 2]
        Wc = R[2, 0] * x + R[2, 1] * y + R[2, 2]
        x, y = X / Wc, Y / Wc
    return np.stack([x, y], axis=1)


def _init_undistort_rectify_map(K, distCoeffs, R, newK, size):
    """cv2.initUndistortRectifyMap(..., CV_32FC1): float32 (mapx, mapy) of shape (h, w)."""
    K = np.asarray(K, dtype=np.float64)
    dist = _dist_vector(distCoeffs)
    w, h = int(size[0]), int(size[1])
    iR = np.linalg.inv(np.asarray(newK, dtype=np.float64)[:3, :3].dot(np.asarray(R, dtype=np.float64)))
    u, v = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    X = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
    Y = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
    Wc = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
    x, y = X / Wc, Y / Wc
    xd, yd = _distort(x, y, dist)
    mapx = K[0, 0] * xd + K[0, 2]
    mapy = K[1, 1] * yd + K[1, 2]
    return mapx.astype(np.float32), mapy.astype(np.float32)


_CUBIC_TABLE = None


def _cubic_table():
    """OpenCV's ``initInterTab2D(INTER_CUBIC, fixpt)`` as published (modules/imgproc/src/imgwarp.cpp): int16
    ``[32 (fy), 32 (fx), 4 (tap row), 4 (tap column)]``, the 15-bit weights of ``cv2.remap(INTER_CUBIC)`` on 8-bit images.
    OpenCV's source is not available where this is built, so every choice is stated, from its published arithmetic:

    * ``interpolateCubic`` in float32 with ``A = -0.75`` at the fractions ``x = i / 32``: ``c0 = ((A(x+1) - 5A)(x+1) + 8A)(x+1) - 4A``,
      ``c1 = ((A+2)x - (A+3))x x + 1``, ``c2`` = the same of ``1 - x``, ``c3 = 1 - c0 - c1 - c2`` (each operation is exact in
      float32 at these fractions, so neither its order nor a fused multiply-add changes a bit);
    * the float32 product ``c[fy][k1] * c[fx][k2]`` times 32768, rounded half to even and saturated to int16
      (``saturate_cast<short>``): the one product that is 1.0, at the fractions (0, 0), becomes 32767 and the correction below
      puts the missing 1 on tap (2, 2) -- still the identity on 8-bit values, ``(32767 a + b + 16384) >> 15 == a``;
    * where the 16 weights do not sum to 32768, the difference is taken from ONE of them, searched over the taps
      ``k1, k2 in {2, 3}`` (``ksize / 2 .. ksize / 2 + 1``, as OpenCV writes the loop -- not the four central taps 1..2): the
      largest when the sum is short, the smallest when it is over; the scan starts with both at ``(2, 2)`` and tests "smaller
      than the minimum" first and "larger than the maximum" only otherwise.

    Which entry takes the correction is recalled, not verified: parity with cv2 stays unpinned (tests/test_cv2_pins_ftp.py
    pins it wherever cv2 exists).  ``csrc/host_ftp_reference.h`` builds the same table for ``ftp_reference_kernel``."""
    global _CUBIC_TABLE
    if _CUBIC_TABLE is None:
        f = np.float32
        A = f(-0.75)
        x = np.arange(32, dtype=np.float32) * f(1.0 / 32)
        c = np.empty((32, 4), np.float32)
        c[:, 0] = ((A * (x + f(1)) - f(5) * A) * (x + f(1)) + f(8) * A) * (x + f(1)) - f(4) * A
        c[:, 1] = ((A + f(2)) * x - (A + f(3))) * x * x + f(1)
        c[:, 2] = ((A + f(2)) * (f(1) - x) - (A + f(3))) * (f(1) - x) * (f(1) - x) + f(1)
        c[:, 3] = f(1) - c[:, 0] - c[:, 1] - c[:, 2]
        v = c[:, None, :, None] * c[None, :, None, :]                      # [fy, fx, k1, k2], float32 products
        tab = np.clip(np.rint(v * f(32768)).astype(np.int64), -32768, 32767)      # saturate_cast<short>: 1.0 -> 32767
        for i in range(32):
            for j in range(32):
                t = tab[i, j]
                diff = int(t.sum()) - 32768
                if diff == 0:
                    continue
                mn = mx = (2, 2)
                for k in ((2, 2), (2, 3), (3, 2), (3, 3)):
                    if t[k] < t[mn]:
                        mn = k
                    elif t[k] > t[mx]:
                        mx = k
                t[mx if diff < 0 else mn] -= diff
        _CUBIC_TABLE = tab.astype(np.int16)
        _CUBIC_TABLE.setflags(write=False)
    return _CUBIC_TABLE


def _remap(img, mapx, mapy, interpolation=INTER_LINEAR):
    """cv2.remap with BORDER_CONSTANT(0), restating OpenCV's published arithmetic
    (modules/imgproc/src/imgwarp.cpp: ``remap`` converts float maps with ``cvRound(map * INTER_TAB_SIZE)``,
    INTER_BITS = 5; ``initInterTab2D`` builds 15-bit integer weights, INTER_REMAP_COEF_BITS = 15 -- with 5-bit
    fractions they are exactly a*b*32 and sum to 32768; ``remapBilinear`` for uint8 ends in
    ``FixedPtCast<int, uchar, 15>``: ``(sum + (1 << 14)) >> 15``, so ties round UP, not to even).
    uint8 images take that fixed-point path, with the common factor 32 divided out: ``(S + 512) >> 10``.  Every other
    dtype goes the way of OpenCV's non-uchar instantiations: float32 weights ``(1-fy)(1-fx)`` ... from the 1/32-pixel
    fractions, a float32 sum in tap order, and for uint16 / int16 ... ``saturate_cast`` = round half to EVEN
    (``np.rint``) + clip; float images keep the float sum.
    Coordinates outside every range -- NaN, +-inf, and anything whose product with 32 leaves the int32 range (2^26 and beyond)
    -- sample nothing and give the border value 0: OpenCV's path is ``saturate_cast<short>(cvRound(v * 32) >> 5)`` and
    ``cvRound`` of NaN or of an out-of-range double is INT_MIN on x86, a cell far outside the image.  Here the conversion
    to int64 sends NaN / +-inf / beyond-int64 values to INT64_MIN and keeps the others as huge cells, outside the image
    either way; the HIP kernels test for them explicitly (``remap_pixel``); ``oracle/rig_oracle.py`` states the rule.
    INTER_CUBIC (2) is restated for uint8 images only (``remapBicubic`` with the table of :func:`_cubic_table`).
    cv2 is absent in this environment: parity with cv2.remap
    itself stays unpinned here (reference call: _rigs.py:564-565) -- tests/test_cv2_pins.py pins it wherever cv2 exists."""
    img = np.asarray(img)
    squeeze = img.ndim == 2
    src = img[:, :, None] if squeeze else img
    H, W = src.shape[:2]
    if interpolation == INTER_NEAREST:
        xi = np.rint(mapx).astype(np.int64)
        yi = np.rint(mapy).astype(np.int64)
        ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
        out = np.zeros(mapx.shape + (src.shape[2],), src.dtype)
        out[ok] = src[yi[ok], xi[ok]]
    elif interpolation == INTER_LINEAR:
        q = np.rint(mapx.astype(np.float64) * 32).astype(np.int64)
        r = np.rint(mapy.astype(np.float64) * 32).astype(np.int64)
        x0, fx = q >> 5, q & 31
        y0, fy = r >> 5, r & 31
        fixed = src.dtype == np.uint8                       # OpenCV's 15-bit FixedPtCast path exists for uchar only
        acc = np.zeros(mapx.shape + (src.shape[2],), np.int64 if fixed else (np.float64 if src.dtype == np.float64 else np.float32))
        for dy, wy in ((0, 32 - fy), (1, fy)):
            for dx, wx in ((0, 32 - fx), (1, fx)):
                xx, yy = x0 + dx, y0 + dy
                ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                val = np.zeros_like(acc)
                val[ok] = src[yy[ok], xx[ok]]
                if fixed:
                    acc += val * (wy * wx)[..., None]      # a*b in 0..1024
                else:                                       # float32 weights a*b/1024 (exact), float32 products and sum
                    acc = acc + val * ((wy * wx).astype(np.float32) * np.float32(1.0 / 1024.0)).astype(acc.dtype)[..., None]
        if fixed:
            out = np.clip((acc + 512) >> 10, 0, 255).astype(np.uint8)
        elif np.issubdtype(src.dtype, np.integer):
            info = np.iinfo(src.dtype)
            out = np.clip(np.rint(acc), info.min, info.max).astype(src.dtype)      # saturate_cast: ties to even
        else:
            out = acc.astype(src.dtype)
    elif interpolation == INTER_CUBIC:
        # remapBicubic for uchar: 4 x 4 taps at cell - 1 .. cell + 2 with the 15-bit weights of _cubic_table, taps outside the
        # image 0, FixedPtCast<int, uchar, 15>: saturate((sum + (1 << 14)) >> 15)
        if src.dtype != np.uint8:
            raise NotImplementedError("INTER_CUBIC (2) is available for uint8 images only without OpenCV")
        with np.errstate(invalid="ignore", over="ignore"):
            q = np.rint(mapx.astype(np.float64) * 32).astype(np.int64)
            r = np.rint(mapy.astype(np.float64) * 32).astype(np.int64)
        wt = _cubic_table()[r & 31, q & 31].astype(np.int64)              # [..., 4, 4]
        x0, y0 = (q >> 5) - 1, (r >> 5) - 1
        acc = np.zeros(mapx.shape + (src.shape[2],), np.int64)
        for k1 in range(4):
            for k2 in range(4):
                xx, yy = x0 + k2, y0 + k1
                ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                val = np.zeros_like(acc)
                val[ok] = src[yy[ok], xx[ok]]
                acc += val * wt[..., k1, k2][..., None]
        out = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
    else:
        raise NotImplementedError("only INTER_NEAREST (0), INTER_LINEAR (1) and, for uint8, INTER_CUBIC (2) are available without OpenCV")
    return np.ascontiguousarray(out[:, :, 0] if squeeze else out)


def _cross_matrix(v):
    v = np.asarray(v, dtype=np.float64).ravel()
    # float32, as the reference's utils.getCrossProductMatrix (utils.py:229-232) builds it: F carries that rounding
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=np.float32)


def _corners_after(H, K, dims, distCoeffs):
    """Image corners (clockwise from top-left) after undistortion and homography H
    (reference rectification.py:125-156)."""
    w, h = dims
    corners = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], dtype=np.float32)
    out = _undistort_points(corners, K, distCoeffs if distCoeffs is not None else np.zeros(5),
                            R=np.asarray(H).dot(K))
    return [(float(x), float(y)) for x, y in out.astype(np.float32)]


def _fitting_matrix(K1, K2, H1, H2, dims1, dims2, dist1=None, dist2=None, destDims=None, alpha=1):
    """Affine fit of both rectified images into destDims without losing rectification
    (reference rectification.py:17-122: common y scale/offset, common x scale, flips)."""
    if destDims is None:
        destDims = dims1
    c1 = _corners_after(H1, K1, dims1, dist1)
    c2 = _corners_after(H2, K2, dims2, dist2)
    xs1, xs2 = [p[0] for p in c1], [p[0] for p in c2]
    ys = [p[1] for p in c1 + c2]
    minX1, maxX1, minX2, maxX2 = min(xs1), max(xs1), min(xs2), max(xs2)
    minY, maxY = min(ys), max(ys)
    tL1, tR1, _, bL1 = c1
    flipX = -1 if tL1[0] > tR1[0] else 1
    flipY = -1 if tL1[1] > bL1[1] else 1
    spanX = max(maxX2 - minX2, maxX1 - minX1)
    scaleX = flipX * destDims[0] / spanX
    scaleY = flipY * destDims[1] / (maxY - minY)
    tX = -min(minX1, minX2) * scaleX if flipX == 1 else -min(maxX1, maxX2) * scaleX
    tY = -minY * scaleY if flipY == 1 else -maxY * scaleY
    Fit = np.array([[scaleX, 0, tX], [0, scaleY, tY], [0, 0, 1]], dtype=np.float64)
    if alpha >= 1:
        return Fit
    alpha = max(alpha, 0)
    tL1, tR1, bR1, bL1 = _corners_after(Fit.dot(H1), K1, destDims, dist1)
    tL2, tR2, bR2, bL2 = _corners_after(Fit.dot(H2), K2, destDims, dist2)
    left = max(tL1[0], bL1[0], tL2[0], bL2[0])
    right = min(tR1[0], bR1[0], tR2[0], bR2[0])
    top = max(tL1[1], tR1[1], tL2[1], tR2[1])
    bottom = min(bL1[1], bR1[1], bL2[1], bR2[1])
    s = max(destDims[0] / (right - left), destDims[1] / (bottom - top))
    s = (s - 1) * (1 - alpha) + 1
    Kz = np.array([[s, 0, -s * left], [0, s, -s * top], [0, 0, 1]], dtype=np.float64)
    return Kz.dot(Fit)


class StereoRig:
    """
    Keep together and manage all parameters of a calibrated stereo rig
    (same constructor, attributes and JSON keys as ``simplestereo.StereoRig``).

    Parameters
    ----------
    res1, res2 : sequence
        Resolution of camera as (width, height)
    intrinsic1, intrinsic2 : list or numpy.ndarray
        3x3 intrinsic camera matrix in the form [[fx, 0, tx], [0, fy, ty], [0, 0, 1]].
    distCoeffs1, distCoeffs2 : list or numpy.ndarray
        List of distortion coefficients of 4, 5, 8, 12 or 14 elements (OpenCV order).
    R : list or numpy.ndarray.
        3x3 rotation matrix between the 1st and the 2nd camera coordinate systems.
    T : list or numpy.ndarray
        Translation vector between the coordinate systems of the cameras.
    F, E : numpy.ndarray, optional
        Fundamental / essential matrix.
    reprojectionError : float, optional
        Total reprojection error resulting from calibration.
    """

    def __init__(self, res1, res2, intrinsic1, intrinsic2, distCoeffs1, distCoeffs2, R, T, F=None, E=None,
                 reprojectionError=None):
        self.res1 = res1
        self.res2 = res2
        self.intrinsic1 = intrinsic1
        self.intrinsic2 = intrinsic2
        self.distCoeffs1 = distCoeffs1
        self.distCoeffs2 = distCoeffs2
        self.R = R
        self.T = T
        self.F = F
        self.E = E
        self.reprojectionError = reprojectionError

    # ndarray-coercing properties (reference _rigs.py:68-130)
    intrinsic1 = property(lambda s: s._intrinsic1, lambda s, v: setattr(s, "_intrinsic1", np.asarray(v)))
    intrinsic2 = property(lambda s: s._intrinsic2, lambda s, v: setattr(s, "_intrinsic2", np.asarray(v)))
    distCoeffs1 = property(lambda s: s._distCoeffs1,
                           lambda s, d: setattr(s, "_distCoeffs1", np.asarray(d) if d is not None else np.zeros(5)))
    distCoeffs2 = property(lambda s: s._distCoeffs2,
                           lambda s, d: setattr(s, "_distCoeffs2", np.asarray(d) if d is not None else np.zeros(5)))
    R = property(lambda s: s._R, lambda s, v: setattr(s, "_R", np.asarray(v).reshape((3, 3))))
    T = property(lambda s: s._T, lambda s, v: setattr(s, "_T", np.asarray(v).reshape((-1, 1))))
    F = property(lambda s: s._F, lambda s, v: setattr(s, "_F", np.asarray(v).reshape((3, 3)) if v is not None else None))
    E = property(lambda s: s._E, lambda s, v: setattr(s, "_E", np.asarray(v).reshape((3, 3)) if v is not None else None))

    _KEYS = ("res1", "res2", "intrinsic1", "intrinsic2", "distCoeffs1", "distCoeffs2", "R", "T", "F", "E",
             "reprojectionError")

    @classmethod
    def fromFile(cls, filepath):
        """Alternative initialization of StereoRig object from JSON file."""
        with open(filepath, "r") as f:
            data = json.load(f)
        args = [data.get(k) for k in cls._KEYS]
        args[0], args[1] = tuple(args[0]), tuple(args[1])
        return cls(*args)

    def _as_dict(self):
        out = {}
        out["res1"] = self.res1
        out["res2"] = self.res2
        for k in ("intrinsic1", "intrinsic2", "R", "T", "distCoeffs1", "distCoeffs2"):
            out[k] = getattr(self, k).tolist()
        if self.F is not None:
            out["F"] = self.F.tolist()
        if self.E is not None:
            out["E"] = self.E.tolist()
        if self.reprojectionError:
            out["reprojectionError"] = self.reprojectionError
        return out

    def save(self, filepath):
        """Save configuration to JSON file (same keys as the reference, _rigs.py:164-191)."""
        with open(filepath, "w") as f:
            json.dump(self._as_dict(), f, indent=4)

    def getProjectionMatrices(self):
        """3x4 projection matrices of camera 1 and camera 2 (world origin in camera 1)."""
        Po1 = np.hstack((self.intrinsic1, np.zeros((3, 1))))
        Po2 = self.intrinsic2.dot(np.hstack((self.R, self.T)))
        return Po1, Po2

    def getCenters(self):
        """Camera centres in world coordinates (the first is always zero)."""
        _, Po2 = self.getProjectionMatrices()
        return np.zeros(3), -np.linalg.inv(Po2[:, :3]).dot(Po2[:, 3])

    def getBaseline(self):
        """Norm of the vector from camera 1 to camera 2."""
        return np.linalg.norm(self.getCenters()[1])

    def getFundamentalMatrix(self):
        """F (computed from the camera parameters when not set; Hartley & Zisserman form).  The cross-product matrix of
        ``K1 R^T T`` is rounded to float32 before the float64 products, as the reference's
        ``utils.getCrossProductMatrix`` does: F is the reference's bit for bit, 1e-7 relative from the all-float64 value."""
        if self.F is None:
            vv = _cross_matrix(self.intrinsic1.dot(self.R.T).dot(self.T))
            self.F = (np.linalg.inv(self.intrinsic2).T).dot(self.R).dot(self.intrinsic1.T).dot(vv)
        return self.F

    def getEssentialMatrix(self):
        """E = K2^T F K1 when not set.  Computed from :meth:`getFundamentalMatrix`, E inherits its float32 rounding of the
        cross-product matrix, as in the reference."""
        if self.E is None:
            self.E = self.intrinsic2.T.dot(self.getFundamentalMatrix()).dot(self.intrinsic1)
        return self.E


class RectifiedStereoRig(StereoRig):
    """
    A calibrated and rectified stereo rig: all the parameters of :class:`StereoRig` plus the
    common orientation and the two rectifying *homographies* (pixel domain), as in
    ``simplestereo.RectifiedStereoRig``.

    Parameters
    ----------
    Rcommon : numpy.ndarray
        3x3 new common camera orientation after rectification.
    rectHomography1, rectHomography2 : numpy.ndarray
        3x3 rectification homographies.
    StereoRig : StereoRig or sequence
        A StereoRig object or, *alternatively*, all the parameters of :class:`StereoRig` (in order).
    """

    def __init__(self, Rcommon, rectHomography1, rectHomography2, *args):
        self.Rcommon = Rcommon
        self.rectHomography1 = rectHomography1
        self.rectHomography2 = rectHomography2
        self.K1 = None
        self.K2 = None
        if isinstance(args[0], StereoRig):
            r = args[0]
            super().__init__(r.res1, r.res2, r.intrinsic1, r.intrinsic2, r.distCoeffs1, r.distCoeffs2, r.R, r.T,
                             r.F, r.E, r.reprojectionError)
        else:
            super().__init__(*args)
        self.computeRectificationMaps()

    Rcommon = property(lambda s: s._Rcommon, lambda s, v: setattr(s, "_Rcommon", np.asarray(v).reshape((3, 3))))
    rectHomography1 = property(lambda s: s._rectHomography1,
                               lambda s, v: setattr(s, "_rectHomography1", np.asarray(v).reshape((3, 3))))
    rectHomography2 = property(lambda s: s._rectHomography2,
                               lambda s, v: setattr(s, "_rectHomography2", np.asarray(v).reshape((3, 3))))

    @classmethod
    def fromFile(cls, filepath):
        """Alternative initialization from a JSON file written by :meth:`save` (or by the reference)."""
        with open(filepath, "r") as f:
            data = json.load(f)
        head = [data.get(k) for k in ("Rcommon", "rectHomography1", "rectHomography2")]
        return cls(*(head + [data.get(k) for k in StereoRig._KEYS]))

    def save(self, filepath):
        """Save configuration to JSON file (keys as reference _rigs.py:439-469)."""
        out = {"Rcommon": self.Rcommon.tolist(), "rectHomography1": self.rectHomography1.tolist(),
               "rectHomography2": self.rectHomography2.tolist()}
        out.update(self._as_dict())
        with open(filepath, "w") as f:
            json.dump(out, f, indent=4)

    def getRectifiedProjectionMatrices(self):
        """Projection matrices after rectification: common orientation, horizontal displacement only."""
        C1, C2 = self.getCenters()
        P1 = self.K1.dot(self.Rcommon).dot(np.hstack((np.eye(3), -C1[:, None])))
        P2 = self.K2.dot(self.Rcommon).dot(np.hstack((np.eye(3), -C2[:, None])))
        return P1, P2

    def computeRectificationMaps(self, destDims=None, alpha=1):
        """
        Compute the two maps to undistort and rectify the stereo pair (reference
        ``_rigs.py:491-541``): fitting affinity, the new camera matrices ``K1``/``K2`` that
        track every transformation applied after rectification, then the float32 maps
        ``mapx1, mapy1, mapx2, mapy2`` of shape (height, width).
        """
        if destDims is None:
            destDims = self.res1
        Fit = _fitting_matrix(self.intrinsic1, self.intrinsic2, self.rectHomography1, self.rectHomography2,
                              self.res1, self.res2, self.distCoeffs1, self.distCoeffs2, destDims, alpha)
        self.K1 = Fit.dot(self.rectHomography1).dot(self.intrinsic1).dot(self.Rcommon.T)
        self.K2 = Fit.dot(self.rectHomography2).dot(self.intrinsic2.dot(self.R)).dot(self.Rcommon.T)
        R1 = self.Rcommon
        R2 = self.Rcommon.dot(self.R.T)
        self.mapx1, self.mapy1 = _init_undistort_rectify_map(self.intrinsic1, self.distCoeffs1, R1, self.K1, destDims)
        self.mapx2, self.mapy2 = _init_undistort_rectify_map(self.intrinsic2, self.distCoeffs2, R2, self.K2, destDims)
        # device copies of the previous maps are stale (a new array may reuse a freed address) and would stay resident in HBM
        self.__dict__["_maps_gen"] = self.__dict__.get("_maps_gen", 0) + 1
        self.__dict__.pop("_dev_maps", None)

    def rectifyImages(self, img1, img2, interpolation=INTER_LINEAR):
        """
        Undistort, rectify and fit a couple of images coming from the stereo rig.  Returns two
        C-contiguous arrays of the destination resolution, ready for ``StereoASW.compute``.

        Extension: two CUDA/HIP ``torch.uint8 [H,W,3]`` tensors are remapped on the GPU
        (``remap_bgr_kernel``; the maps are uploaded once per rig and device) and returned as
        device tensors, so the rectified pair can go straight into ``compute`` without a host
        round trip.
        """
        if _is_device_tensor(img1) and _is_device_tensor(img2):
            return (self._remap_device(img1, 1, interpolation), self._remap_device(img2, 2, interpolation))
        return (_remap(img1, self.mapx1, self.mapy1, interpolation),
                _remap(img2, self.mapx2, self.mapy2, interpolation))

    def _device_maps(self, which, device):
        """float32 maps of camera `which` (1 / 2) as tensors on `device`, uploaded once per rig, device and map array"""
        import torch
        mx, my = (self.mapx1, self.mapy1) if which == 1 else (self.mapx2, self.mapy2)
        key = (which, str(device), self.__dict__.get("_maps_gen", 0), mx.ctypes.data, mx.shape)
        cache = self.__dict__.setdefault("_dev_maps", {})
        if key not in cache:                      # maps change only through computeRectificationMaps
            cache[key] = (torch.from_numpy(np.ascontiguousarray(mx)).to(device),
                          torch.from_numpy(np.ascontiguousarray(my)).to(device))
        return cache[key]

    def _remap_device(self, img, which, interpolation):
        import torch
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
            raise ValueError("device rectification expects uint8 [H,W,3] tensors")
        if interpolation not in (INTER_NEAREST, INTER_LINEAR):
            raise NotImplementedError("only INTER_NEAREST (0) and INTER_LINEAR (1) are available")
        dmx, dmy = self._device_maps(which, img.device)
        src = img.contiguous()
        h, w = (self.mapx1 if which == 1 else self.mapx2).shape
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=img.device)
        _native.call_on_stream(img, _native.lib().ssamd_remap_bgr_device, src.data_ptr(), int(src.shape[0]), int(src.shape[1]),
                               dmx.data_ptr(), dmy.data_ptr(), h, w, int(interpolation), out.data_ptr())
        return out

    def getQ(self):
        """The 4x4 disparity-to-depth matrix built by the reference in get3DPoints (_rigs.py:604-625)."""
        b = self.getBaseline()
        fx, fy = self.K1[0, 0], self.K2[1, 1]
        cx1, cx2 = self.K1[0, 2], self.K2[0, 2]
        a1, a2 = self.K1[0, 1], self.K2[0, 1]
        cy = self.K1[1, 2]
        Q = np.eye(4, dtype="float64")
        Q[0, 1] = -a1 / fy
        Q[0, 3] = a1 * cy / fy - cx1
        Q[1, 1] = fx / fy
        Q[1, 3] = -cy * fx / fy
        Q[2, 2] = 0
        Q[2, 3] = -fx
        Q[3, 1] = (a2 - a1) / (fy * b)
        Q[3, 2] = 1 / b
        Q[3, 3] = ((a1 - a2) * cy + (cx2 - cx1) * fy) / (fy * b)
        return Q

    def get3DPoints(self, disparityMap):
        """
        3D points (height, width, 3) float32 from a disparity map, world origin in the left camera:
        [X Y Z W]^T = Q [x y d 1]^T, point = (X/W, Y/W, Z/W)  (cv2.reprojectImageTo3D semantics).
        """
        if _is_device_tensor(disparityMap):
            return self._get3DPoints_device(disparityMap)
        d = np.asarray(disparityMap)
        h, w = d.shape[:2]
        Q = self.getQ()
        x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        v = np.stack([x, y, d.astype(np.float64), np.ones_like(x)], axis=-1)
        p = v.dot(Q.T)
        with np.errstate(divide="ignore", invalid="ignore"):
            out = p[..., :3] / p[..., 3:4]
        return out.astype(np.float32)

    def _get3DPoints_device(self, disp):
        """int16 disparity tensor on the GPU -> float32 [H,W,3] point tensor on the GPU (reproject_kernel)."""
        import ctypes
        import torch
        if disp.dtype != torch.int16 or disp.dim() != 2:
            raise ValueError("device reprojection expects an int16 [H,W] tensor")
        d = disp.contiguous()
        h, w = int(d.shape[0]), int(d.shape[1])
        if w % 4 == 0 and d.data_ptr() % 8:
            d = d.clone()         # a view at an odd storage offset: the kernel reads four disparities per 8-byte load
        Q = np.ascontiguousarray(self.getQ(), dtype=np.float64)
        out = torch.empty((h, w, 3), dtype=torch.float32, device=d.device)
        _native.call_on_stream(d, _native.lib().ssamd_reproject_device, d.data_ptr(), h, w,
                               Q.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), out.data_ptr())
        return out


# ------------------------------------------------------------------------------------------------ camera-projector geometry
NGEOM = 68                # SSAMD_FTP_CLOUD_NGEOM


def _low_level_rectify(rig):
    """The rectifying transforms of Fusiello et al. for a camera at the world origin (the reference's ``_lowLevelRectify``,
    ``rectification.py:271-302``): the new x axis along the baseline, y orthogonal to it and to the old z, no new intrinsics."""
    ax = rig.getCenters()[1]
    ay = np.cross([0, 0, 1], ax)
    az = np.cross(ax, ay)
    rot = np.array([ax / np.linalg.norm(ax), ay / np.linalg.norm(ay), az / np.linalg.norm(az)])
    rect1 = rot.dot(np.linalg.inv(rig.intrinsic1))
    rect2 = rot.dot(np.linalg.inv(rig.R)).dot(np.linalg.inv(rig.intrinsic2))
    return rect1, rect2, rot


def _r_inv4(common):
    """The reference's 4 x 4 ``R_inv`` (``active.py:398-401``): the inverse of the common orientation, padded"""
    R_inv = np.eye(4)
    R_inv[:3, :3] = np.linalg.inv(common)
    return R_inv


def _triangulation_geom(rig, dist, rect1, rect2, common_inv):
    """``geom`` with what the triangulation reads (``[12:37]`` and ``[40:68]``: K2, ``distCoeffs2``, the rectifying transforms, the
    inverse common orientation, the baseline) and 0 elsewhere: the part all three geometry builders share"""
    K2 = np.asarray(rig.intrinsic2, dtype=np.float64)
    g = np.zeros(NGEOM)
    g[12:16] = K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2]
    g[16:28] = dist[:12]
    g[28:37] = K2.ravel()
    g[40:49] = rect1.ravel()
    g[49:58] = rect2.ravel()
    g[58:67] = common_inv.ravel()
    g[67] = rig.getBaseline()
    return g


def _triangulation_geometry(rig, rect1, rect2, common_inv):
    """The ``SSAMD_FTP_CLOUD_NGEOM`` doubles of a triangulation alone (``ssamd_graycode_cloud``, ``ssamd_sl_triangulate``):
    :func:`_triangulation_geom` of the rig's own ``distCoeffs2`` and ``getBaseline()``, finite.  Neither the epipole nor a phase
    period is in it, so ``T[2] == 0`` is fine."""
    dist = _dist_vector(rig.distCoeffs2)                          # NotImplementedError for a tilted sensor; None is no distortion
    g = _triangulation_geom(rig, dist, rect1, rect2, common_inv)
    if not np.isfinite(g).all():
        raise ValueError("the rig gives a geometry that is not finite")
    return g


def _undistort_maps(rig, which=1):
    """float32 (mapx, mapy) of ``cv2.undistort(img, K1, distCoeffs1)``: ``initUndistortRectifyMap(K1, D1, I, K1, res1)`` -- with
    ``which=2`` those of the rig's second camera (K2, D2, res2)"""
    if which == 2:
        return _init_undistort_rectify_map(rig.intrinsic2, rig.distCoeffs2, np.eye(3), rig.intrinsic2, rig.res2)
    return _init_undistort_rectify_map(rig.intrinsic1, rig.distCoeffs1, np.eye(3), rig.intrinsic1, rig.res1)


def _cached_maps(cache, rig, device=None, which=1):
    """The float32 (mapx, mapy) of ``cv2.undistort`` of a rig's camera (``which``: 1 or 2), on the host (``device`` None) or as tensors
    on a device, built on first use and kept in ``cache``, the dict ``StereoFTP``, ``GrayCode``, ``GrayCodeStereo`` and
    ``StructuredLightRig`` hold per instance."""
    host, on = ("host", "maps ") if which == 1 else ("host %d" % which, "maps %d " % which)
    if host not in cache:
        cache[host] = _undistort_maps(rig, which)
    if device is None:
        return cache[host]
    if on + str(device) not in cache:
        import torch
        cache[on + str(device)] = tuple(torch.from_numpy(m).to(device) for m in cache[host])
    return cache[on + str(device)]


def _undistort_device(cache, rig, img):
    """``cv2.undistort(img, K1, distCoeffs1)`` of a contiguous uint8 ``[H, W, 3]`` device tensor: ``remap_bgr_kernel`` on the cached
    maps of the rig's camera, on the tensor's current stream -> uint8 ``[res1 height, res1 width, 3]``"""
    import torch
    dmx, dmy = _cached_maps(cache, rig, img.device)
    h, w = int(dmx.shape[0]), int(dmx.shape[1])
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=img.device)
    _native.call_on_stream(img, _native.lib().ssamd_remap_bgr_device, img.data_ptr(), int(img.shape[0]), int(img.shape[1]),
                           dmx.data_ptr(), dmy.data_ptr(), h, w, INTER_LINEAR, out.data_ptr())
    return out


class StructuredLightRig(StereoRig):
    """
    A camera-projector rig with the structured-light methods of ``simplestereo.StructuredLightRig`` (reference
    ``_rigs.py:631-715``): camera in position 1 (world origin), projector in position 2.

    Parameters
    ----------
    r : StereoRig
        The calibrated rig to extend; anything else is ``ValueError("Invalid argument!")``.

    The attributes are the reference's: ``R1`` and ``R2``, the rectifying transforms of ``rectification._lowLevelRectify``
    (no new intrinsics), ``R_inv`` (4 x 4, the inverse of the common orientation, padded) -- and ``R``, which the reference
    overwrites with the common orientation once the transforms are built.  ``getBaseline()`` reads ``R``, so it differs from
    the plain rig's in the last bits; that baseline is the one :meth:`triangulate` uses, as in the reference.
    """

    def __init__(self, r):
        if not isinstance(r, StereoRig):
            raise ValueError("Invalid argument!")
        super().__init__(r.res1, r.res2, r.intrinsic1, r.intrinsic2, r.distCoeffs1, r.distCoeffs2, r.R, r.T, r.F, r.E,
                         r.reprojectionError)
        self._computeMatrices()

    def _computeMatrices(self):
        self.R1, self.R2, self.R = _low_level_rectify(self)
        self.R_inv = _r_inv4(self.R)
        self._cache = {}                          # _cached_maps' entries: the camera's undistortion maps, per device

    @classmethod
    def fromFile(cls, filepath):
        """A StructuredLightRig from the JSON file of a :class:`StereoRig`."""
        return cls(StereoRig.fromFile(filepath))

    def _geometry(self):
        """The ``SSAMD_FTP_CLOUD_NGEOM`` doubles of ``ssamd_sl_triangulate``: K2, ``distCoeffs2``, ``R1``, ``R2``, the inverse common
        orientation and ``getBaseline()`` (computed with the overwritten ``R``)."""
        return _triangulation_geometry(self, self.R1, self.R2, self.R_inv[:3, :3])

    @staticmethod
    def _points(p, name):
        """-> float64 [n, 2], contiguous, where it is (host array or device tensor)"""
        if _is_device_tensor(p):
            import torch
            if p.dtype == torch.bool or p.is_complex():
                raise TypeError("%s must be of a real dtype" % name)
            if p.dim() < 1 or p.shape[-1] != 2:
                raise ValueError("%s: the last dimension must be 2" % name)
            return p.reshape(-1, 2).to(torch.float64).contiguous()
        if not isinstance(p, np.ndarray):
            raise TypeError("%s must be an ndarray or a CUDA/HIP tensor" % name)
        if p.dtype.kind not in "iuf":
            raise TypeError("%s must be of a real dtype" % name)
        if p.ndim < 1 or p.shape[-1] != 2:
            raise ValueError("%s: the last dimension must be 2" % name)
        return np.ascontiguousarray(p.reshape(-1, 2), dtype=np.float64)

    def triangulate(self, camPoints, projPoints):
        """
        Triangulate camera-projector correspondences (reference ``_rigs.py:654-700``), by one HIP kernel
        (``sl_triangulate_kernel``): ``R1`` on the camera points, ``cv2.undistortPoints(projPoints, K2, distCoeffs2, P=K2)``
        (five iterations), ``R2``, ``getBaseline() / |disparity|`` and the common rotation undone -- the operations that end
        ``active.ftpCloud`` and ``active.GrayCode.getCloud``, by the same device function, fp64.

        Parameters
        ----------
        camPoints, projPoints : numpy.ndarray or CUDA/HIP tensor
            Ordered corresponding (x, y) couples of the camera and of the projector, of any real dtype; the last dimension
            must be 2.  Camera points must already be undistorted.  Both on the host or both on one device.  They are
            converted to float64: float32 input gives float64 results (the reference's have float32 precision then).

        Returns
        -------
        numpy.ndarray or tensor
            float64 ``(n, 1, 3)``; three NaN where a projector point holds a NaN.  A tensor on the inputs' device, computed on
            its current stream, for tensors.
        """
        import ctypes
        pc, pp = self._points(camPoints, "camPoints"), self._points(projPoints, "projPoints")
        if _is_device_tensor(pc) != _is_device_tensor(pp) or (_is_device_tensor(pc) and pc.device != pp.device):
            raise TypeError("camPoints and projPoints must both be on the host or both on one device")
        if pc.shape[0] != pp.shape[0]:
            raise ValueError("%d camera points but %d projector points" % (pc.shape[0], pp.shape[0]))
        n = int(pc.shape[0])
        gp = self._geometry().ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        return _native.run("ssamd_sl_triangulate", (pc, pp), (n, 1, 3), lambda c, p, out: (c, p, n, 1, 0, 0, gp, out),
                           (_native.EINVAL, _native.ELIMIT))

    def undistortCameraImage(self, imgObj):
        """
        Undistort a camera image: ``cv2.undistort(imgObj, intrinsic1, distCoeffs1)`` (reference ``_rigs.py:702-715``), as
        ``active.StereoFTP`` undistorts its frames -- the float32 maps of ``initUndistortRectifyMap(K1, D1, I, K1, res1)`` and a
        bilinear remap with a constant border 0.

        Parameters
        ----------
        imgObj : numpy.ndarray or CUDA/HIP tensor
            uint8 ``[H, W]`` or ``[H, W, 3]``.  A host array goes through :func:`_remap`, a device tensor through
            ``remap_bgr_kernel`` (a gray tensor as three equal channels, of which the first is returned: the bilinear
            arithmetic is per channel, so the bytes are the same).

        Returns
        -------
        The undistorted image, of the rig's ``res1``, where the input is.
        """
        if not _is_device_tensor(imgObj):
            mx, my = _cached_maps(self._cache, self)
            return _remap(imgObj, mx, my, INTER_LINEAR)
        import torch
        if imgObj.dtype != torch.uint8 or imgObj.dim() not in (2, 3) or (imgObj.dim() == 3 and imgObj.shape[2] != 3):
            raise ValueError("device undistortion expects a uint8 [H,W] or [H,W,3] tensor")
        gray = imgObj.dim() == 2
        out = _undistort_device(self._cache, self, (imgObj.unsqueeze(2).expand(-1, -1, 3) if gray else imgObj).contiguous())
        return out[:, :, 0].contiguous() if gray else out
