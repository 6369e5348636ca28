"""The reference's Gray-code chain (active.py:23-64 generateGrayCodeImgs, :1130-1263 GrayCode) restated in plain numpy.  Where
the reference calls cv2, OpenCV's published algorithm is written out: GrayCodePattern.generate() and getProjPixel
(structured_light/src/graycodepattern.cpp) -- the latter twice, literally per pixel and vectorised --, cv2.undistort through the
bilinear remap of tests/_stereo_ftp_ref.py, and the triangulation in the operations and the order of
tests/_ftp_cloud_ref.py (cloud_from_geometry, from its undistort_points line to the end).  Seeded generators make the inputs.

Nothing here imports simplestereo_amd."""
import math

import numpy as np

import _ftp_cloud_ref as C
import _stereo_ftp_ref as S

NGEOM = C.NGEOM


# ------------------------------------------------------------------------------------------------ the pattern
def num_bits(n):
    """ceil(log(double(n)) / log(2.0)): numOfColImgs / numOfRowImgs of GrayCodePattern::computeNumberOfPatternImages"""
    return int(math.ceil(math.log(float(n)) / math.log(2.0)))


def num_patterns(width, height):
    return 2 * num_bits(width) + 2 * num_bits(height)


def pattern(width, height):
    """GrayCodePattern::generate(): uint8 [N, height, width], with OpenCV's loops"""
    ncol, nrow = num_bits(width), num_bits(height)
    out = np.zeros((2 * ncol + 2 * nrow, height, width), np.uint8)
    for j in range(width):
        num = j
        prevRem = j % 2
        for k in range(ncol):
            num = num // 2
            rem = num % 2
            flag = 1 if rem != prevRem else 0
            out[2 * ncol - 2 * k - 2, :, j] = flag * 255
            out[2 * ncol - 2 * k - 1, :, j] = 0 if flag else 255
            prevRem = rem
    for i in range(height):
        num = i
        prevRem = i % 2
        for k in range(nrow):
            num = num // 2
            rem = num % 2
            flag = 1 if rem != prevRem else 0
            out[2 * nrow - 2 * k + 2 * ncol - 2, i, :] = flag * 255
            out[2 * nrow - 2 * k + 2 * ncol - 1, i, :] = 0 if flag else 255
            prevRem = rem
    return out


# ------------------------------------------------------------------------------------------------ getProjPixel
def gray_to_dec(gray):
    """grayToDec of graycodepattern.cpp; an empty code (a projector axis of one pixel) is 0"""
    if not gray:
        return 0
    dec = 0
    tmp = gray[0]
    if tmp:
        dec += int(2 ** (len(gray) - 1))
    for i in range(1, len(gray)):
        tmp = tmp ^ gray[i]
        if tmp:
            dec += int(2 ** (len(gray) - i - 1))
    return dec


def get_proj_pixel(images, x, y, width, height, white_thr):
    """getProjPixel, literally: -> (error, (xDec, yDec))"""
    ncol, nrow = num_bits(width), num_bits(height)
    error = False
    codes = []
    for first, count in ((0, ncol), (2 * ncol, nrow)):
        gray = []
        for c in range(count):
            val1 = float(images[first + c * 2][y, x])
            val2 = float(images[first + c * 2 + 1][y, x])
            if abs(val1 - val2) < white_thr:
                error = True
            gray.append(1 if val1 > val2 else 0)
        codes.append(gray_to_dec(gray))
    xDec, yDec = codes
    if yDec >= height or xDec >= width:
        error = True
    return error, (xDec, yDec)


def decode_literal(images, width, height, white_thr):
    h, w = images[0].shape if len(images) else (0, 0)
    out = np.empty((h, w, 2), np.int32)
    for y in range(h):
        for x in range(w):
            err, pix = get_proj_pixel(images, x, y, width, height, white_thr)
            out[y, x] = (-1, -1) if err else pix
    return out


def decode(images, width, height, white_thr, shape=None):
    """getProjPixel for every pixel, vectorised: int32 [H, W, 2], (-1, -1) where it reports an error.  `images` [M >= N, H, W];
    `shape` = (H, W) when there is no image to take it from (N = 0)."""
    ncol, nrow = num_bits(width), num_bits(height)
    images = np.asarray(images)
    H, W = images.shape[1:] if shape is None else shape
    err = np.zeros((H, W), bool)
    codes = []
    for first, count in ((0, ncol), (2 * ncol, nrow)):
        dec = np.zeros((H, W), np.int64)
        tmp = np.zeros((H, W), np.int64)
        for c in range(count):
            v1 = images[first + 2 * c].astype(np.int64)
            v2 = images[first + 2 * c + 1].astype(np.int64)
            err |= np.abs(v1 - v2) < white_thr
            tmp = tmp ^ (v1 > v2)
            dec = dec * 2 + tmp
        codes.append(dec)
    err |= (codes[0] >= width) | (codes[1] >= height)
    out = np.stack(codes, axis=-1).astype(np.int32)
    out[err] = -1
    return out


# ------------------------------------------------------------------------------------------------ cv2.undistort of every plane
def undistort_stack(images, K1, d1, res1):
    """cv2.undistort(img, K1, d1) of every plane: the maps of initUndistortRectifyMap(K1, d1, I, K1, res1) and the 8-bit bilinear
    remap, three planes at a time as the channels of one image"""
    mx, my = S.undistort_maps(np.asarray(K1, dtype=np.float64), d1, tuple(res1))
    return remap_stack(images, mx, my)


def remap_stack(images, mx, my):
    images = np.asarray(images)
    out = np.empty((images.shape[0],) + mx.shape, np.uint8)
    for i in range(0, images.shape[0], 3):
        grp = images[i:i + 3]
        pad = np.concatenate([grp, np.zeros((3 - grp.shape[0],) + grp.shape[1:], np.uint8)]) if grp.shape[0] < 3 else grp
        out[i:i + 3] = np.moveaxis(S.remap_linear(np.ascontiguousarray(np.moveaxis(pad, 0, -1)), mx, my), -1, 0)[:grp.shape[0]]
    return out


def remap_stack_taps_once(images, mx, my):
    """remap_stack with the cells, fractions and border tests of a pixel computed once for all planes: the same bytes
    (tests/test_graycode_cpu.py holds it to remap_stack), at a cost a full frame can afford"""
    images = np.asarray(images)
    H, W = images.shape[1:]
    q, r = S._q32(mx), S._q32(my)
    x0, fx, y0, fy = q >> 5, q & 31, r >> 5, r & 31
    acc = np.zeros((images.shape[0],) + q.shape, np.int64)
    for dy, wy in ((0, 32 - fy), (1, fy)):
        for dx, wx in ((0, 32 - fx), (1, fx)):
            xx, yy = x0 + dx, y0 + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            acc[:, ok] += images[:, yy[ok], xx[ok]].astype(np.int64) * (wy * wx)[ok]
    return ((acc + 512) >> 10).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the triangulation
def geometry(rig):
    """The doubles of the FTP cloud geometry (layout of include/ssamd.h) that the Gray-code triangulation reads, in fp64 as the
    reference computes them (active.py:1167-1171, rectification.py:271-302); M, T, the epipole and 2 pi fp stay 0."""
    K1, K2 = np.array(rig["intrinsic1"], dtype=np.float64), np.array(rig["intrinsic2"], dtype=np.float64)
    R, T = np.array(rig["R"], dtype=np.float64).reshape(3, 3), np.array(rig["T"], dtype=np.float64).reshape(3, 1)
    dist = np.zeros(12)
    d2 = rig["distCoeffs2"] or []
    dist[:len(d2)] = d2
    Po2 = K2.dot(np.hstack((R, T)))
    B = -np.linalg.inv(Po2[:, :3]).dot(Po2[:, 3])
    v2 = np.cross([0, 0, 1], B)
    v3 = np.cross(B, v2)
    Rot = np.array([B / np.linalg.norm(B), v2 / np.linalg.norm(v2), v3 / np.linalg.norm(v3)])
    g = np.zeros(NGEOM)
    g[12:16] = K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2]
    g[16:28] = dist
    g[28:37] = K2.ravel()
    g[40:49] = Rot.dot(np.linalg.inv(K1)).ravel()
    g[49:58] = Rot.dot(np.linalg.inv(R)).dot(np.linalg.inv(K2)).ravel()
    g[58:67] = np.linalg.inv(Rot).ravel()
    g[67] = np.linalg.norm(B)
    return g


def cloud_dense(g, decoded, x0, y0, dtype=np.float64):
    """`dtype` [h, w, 3]: the point of every valid pixel of `decoded` [h, w, 2] (region origin x0, y0), NaN at the invalid ones.
    pc = (x + 0.5, y + 0.5), pp = (xDec + 0.5, yDec + 0.5) (active.py:1236-1237), then the lines of
    _ftp_cloud_ref.cloud_from_geometry from undistort_points to the end, with (Xh, Yh) = pp.  np.float64 is the restatement;
    np.longdouble evaluates the same function of the fp64 geometry as a truth."""
    g = np.asarray(g, dtype=np.float64).astype(dtype)
    h, w = decoded.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    u = (xx + x0).astype(dtype) + dtype(0.5)
    v = (yy + y0).astype(dtype) + dtype(0.5)
    Xh = decoded[..., 0].astype(dtype) + dtype(0.5)
    Yh = decoded[..., 1].astype(dtype) + dtype(0.5)
    with np.errstate(all="ignore"):
        hx, hy = C.undistort_points(g, Xh, Yh)
        R1, R2, Ri, baseline = g[40:49], g[49:58], g[58:67], g[67]
        ppx = ((R2[0] * hx + R2[1] * hy) + R2[2]) / ((R2[6] * hx + R2[7] * hy) + R2[8])
        Wc = (R1[6] * u + R1[7] * v) + R1[8]
        pcx = ((R1[0] * u + R1[1] * v) + R1[2]) / Wc
        pcy = ((R1[3] * u + R1[4] * v) + R1[5]) / Wc
        disparity = np.abs(ppx - pcx)
        px, py, pz = baseline * (pcx / disparity), baseline * (pcy / disparity), baseline * (1 / disparity)
        out = np.stack([(Ri[0] * px + Ri[1] * py) + Ri[2] * pz,
                        (Ri[3] * px + Ri[4] * py) + Ri[5] * pz,
                        (Ri[6] * px + Ri[7] * py) + Ri[8] * pz], axis=-1)
    out[decoded[..., 0] < 0] = np.nan
    return out


def compact(dense, decoded):
    """(n, 1, 3): the points of the valid pixels in raster order, as the reference's lists collect them"""
    return dense[decoded[..., 0] >= 0].reshape(-1, 1, 3)


def same_points(got, want):
    """float64 arrays equal on their bit patterns, NaN where `want` has NaN (any payload or sign)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != np.float64 or want.dtype != np.float64:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    return np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


# ------------------------------------------------------------------------------------------------ rigs and inputs
def rig(res1, res2, dist2="none", dist1=None, T=(-250.0, 10.0, 60.0), R=None, K1=None, K2=None):
    """A camera (position 1) of res1 and a projector (position 2) of res2 to its side, focal lengths in proportion to the widths"""
    w1, h1 = res1
    w2, h2 = res2
    K1 = [[1.2 * w1, 0, w1 / 2 + 0.25], [0, 1.2 * w1, h1 / 2 - 0.5], [0, 0, 1]] if K1 is None else K1
    K2 = [[1.15 * w2, 0, w2 / 2 + 0.5], [0, 1.16 * w2, h2 / 2 + 0.25], [0, 0, 1]] if K2 is None else K2
    return {"res1": [int(w1), int(h1)], "res2": [int(w2), int(h2)], "intrinsic1": np.asarray(K1, dtype=float).tolist(),
            "intrinsic2": np.asarray(K2, dtype=float).tolist(), "distCoeffs1": list(dist1) if dist1 is not None else [0.0] * 5,
            "distCoeffs2": None if dist2 is None else list(C.DIST_MODELS[dist2]),
            "R": (C.rotation(1.5, -9.0, 2.0) if R is None else np.asarray(R, dtype=float)).tolist(), "T": list(T)}


def make_rig(ss, r):
    return ss.StereoRig(tuple(r["res1"]), tuple(r["res2"]), r["intrinsic1"], r["intrinsic2"], r["distCoeffs1"], r["distCoeffs2"], r["R"], r["T"])


def random_stack(seed, n, h, w):
    """Seeded random bytes: a mix of valid pixels, pixels with a low-contrast bit and codes beyond the projector"""
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)


def render(px, py, width, height, contrast, low=20, extra=0):
    """The stack a camera would see if pixel (y, x) looked at projector pixel (px, py)[y, x]: per bit the pattern plane is
    `low + contrast` where the Gray bit is 1 and `low` where it is 0, the inverse plane the other way round.  `contrast` is a
    number, one value per bit (column bits first, MSB first) or an array [bits, H, W]; `extra` planes of 255 follow (ignored)."""
    ncol, nrow = num_bits(width), num_bits(height)
    px, py = np.asarray(px, dtype=np.int64), np.asarray(py, dtype=np.int64)
    c = np.asarray(contrast, dtype=np.int64)
    c = np.broadcast_to(c.reshape(-1, 1, 1) if c.ndim < 3 else c, (ncol + nrow,) + px.shape)
    out = np.full((2 * (ncol + nrow) + extra,) + px.shape, 255, np.uint8)
    b = 0
    for first, count, pos in ((0, ncol, px), (2 * ncol, nrow, py)):
        gray = pos ^ (pos >> 1)
        for i in range(count):
            bit = (gray >> (count - 1 - i)) & 1
            out[first + 2 * i] = low + c[b] * bit
            out[first + 2 * i + 1] = low + c[b] * (1 - bit)
            b += 1
    return out


def scene(seed, res1, res2, noise=0, holes=0.1):
    """A smooth projector coordinate per camera pixel (a tilted plane seen through the rig, roughly), a contrast of 60 with
    +-noise on every byte, and a fraction `holes` of pixels with one washed-out bit: -> uint8 stack [N, H, W]"""
    rng = np.random.default_rng(seed)
    (w1, h1), (w2, h2) = res1, res2
    y, x = np.mgrid[0:h1, 0:w1].astype(np.float64)
    px = np.clip(np.rint((x / w1) * 0.8 * w2 + 0.1 * w2 + 0.02 * w2 * np.sin(y / 23.0)), 0, w2 - 1).astype(np.int64)
    py = np.clip(np.rint((y / h1) * 0.9 * h2 + 0.03 * h2 * np.cos(x / 31.0)), 0, h2 - 1).astype(np.int64)
    nb = num_bits(w2) + num_bits(h2)
    contrast = np.full((nb, h1, w1), 60, np.int64)
    if nb and holes:
        hole = rng.random((h1, w1)) < holes
        which = rng.integers(0, nb, (h1, w1))
        contrast[which[hole], np.nonzero(hole)[0], np.nonzero(hole)[1]] = rng.integers(0, 6, int(hole.sum()))
    out = render(px, py, w2, h2, contrast)
    if noise:
        out = np.clip(out.astype(np.int64) + rng.integers(-noise, noise + 1, out.shape), 0, 255).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ the front of the decode kernels
GRAY_ROW4, GRAY_BYTES, GRAY_TAPS, GRAY_WINDOW = 0, 1, 2, 3      # the modes of graycode_kernels.hip.h
WINDOW_CONDITIONS = ("dead", "outside", "columns", "rows", "end")


def front(hc, wc, box, maps=None):
    """plane_stack_frame of graycode_kernels.hip.h restated: for the region `box` = (x0, y0, w, h) of hc x wc planes, per thread of
    four consecutive region pixels that owns a pixel -> (mode int [threads], {condition: bool [threads]}).  The conditions, under
    maps only, are those of graycode_window, each True where it FAILS (several may): a `dead` pixel (past the region's end), a tap
    of a living pixel `outside` the image, a column spread over 6, a row spread over 1, the third row's 8 bytes ending outside
    the plane (`end`); the mode is GRAY_WINDOW where none fails and GRAY_TAPS otherwise.  A pixel without an interior cell counts
    as cell (0, 0) in the spreads, as in the kernel."""
    x0, y0, w, h = box
    npix = h * w
    p = 4 * np.arange((npix + 3) // 4, dtype=np.int64)[:, None] + np.arange(4)
    live = p < npix
    q = np.where(live, p, 0)
    at = (y0 + q // max(w, 1)) * wc + (x0 + q % max(w, 1))
    if maps is None:
        row4 = live[:, 3] & (at[:, 3] == at[:, 0] + 3)
        return np.where(row4, GRAY_ROW4, GRAY_BYTES), {}
    mx = np.where(live, np.asarray(maps[0], np.float32).ravel()[at], np.float32(np.nan))
    my = np.where(live, np.asarray(maps[1], np.float32).ravel()[at], np.float32(0))
    with np.errstate(invalid="ignore"):
        finite = (np.abs(mx) < 2.0 ** 26) & (np.abs(my) < 2.0 ** 26)
        cx = np.rint(np.where(finite, mx, 0).astype(np.float64) * 32.0).astype(np.int64) >> 5      # llrint: half to even
        cy = np.rint(np.where(finite, my, 0).astype(np.float64) * 32.0).astype(np.int64) >> 5
    interior = finite & (cx >= 0) & (cx + 1 < wc) & (cy >= 0) & (cy + 1 < hc)
    cx, cy = np.where(interior, cx, 0), np.where(interior, cy, 0)
    lo_x, lo_y = cx.min(axis=1), cy.min(axis=1)
    fails = {"dead": ~live.all(axis=1), "outside": (live & ~interior).any(axis=1), "columns": cx.max(axis=1) - lo_x > 6,
             "rows": cy.max(axis=1) - lo_y > 1, "end": (lo_y + 2) * wc + lo_x + 8 > hc * wc}
    window = ~np.logical_or.reduce([fails[c] for c in WINDOW_CONDITIONS])
    return np.where(window, GRAY_WINDOW, GRAY_TAPS), fails
