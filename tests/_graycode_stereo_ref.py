"""Two-camera Gray code (what the reference's GrayCodeDouble.getCloud, active.py:1508-1608, sets out to do) restated in plain
numpy on tests/_graycode_ref.py: the decode per camera, the projector-shaped tables by np.maximum.at / np.add.at, the match, and
the triangulation of active.py:1594-1606 in the operation order of graycode_stereo_kernels.hip.h, each operation rounded once.
`table_last_literal` is the reference's double Python loop with the indices the right way round.

Nothing here imports simplestereo_amd."""
import numpy as np

import _graycode_ref as G

NGEOM = G.NGEOM
BLOCK = 1024                # SSAMD_GRAYCODE_BLOCK: cells per workgroup, four per thread, 64 threads per wave


# ------------------------------------------------------------------------------------------------ decode
def decode_camera(stack, K, dist, res, proj, white_thr, box=None):
    """cv2.undistort(img, K, dist) of every plane, getProjPixel for every pixel, cut to `box` = (x0, y0, w, h): int32 [h, w, 2]"""
    pw, ph = proj
    n = G.num_patterns(pw, ph)
    stack = np.asarray(stack)[:n]
    und = G.undistort_stack(stack, K, dist, res)
    dec = G.decode(und, pw, ph, white_thr, shape=(int(res[1]), int(res[0])))
    if box is None:
        return dec
    x0, y0, w, h = box
    return np.ascontiguousarray(dec[y0:y0 + h, x0:x0 + w])


# ------------------------------------------------------------------------------------------------ the tables
def _cells(decoded, origin, proj):
    """-> (cell, x, y) of the pixels that decode to a projector pixel, absolute coordinates, int64, in raster order"""
    pw, ph = proj
    h, w = decoded.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    dx, dy = decoded[..., 0].astype(np.int64), decoded[..., 1].astype(np.int64)
    ok = (dx >= 0) & (dx < pw) & (dy >= 0) & (dy < ph)
    return (dy * pw + dx)[ok], (xx + origin[0])[ok].astype(np.int64), (yy + origin[1])[ok].astype(np.int64)


def table_last(decoded, origin, proj):
    """int64 [Hp, Wp, 2]: the (x, y) of the pixel that comes last in raster order among those decoding to the cell, or (-1, -1):
    np.maximum.at on the key y * stride + x, stride = x0 + w"""
    pw, ph = proj
    stride = max(origin[0] + decoded.shape[1], 1)
    cell, x, y = _cells(decoded, origin, proj)
    key = np.full(pw * ph, -1, np.int64)
    np.maximum.at(key, cell, y * stride + x)
    out = np.stack([np.where(key >= 0, key % stride, -1), np.where(key >= 0, key // stride, -1)], axis=-1)
    return out.reshape(ph, pw, 2)


def table_last_literal(decoded, origin, proj):
    """The reference's loop (active.py:1559-1564) with the projector pixel as the index and the camera pixel as the value"""
    pw, ph = proj
    corresp = np.full((ph, pw, 2), -1, dtype=np.int64)
    h, w = decoded.shape[:2]
    for y in range(h):
        for x in range(w):
            px, py = int(decoded[y, x, 0]), int(decoded[y, x, 1])
            if 0 <= px < pw and 0 <= py < ph:
                corresp[py, px, 0] = x + origin[0]
                corresp[py, px, 1] = y + origin[1]
    return corresp


def table_mean(decoded, origin, proj):
    """(sum of x, sum of y, count) int64 [Hp, Wp] each: np.add.at"""
    pw, ph = proj
    cell, x, y = _cells(decoded, origin, proj)
    sx, sy, n = (np.zeros(pw * ph, np.int64) for _ in range(3))
    np.add.at(sx, cell, x)
    np.add.at(sy, cell, y)
    np.add.at(n, cell, 1)
    return sx.reshape(ph, pw), sy.reshape(ph, pw), n.reshape(ph, pw)


def side(decoded, origin, proj, reduce):
    """-> (seen bool [Hp, Wp], x float64, y float64): the pixel that stands for each cell"""
    if reduce == "last":
        t = table_last(decoded, origin, proj)
        return t[..., 0] >= 0, t[..., 0].astype(np.float64), t[..., 1].astype(np.float64)
    sx, sy, n = table_mean(decoded, origin, proj)
    with np.errstate(all="ignore"):
        return n > 0, sx.astype(np.float64) / n.astype(np.float64), sy.astype(np.float64) / n.astype(np.float64)


def match(decoded1, decoded2, proj, reduce="last", origin1=(0, 0), origin2=(0, 0)):
    """float64 [Hp, Wp, 4]: (x1 + 0.5, y1 + 0.5, x2 + 0.5, y2 + 0.5) where both cameras see the projector pixel, NaN elsewhere"""
    s1, x1, y1 = side(decoded1, origin1, proj, reduce)
    s2, x2, y2 = side(decoded2, origin2, proj, reduce)
    out = np.stack([x1 + 0.5, y1 + 0.5, x2 + 0.5, y2 + 0.5], axis=-1)
    out[~(s1 & s2)] = np.nan
    return out


# ------------------------------------------------------------------------------------------------ the triangulation
def geometry(rig):
    """The doubles [40:68] of the geometry (Rectify1, Rectify2, inv(commonR), the baseline) for the rig dict, 0 elsewhere"""
    g = G.geometry(rig)
    out = np.zeros(NGEOM)
    out[40:] = g[40:]
    return out


def triangulate(g, p1, p2, dtype=np.float64):
    """`dtype` (n, 1, 3): active.py:1594-1606 on the couples p1, p2 [..., 2] -- Rectify1 on p1, Rectify2 on p2 (x only),
    disparity = |p1x - p2x|, baseline * (p1 / disparity), the common rotation undone; three NaN where a couple holds a NaN"""
    g = np.asarray(g, dtype=np.float64).astype(dtype)
    p1, p2 = (np.asarray(a).reshape(-1, 2).astype(dtype) for a in (p1, p2))
    u, v, hx, hy = p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]
    with np.errstate(all="ignore"):
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
    out[np.isnan(p1).any(axis=1) | np.isnan(p2).any(axis=1)] = np.nan
    return out.reshape(-1, 1, 3)


def cloud(g, matches, dense=False):
    """The points of a match: [Hp, Wp, 3] with NaN, or (n, 1, 3) of the matched cells in projector raster order"""
    ph, pw = matches.shape[:2]
    pts = triangulate(g, matches[..., 0:2], matches[..., 2:4])
    if dense:
        return pts.reshape(ph, pw, 3)
    return pts[~np.isnan(matches.reshape(-1, 4)).any(axis=1)]


def get_cloud(rig, stacks, proj, white_thr=5, reduce="last", rois=(None, None), dense=False):
    """The whole chain for the rig dict `rig` (two cameras) and its two stacks; `rois` as (x, y, x_end, y_end) or None"""
    decoded, origins = [], []
    for i, (K, d, res) in enumerate(((rig["intrinsic1"], rig["distCoeffs1"], rig["res1"]), (rig["intrinsic2"], rig["distCoeffs2"], rig["res2"]))):
        x0, y0, xe, ye = rois[i] if rois[i] is not None else (0, 0, res[0], res[1])
        box = (x0, y0, max(xe - x0, 0), max(ye - y0, 0))
        decoded.append(decode_camera(stacks[i], K, d if d is not None else [0.0] * 5, res, proj, white_thr, box))
        origins.append((x0, y0))
    m = match(decoded[0], decoded[1], proj, reduce, origins[0], origins[1])
    return cloud(geometry(rig), m, dense), m, decoded


# ------------------------------------------------------------------------------------------------ inputs
def two_camera_rig(res1, res2, dist1=None, dist2=None):
    """A rig dict of two cameras side by side (camera 2 where _graycode_ref.rig puts its projector)"""
    r = G.rig(res1, res2, dist2=None, dist1=dist1)
    r["distCoeffs2"] = list(dist2) if dist2 is not None else [0.0] * 5
    return r


def render_runs(res, proj, runs, start=0):
    """The stack of a camera of `res` whose pixels, in raster order from pixel `start` on, look at consecutive projector pixels in
    runs of the lengths `runs` (cycled): run k covers projector pixel k % (pw * ph).  The pixels before `start` see nothing
    (zero contrast).  -> (stack uint8 [N, H, W], cell int64 [H, W] with -1 before start)"""
    w, h = res
    pw, ph = proj
    n = w * h
    lengths = np.resize(np.asarray(runs, dtype=np.int64), n)
    owner = np.repeat(np.arange(n), lengths)[:n - start] % (pw * ph)
    cell = np.full(n, -1, np.int64)
    cell[start:] = owner
    px, py = np.where(cell >= 0, cell % pw, 0).reshape(h, w), np.where(cell >= 0, cell // pw, 0).reshape(h, w)
    nb = G.num_bits(pw) + G.num_bits(ph)
    contrast = np.broadcast_to(np.where(cell >= 0, 60, 0).reshape(1, h, w), (nb, h, w))
    return G.render(px, py, pw, ph, contrast), cell.reshape(h, w)
