"""The reference's FTP without a reference plane restated in plain numpy: StereoFTP_Mapping.getCloud (active.py:1288-1450) and
StereoFTP_PhaseOnly.getPhase (:1950-2074) -- the demodulation of one image the np.fft way and as an extended-precision truth,
the bilinear sample of the phase along the stripe (scipy's map_coordinates, order 1, mode 'constant'), the per-pixel
_triangulate written out elementwise, and both pipelines returning every stage.

Nothing here imports simplestereo_amd."""
import json
import os

import numpy as np

import _ftp_cloud_ref as C
import _ftp_ref as P
import _stereo_ftp_ref as S

LD = np.longdouble


# ------------------------------------------------------------------------------------------------ one-image demodulation
def carrier_phase_numpy(img, fc, radius_factor):
    """np.angle(np.fft.ifft(bandpass(np.fft.fft(gray)))), active.py:1354-1401"""
    g = P.gray(img)
    h, w = g.shape
    fmin, fmax = P.band(fc, radius_factor, h)
    G = np.fft.fft(g, axis=1)
    G[~P.keep_mask(w, fmin, fmax)] = 0
    return np.angle(np.fft.ifft(G, axis=1))


def carrier_truth_longdouble(img, fc, radius_factor):
    """(phase fp64 [h, w], ratio fp64 [h, w]): the band-limited sums evaluated directly in np.longdouble and rounded once;
    ratio = |ghat| over its row's maximum (1 on rows with an empty band, whose phase is 0)."""
    g = P.gray(img).astype(LD)
    h, w = g.shape
    fmin, fmax = P.band(fc, radius_factor, h)
    lo, hi = P.band_ranges(w, fmin, fmax)
    two_pi = LD(8) * np.arctan(LD(1))
    x = np.arange(w, dtype=np.int64)
    phase = np.zeros((h, w), dtype=np.float64)
    ratio = np.ones((h, w), dtype=np.float64)
    for y in range(h):
        if hi[y] < lo[y]:
            continue
        s = np.arange(lo[y], hi[y] + 1, dtype=np.int64)
        ang = two_pi * (np.outer(s, x) % w).astype(LD) / LD(w)           # [K, w], the angle reduced exactly
        c, sn = np.cos(ang), np.sin(ang)
        gr, gi = c @ g[y], -(sn @ g[y])                                  # G[s]
        ar, ai = gr @ c - gi @ sn, gr @ sn + gi @ c                      # ghat[x] (times w)
        phase[y] = np.arctan2(ai, ar).astype(np.float64)
        mod = np.hypot(ar, ai)
        ratio[y] = (mod / mod.max()).astype(np.float64)
    return phase, ratio


def unwrap2d(wrapped):
    """active.py:1406-1408"""
    return np.unwrap(np.unwrap(wrapped, axis=1), axis=0)


# ------------------------------------------------------------------------------------------------ the phase at the stripe
def stripe_phase(phase, stripe):
    """np.mean(map_coordinates(phase, (y, x), order=1)) for stripe [n, 2] of (x, y), active.py:1431-1432: scipy's linear
    spline with mode='constant', cval 0 -- a point strictly outside [0, n - 1] on either axis is 0.0"""
    h, w = phase.shape
    x, y = np.asarray(stripe, dtype=np.float64)[:, 0], np.asarray(stripe, dtype=np.float64)[:, 1]
    inside = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
    xc, yc = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
    fx, fy = np.floor(xc), np.floor(yc)
    tx, ty = xc - fx, yc - fy
    ix0, iy0 = fx.astype(np.int64), fy.astype(np.int64)
    ix1, iy1 = np.minimum(ix0 + 1, w - 1), np.minimum(iy0 + 1, h - 1)
    val = ((((1 - ty) * (1 - tx)) * phase[iy0, ix0] + ((1 - ty) * tx) * phase[iy0, ix1]) + (ty * (1 - tx)) * phase[iy1, ix0]) \
        + (ty * tx) * phase[iy1, ix1]
    return float(np.mean(np.where(inside, val, 0.0)))


# ------------------------------------------------------------------------------------------------ per-pixel _triangulate
def mapping_geometry(rig, period):
    """(g [68], F [9]): the entries of the FTP cloud geometry the triangulation reads plus 2 pi fp, the others 0 -- no reference
    plane, no epipole -- and the fundamental matrix row by row (active.py:385-401)"""
    rg = S.Rig(rig, period, 1280)
    d = np.zeros(12)
    d[:len(rg.d2)] = rg.d2
    g = np.zeros(C.NGEOM)
    g[12:16] = rg.K2[0, 0], rg.K2[1, 1], rg.K2[0, 2], rg.K2[1, 2]
    g[16:28] = d
    g[28:37] = rg.K2.ravel()
    g[39] = 2 * np.pi * rg.fp
    g[40:49], g[49:58], g[58:67], g[67] = rg.Rectify1.ravel(), rg.Rectify2.ravel(), rg.R_inv.ravel(), rg.baseline
    return g, np.ascontiguousarray(rg.F.reshape(9))


def mapping_cloud(g, F, phase, theta, peak, x0, y0):
    """[h, w, 3]: active.py:1436-1447 and _triangulate (:561-605) per pixel, elementwise, each operation rounded once"""
    g, F = np.asarray(g, dtype=np.float64), np.asarray(F, dtype=np.float64).reshape(9)
    phase = np.asarray(phase, dtype=np.float64)
    h, w = phase.shape
    yy, xx = np.mgrid[0:h, 0:w]
    with np.errstate(all="ignore"):
        cx = (xx.astype(np.float64) + 0.5) + float(x0)
        cy = (yy.astype(np.float64) + 0.5) + float(y0)
        px = (((phase - theta) / g[39]) + peak) + 0.5                        # :1436-1441
        l0 = (F[0] * cx + F[1] * cy) + F[2]                                  # :573
        l1 = (F[3] * cx + F[4] * cy) + F[5]
        l2 = (F[6] * cx + F[7] * cy) + F[8]
        py = -((l0 * px + l2) / l1)                                          # :584
        hx, hy = C.undistort_points(g, px, py)                               # :590-594, then the tail of cloud_from_geometry
        R1, R2, Ri, baseline = g[40:49], g[49:58], g[58:67], g[67]
        ppx = ((R2[0] * hx + R2[1] * hy) + R2[2]) / ((R2[6] * hx + R2[7] * hy) + R2[8])
        Wc = (R1[6] * cx + R1[7] * cy) + R1[8]
        pcx = ((R1[0] * cx + R1[1] * cy) + R1[2]) / Wc
        pcy = ((R1[3] * cx + R1[4] * cy) + R1[5]) / Wc
        disparity = np.abs(ppx - pcx)
        qx, qy, qz = baseline * (pcx / disparity), baseline * (pcy / disparity), baseline * (1 / disparity)
        return np.stack([(Ri[0] * qx + Ri[1] * qy) + Ri[2] * qz, (Ri[3] * qx + Ri[4] * qy) + Ri[5] * qz,
                         (Ri[6] * qx + Ri[7] * qy) + Ri[8] * qz], axis=-1)


# ------------------------------------------------------------------------------------------------ the pipelines
def _front(rig, fringe, period, frame, roi):
    rg = S.Rig(rig, period, fringe.shape[1])
    W, H = rg.res1
    mx, my = S.undistort_maps(rg.K1, rg.d1, rg.res1)
    und = S.remap_linear(frame, mx, my)
    box = (0, 0, W, H) if roi is None else tuple(roi)
    x0, y0, w, h = box
    cut = np.ascontiguousarray(und[y0:y0 + h, x0:x0 + w])
    return rg, cut, box, S.find_central_stripe(cut, "r", 0.5)


def pipeline_mapping(rig, fringe, period, frame, roi=None, radius_factor=0.5, phase_of=None, unwrap=unwrap2d):
    """StereoFTP_Mapping(rig, fringe, period).getCloud(frame, radius_factor, roi) in numpy -> dict of every stage; the stripe
    is sampled where it is (the reference shifts it by the roi origin first, in place).  `phase_of(cut, fc, radius_factor)`
    replaces the np.fft demodulation."""
    rg, cut, box, stripe = _front(rig, fringe, period, frame, roi)
    world = S.triangulate(rg, stripe, rg.peak, box)
    fc = S.camera_frequency(rg, world)
    fmin, fmax = P.band(fc, radius_factor, box[3])
    wrapped = (phase_of or carrier_phase_numpy)(cut, fc, radius_factor)
    phase = unwrap(wrapped)
    theta = stripe_phase(phase, stripe)
    g, F = mapping_geometry(rig, period)
    cloud = mapping_cloud(g, F, phase, theta, rg.peak, box[0], box[1])
    return {"undistorted": cut, "stripe": stripe, "world": world, "fc": fc, "fmin": fmin, "fmax": fmax, "wrapped": wrapped,
            "phase": phase, "theta_shift": theta, "geom": g, "F": F, "peak": rg.peak, "cloud": cloud}


def pipeline_phase_only(rig, fringe, period, frame, roi=None, radius_factor=0.5):
    """StereoFTP_PhaseOnly(rig, fringe, period).getPhase(frame, radius_factor, roi) in numpy -> dict of every stage"""
    rg, cut, box, stripe = _front(rig, fringe, period, frame, roi)
    stripe_cam = S.undistort_points(stripe, rg.K1, rg.d1, rg.K1)             # :1992-1997
    world = S.triangulate(rg, stripe_cam, rg.peak, box)
    fc = S.camera_frequency(rg, world)
    z_plane = np.min(world[:, 2])                                            # :2007
    g, _ = C.geometry(rig, z_plane, period)
    ref = S.reference_image(np.max(fringe, axis=2), g, *box)
    return {"undistorted": cut, "stripe": stripe, "stripe_cam": stripe_cam, "world": world, "fc": fc, "z_plane": z_plane, "geom": g,
            "ref": ref, "phase": P.ftp_phase_numpy(cut, ref, fc, radius_factor), "phase_obj": carrier_phase_numpy(cut, fc, radius_factor),
            "phase_ref": carrier_phase_numpy(ref, fc, radius_factor)}


# ------------------------------------------------------------------------------------------------ golden cases
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_LOADED = []


def load():
    """(meta, arrays) of tests/golden/ftp_mapping_cases.{json,npz} (make_golden_ftp_mapping.py); loaded once, read-only"""
    if not _LOADED:
        with open(os.path.join(GOLDEN, "ftp_mapping_cases.json")) as f:
            meta = json.load(f)
        z = np.load(os.path.join(GOLDEN, "ftp_mapping_cases.npz"))
        arrays = {k: z[k] for k in z.files}
        for a in arrays.values():
            a.setflags(write=False)
        _LOADED.extend([meta, arrays])
    return _LOADED[0], _LOADED[1]
