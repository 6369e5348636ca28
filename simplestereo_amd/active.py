"""
active
======
The data-parallel core of ``simplestereo.active`` (reference ``simplestereo/active.py``): the demodulation step of
Fourier-transform profilometry and the triangulation of its unwrapped phase into a point cloud, each executed by one HIP
kernel on an AMD MI355X through the C ABI of ``libssamd.so`` (``ssamd_ftp_phase``, ``ssamd_ftp_cloud``, ``include/ssamd.h``).

    import simplestereo_amd as ss
    phase = ss.active.ftpPhase(imgObj, imgRef, fc, radius_factor=0.5, unwrap="iir", tau=0.8)
    phase = ss.active.ftpPhase(imgObj, imgRef, fc, unwrap="numpy")      # the reference's default unwrapping
    k = ss.active.ftpFringeOrder(phase, stripe_indexes, rig, z_plane, period, stripeCentralPeak)
    cloud = ss.active.ftpCloud(phase, rig, z_plane, period, k)         # float64 [H, W, 3], on the device if phase is

``ftpPhase`` is the demodulation of ``StereoFTP.getCloud`` (``active.py:675-737``; the same lines are
``StereoFTP_PhaseOnly.getPhase``, ``:2012-2074``): gray by the channel maximum, a row-wise FFT of the object image and of
the (virtual) reference image, the per-row band-pass around the carrier ``fc``, an inverse FFT and
``angle(ghat * conj(g0hat))`` -- optionally followed by the unwrapper the reference passes as ``unwrappingMethod``
(``unwrap="iir"``) or by what it runs when none is passed, ``np.unwrap`` along x and then along y (``unwrap="numpy"``,
``active.py:739-745``).
It is NOT ``StereoFTP``: building the virtual reference image (``undistort``, ``projectPoints``, ``remap``), finding the
central stripe and estimating ``fc`` are cv2 calls in the reference and stay with the caller.

``ftpCloud`` is the triangulation that ends ``StereoFTP.getCloud`` (``active.py:776-841``, with the projector coordinates
of ``_getProjectorMapping``, ``:463-485``): ``cv2.projectPoints`` of every pixel centre onto the projector, phase to projector
column, the epipolar line, ``cv2.undistortPoints``, two rectifying homographies, disparity to depth and the common
rotation undone -- per pixel, in fp64, in one kernel, so that camera frame -> phase -> unwrapped phase -> cloud stays in HBM.
``ftpFringeOrder`` is the one step between the two that needs the central stripe (``active.py:779-788``); ``ftpGeometry``
packs what both read from the rig.  They are not ``StereoFTP`` either: the virtual reference image (``cv2.remap``),
``findCentralStripe`` and ``_calculateCameraFrequency`` (which give ``z_plane``, the stripe pixels and ``fc``) stay with the
caller.

The band is the reference's, decided exactly (numpy's mask on ``np.fft.fftfreq``); the phase is not bit-identical to
numpy's pocketfft -- the kernel sums a band-limited direct DFT in another order -- but agrees with the exact angle to a few
ulp of pi wherever ``|ghat * conj(g0hat)|`` is not tiny against its row.

=========================================================  ==============
condition                                                  exception
=========================================================  ==============
an image that is neither ndarray nor CUDA/HIP tensor,      ``TypeError``
or not uint8
one image on the host and one on a device, or on two       ``TypeError``
devices
an image not [H, W] or [H, W, 3]                           ``ValueError``
the two images differ in H or W                            ``ValueError``
``fc`` not a number or H numbers                           ``ValueError``
``radius_factor`` not a number                             ``ValueError``
``unwrap`` not ``None``, ``"iir"`` or ``"numpy"``          ``ValueError``
``unwrap="iir"`` and ``tau`` not a number in [0, 1]        ``ValueError``
W > ``MAX_WIDTH`` (8192)                                   ``ValueError``
=========================================================  ==============

``ftpCloud``, ``ftpFringeOrder`` and ``ftpGeometry``:

=========================================================  =======================
condition                                                  exception
=========================================================  =======================
the phase neither ndarray nor CUDA/HIP tensor, or not      ``TypeError``
float64
the phase not [H, W], or (W, H) not the ``roi``'s          ``ValueError``
``roi`` not four non-negative integers inside ``res1``     ``ValueError``
``z_plane``, ``period`` or ``k`` not a finite number,      ``ValueError``
or ``period == 0``
``distCoeffs2`` with a tilted sensor (tauX, tauY)          ``NotImplementedError``
``T[2] == 0``: the epipole on the projector is at          ``ValueError``
infinity (the reference yields NaN there)
``stripe_indexes`` not [n >= 1, 2] integers inside the     ``ValueError``
map; ``stripeCentralPeak`` not a finite number
=========================================================  =======================

All of them are raised before any native call.  An image or a phase map with no rows or no columns gives an empty array.
"""
import numbers

import numpy as np

from . import _native
from ._rigs import _dist_vector
from ._native import c_double as _c_double, is_device_tensor as _is_device_tensor

__all__ = ["ftpPhase", "ftpCloud", "ftpFringeOrder", "ftpGeometry", "FtpGeometry", "MAX_WIDTH"]

MAX_WIDTH = 8192          # SSAMD_FTP_MAX_W: twiddle table, gray rows and a chunk of bins of one row in 160 KiB of LDS


def _number(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.integer, np.floating)):
        raise ValueError("%s must be a number" % what)
    return float(v)


def _image(img, name):
    """-> (contiguous image, H, W, channels)"""
    dev = _is_device_tensor(img)
    if not (dev or isinstance(img, np.ndarray)):
        raise TypeError("%s must be a uint8 ndarray or a CUDA/HIP torch.uint8 tensor" % name)
    if dev:
        import torch
        if img.dtype != torch.uint8:
            raise TypeError("%s must be a uint8 tensor" % name)
    elif img.dtype != np.uint8:
        raise TypeError("%s must be a uint8 array" % name)
    if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError("%s must be [H, W] (gray) or [H, W, 3] (BGR)" % name)
    ch = 1 if img.ndim == 2 else 3
    return (img.contiguous() if dev else np.ascontiguousarray(img)), int(img.shape[0]), int(img.shape[1]), ch


def _band(fc, radius_factor, h):
    """The reference's pass band (active.py:684-686) in fp64 numpy: fmin[h], fmax[h]."""
    rf = _number(radius_factor, "radius_factor")
    if isinstance(fc, (str, bytes, bytearray)) or _is_device_tensor(fc):
        raise ValueError("fc must be a number or a host array of H numbers")
    try:
        f = np.asarray(fc)
        if f.dtype == np.bool_ or not (np.issubdtype(f.dtype, np.integer) or np.issubdtype(f.dtype, np.floating)):
            raise TypeError
        f = f.astype(np.float64)
    except (TypeError, ValueError):
        raise ValueError("fc must be a number or a host array of H numbers") from None
    if f.ndim == 0:
        f = np.full(h, float(f), dtype=np.float64)
    elif f.ndim != 1 or f.shape[0] != h:
        raise ValueError("fc must have one value per image row (%d), got shape %s" % (h, tuple(f.shape)))
    with np.errstate(all="ignore"):
        radius = rf * f
        fmin = f - radius
        fmax = f + radius
    return np.ascontiguousarray(fmin), np.ascontiguousarray(fmax)


_INVALID = (_native.EINVAL, _native.ELIMIT)


def ftpPhase(imgObj, imgRef, fc, radius_factor=0.5, unwrap=None, tau=1):
    """
    Phase of a fringe image against a reference fringe image by Fourier-transform profilometry.

    The demodulation of the reference's ``StereoFTP.getCloud`` (``active.py:675-737``): for every image row, the spectrum
    of the object image and of the reference image is cut to the band ``[fc - radius_factor*fc, fc + radius_factor*fc]``
    (bins of ``np.fft.fftfreq(W)``, bounds included), transformed back, and the phase is
    ``angle(ghat * conj(g0hat))``.  It is not ``StereoFTP``: the reference image, ``fc`` and the triangulation of the
    phase are the caller's.

    Parameters
    ----------
    imgObj, imgRef : ndarray or CUDA/HIP tensor, uint8
        ``[H, W]`` gray or ``[H, W, 3]`` BGR (reduced by the channel maximum, the reference's ``convertGrayscale``).
        The channel counts may differ; H and W must agree; both host arrays, or both tensors on one device.
    fc : float or array of H floats (host)
        Carrier frequency of each row in cycles per pixel (what ``_calculateCameraFrequency`` yields); a scalar is used for
        every row.
    radius_factor : float, optional
        Half width of the pass band as a fraction of ``fc``.  Default 0.5.
    unwrap : None, "iir" or "numpy", optional
        ``None``: the wrapped phase.  ``"iir"``: ``unwrapping.infiniteImpulseResponse`` of it with ``tau``, on the same
        stream without leaving the device; equal to calling the unwrapper on the wrapped result, bit for bit.
        ``"numpy"``: ``unwrapping.unwrap2D`` of it, the reference's default (``np.unwrap`` with ``discont=np.pi`` along x,
        then along y), likewise on the same stream and equal bit for bit to numpy's result on the wrapped map.
    tau : float, optional
        The IIR unwrapper's noise regularisation, 0 to 1 (only read with ``unwrap="iir"``).  Default 1.

    Returns
    -------
    ndarray or tensor
        float64 ``[H, W]``: a new array, or a tensor on the inputs' device computed on its current stream.  A row whose
        band holds no bin is 0.0.
    """
    obj, h, w, ch_obj = _image(imgObj, "imgObj")
    ref, h2, w2, ch_ref = _image(imgRef, "imgRef")
    dev = _is_device_tensor(obj)
    if dev != _is_device_tensor(ref):
        raise TypeError("imgObj and imgRef must both be host arrays or both be device tensors")
    if dev and obj.device != ref.device:
        raise TypeError("imgObj and imgRef must be on the same device")
    if (h, w) != (h2, w2):
        raise ValueError("imgObj and imgRef must have the same height and width (%dx%d, %dx%d)" % (h, w, h2, w2))
    fmin, fmax = _band(fc, radius_factor, h)
    if unwrap is not None and not (isinstance(unwrap, str) and unwrap in ("iir", "numpy")):
        raise ValueError('unwrap must be None, "iir" or "numpy"')
    t = 1.0
    if unwrap == "iir":
        t = _c_double(tau)
        if t < 0 or t > 1:
            raise ValueError("Wrong tau value!")
    if w > MAX_WIDTH:
        raise ValueError("rows wider than %d columns are not supported (width %d)" % (MAX_WIDTH, w))
    uw = {None: 0, "iir": 1, "numpy": 2}[unwrap]
    return _native.run("ssamd_ftp_phase", (obj, ref), (h, w),
                       lambda o, r, out: (o, ch_obj, r, ch_ref, h, w, fmin.ctypes.data, fmax.ctypes.data, uw, t, out), _INVALID)


# ------------------------------------------------------------------------------------------------ phase -> point cloud
NGEOM = 68                # SSAMD_FTP_CLOUD_NGEOM


def _finite(v, what):
    v = _number(v, what)
    if not np.isfinite(v):
        raise ValueError("%s must be finite" % what)
    return v


def _roi(roi, res1):
    """-> (x, y, w, h), inside the camera image"""
    W, H = int(res1[0]), int(res1[1])
    if roi is None:
        return 0, 0, W, H
    try:
        vals = tuple(roi)
    except TypeError:
        vals = ()
    if len(vals) != 4 or any(isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Integral, np.integer)) for v in vals):
        raise ValueError("roi must be four integers (x, y, width, height)")
    x, y, w, h = (int(v) for v in vals)
    if min(x, y, w, h) < 0 or x + w > W or y + h > H:
        raise ValueError("roi %s is not inside the camera image (%d x %d)" % ((x, y, w, h), W, H))
    return x, y, w, h


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


class FtpGeometry:
    """What ``ftpCloud`` and ``ftpFringeOrder`` read from a rig, a reference plane and a fringe period: ``geom``, the
    ``SSAMD_FTP_CLOUD_NGEOM`` doubles of ``ssamd_ftp_cloud`` (layout in ``include/ssamd.h``), and ``roi = (x, y, w, h)``."""
    __slots__ = ("geom", "roi", "fp")

    def __init__(self, geom, roi, fp):
        self.geom = geom
        self.roi = roi
        self.fp = fp              # 1 / period (active.py:385)


def ftpGeometry(rig, z_plane, period, roi=None):
    """
    Pack the geometry of ``ftpCloud`` / ``ftpFringeOrder``: build it once per ``z_plane`` and pass it in place of ``rig``.

    Built on the host in numpy as the reference builds it: ``M = z_plane * R.dot(inv(K1))`` (``active.py:479``, handed to
    ``cv2.projectPoints`` as a 3x3 ``rvec``), ``T``, ``K2``, ``distCoeffs2``, the epipole ``K2.dot(T) / K2.dot(T)[2]``
    (``:394-395``), ``2 * pi * fp`` with ``fp = 1 / period`` (``:385``, ``:799``), the rectifying transforms and the common
    orientation of ``_lowLevelRectify`` (``rectification.py:271-302``), its inverse (``:398``) and ``rig.getBaseline()``.

    Parameters
    ----------
    rig : StereoRig
        Camera in position 1 (world origin), projector in position 2.
    z_plane : float
        Distance of the reference plane from the camera.
    period : float
        Fringe period on the projector image, in pixels.
    roi : (x, y, width, height), optional
        Region of the camera image the phase map covers.  Default: the whole ``rig.res1``.

    Returns
    -------
    FtpGeometry
        ``.geom`` float64 [68], ``.roi`` (x, y, width, height).
    """
    z = _finite(z_plane, "z_plane")
    per = _finite(period, "period")
    if per == 0:
        raise ValueError("period must not be 0")
    box = _roi(roi, rig.res1)
    dist = _dist_vector(rig.distCoeffs2)                      # NotImplementedError for a tilted sensor
    K1 = np.asarray(rig.intrinsic1, dtype=np.float64)
    K2 = np.asarray(rig.intrinsic2, dtype=np.float64)
    R = np.asarray(rig.R, dtype=np.float64)
    T = np.asarray(rig.T, dtype=np.float64).reshape(3)
    if T[2] == 0:
        raise ValueError("T[2] == 0: the epipole on the projector image is at infinity")
    M = z * R.dot(np.linalg.inv(K1))
    ep = K2.dot(T)
    ep = ep / ep[2]
    fp = 1 / per
    rect1, rect2, common = _low_level_rectify(rig)
    g = np.concatenate([M.ravel(), T, [K2[0, 0], K2[1, 1], K2[0, 2], K2[1, 2]], dist[:12], K2.ravel(), ep[:2],
                        [2 * np.pi * fp], rect1.ravel(), rect2.ravel(), np.linalg.inv(common).ravel(),
                        [rig.getBaseline()]]).astype(np.float64)
    assert g.shape == (NGEOM,)
    if not np.isfinite(g).all():
        raise ValueError("the rig, z_plane and period give a geometry that is not finite")
    return FtpGeometry(np.ascontiguousarray(g), box, fp)


def _geometry(rig, z_plane, period, roi):
    if isinstance(rig, FtpGeometry):
        if z_plane is not None or period is not None or roi is not None:
            raise ValueError("with a packed geometry in place of the rig, z_plane, period and roi are the geometry's: pass None")
        return rig
    return ftpGeometry(rig, z_plane, period, roi)


def _phase_map(phase, box):
    """-> (contiguous map, is it on a device), checked against the roi"""
    dev = _is_device_tensor(phase)
    if not (dev or isinstance(phase, np.ndarray)):
        raise TypeError("phaseUnwrapped must be a float64 ndarray or a CUDA/HIP torch.float64 tensor")
    if dev:
        import torch
        if phase.dtype != torch.float64:
            raise TypeError("phaseUnwrapped must be a float64 tensor")
    elif phase.dtype != np.float64:
        raise TypeError("phaseUnwrapped must be a float64 array")
    if phase.ndim != 2:
        raise ValueError("phaseUnwrapped must be [H, W]")
    if (int(phase.shape[1]), int(phase.shape[0])) != (box[2], box[3]):
        raise ValueError("phaseUnwrapped is %d x %d but the roi is %d x %d (width x height)" %
                         (phase.shape[1], phase.shape[0], box[2], box[3]))
    return phase, dev


def _project_x(g, u, v):
    """x of ``cv2.projectPoints((u, v, 1), M, T, K2, distCoeffs2)`` (``active.py:478-481``) in numpy, the operations of
    ``ftp_cloud_kernel`` in its order."""
    M, T, (fx, _, cx, _), d = g[0:9], g[9:12], g[12:16], g[16:28]
    k1, k2, p1, p2, k3, k4, k5, k6, s1, s2, s3, s4 = d
    X = ((M[0] * u + M[1] * v) + M[2]) + T[0]
    Y = ((M[3] * u + M[4] * v) + M[5]) + T[1]
    Z = ((M[6] * u + M[7] * v) + M[8]) + T[2]
    iz = 1.0 / Z
    x, y = X * iz, Y * iz
    r2 = x * x + y * y
    r4 = r2 * r2
    r6 = r4 * r2
    kr = (((1.0 + k1 * r2) + k2 * r4) + k3 * r6) / (((1.0 + k4 * r2) + k5 * r4) + k6 * r6)
    xd = (((x * kr + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x)) + s1 * r2) + s2 * r4
    return fx * xd + cx


def ftpFringeOrder(phaseUnwrapped, stripe_indexes, rig, z_plane=None, period=None, stripeCentralPeak=None, roi=None):
    """
    The fringe order ``k`` of an unwrapped phase map from the pixels of the central stripe (``active.py:779-788``).

    With ``theta`` the phase at the stripe pixels and ``u_A`` the projector column of those pixels on the reference plane,
    ``k = ceil(mean((stripeCentralPeak - u_A) * fp - theta / (2 * pi)) - 0.5)``: the mean rounded to the nearest integer,
    a half rounded down.  It is not ``StereoFTP``: finding the stripe (``findCentralStripe``), ``z_plane`` and
    ``stripeCentralPeak`` stay with the caller.

    Parameters
    ----------
    phaseUnwrapped : ndarray or CUDA/HIP tensor, float64 ``[H, W]``
        A tensor is read at the stripe pixels with one indexed read and one small copy to the host.
    stripe_indexes : integer array ``[n, 2]``
        (x, y) of the stripe pixels inside the map (the reference's ``np.ceil(stripe_cam - 0.5)``).
    rig, z_plane, period, roi
        As in :func:`ftpCloud`.
    stripeCentralPeak : float
        Column of the central stripe's peak on the projector image.

    Returns
    -------
    float
        ``k``, integer valued.
    """
    G = _geometry(rig, z_plane, period, roi)
    peak = _finite(stripeCentralPeak, "stripeCentralPeak")
    phase, dev = _phase_map(phaseUnwrapped, G.roi)
    try:
        idx = np.asarray(stripe_indexes)
    except (TypeError, ValueError):
        idx = np.zeros(0)
    if idx.dtype == np.bool_ or not np.issubdtype(idx.dtype, np.integer) or idx.ndim != 2 or idx.shape[1] != 2 or idx.shape[0] < 1:
        raise ValueError("stripe_indexes must be an integer array [n >= 1, 2] of (x, y)")
    idx = idx.astype(np.int64)
    if idx.min() < 0 or idx[:, 0].max() >= G.roi[2] or idx[:, 1].max() >= G.roi[3]:
        raise ValueError("stripe_indexes outside the phase map")
    if dev:
        import torch
        where = torch.from_numpy(idx).to(phase.device)
        theta = phase[where[:, 1], where[:, 0]].cpu().numpy()
    else:
        theta = phase[idx[:, 1], idx[:, 0]]
    u_A = _project_x(G.geom, (idx[:, 0] + G.roi[0]) + 0.5, (idx[:, 1] + G.roi[1]) + 0.5)
    k = (peak - u_A) * G.fp - theta / (2 * np.pi)
    return float(np.ceil(np.mean(k) - 0.5))


def ftpCloud(phaseUnwrapped, rig, z_plane=None, period=None, k=0, roi=None):
    """
    Point cloud of an unwrapped Fourier-profilometry phase map.

    The triangulation of the reference's ``StereoFTP.getCloud`` (``active.py:776-841``): for every camera pixel centre
    ``(x + 0.5, y + 0.5)``, its projector coordinates on the reference plane (``cv2.projectPoints`` with
    ``z_plane * R.dot(inv(K1))`` as the 3x3 rotation, ``active.py:463-485``), the projector column moved by
    ``(phase + 2 k pi) / (2 pi fp)``, the row on the epipolar line, ``cv2.undistortPoints`` with ``P = K2`` (five
    iterations), the two rectifying homographies, ``baseline / |disparity|`` and the common rotation undone.  One HIP kernel,
    fp64 throughout (``ftp_cloud_kernel``).  It is not ``StereoFTP``: the phase, ``z_plane`` and ``k`` are the caller's
    (``ftpPhase``, ``ftpFringeOrder``).  Not bit-identical to cv2 (another operation order).

    Parameters
    ----------
    phaseUnwrapped : ndarray or CUDA/HIP tensor, float64 ``[H, W]``
        A tensor is made contiguous and the work goes on its device's current stream.
    rig : StereoRig
        Camera in position 1, projector in position 2 -- or an :func:`ftpGeometry` result, with ``z_plane``, ``period`` and
        ``roi`` left ``None``.
    z_plane : float
        Distance of the reference plane from the camera.
    period : float
        Fringe period on the projector image, in pixels.
    k : float, optional
        Fringe order (:func:`ftpFringeOrder`).  Default 0.
    roi : (x, y, width, height), optional
        Region of the camera image the map covers, as in the reference; (width, height) must be the map's.  Default: the
        whole ``rig.res1``.

    Returns
    -------
    ndarray or tensor
        float64 ``[H, W, 3]`` in the camera's coordinate system.  A pixel with a non-finite phase or a disparity of exactly
        0 holds the non-finite values the formulas give there.
    """
    G = _geometry(rig, z_plane, period, roi)
    order = _finite(k, "k")
    phase, dev = _phase_map(phaseUnwrapped, G.roi)
    x0, y0, w, h = G.roi
    if dev:
        phase = phase.contiguous()
        if phase.data_ptr() % 16:
            phase = phase.clone()     # a view at an odd storage offset: the kernel reads two phases per 16-byte load
    return _native.run("ssamd_ftp_cloud", (phase,), (h, w, 3), lambda src, out: (src, h, w, x0, y0, G.geom.ctypes.data, order, out), _INVALID)
