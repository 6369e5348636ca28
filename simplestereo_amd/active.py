"""
active
======
The data-parallel core of ``simplestereo.active`` (reference ``simplestereo/active.py``): the demodulation step of
Fourier-transform profilometry, executed by one HIP kernel on an AMD MI355X through the C ABI of ``libssamd.so``
(``ssamd_ftp_phase``, ``include/ssamd.h``).

    import simplestereo_amd as ss
    phase = ss.active.ftpPhase(imgObj, imgRef, fc, radius_factor=0.5, unwrap="iir", tau=0.8)
    phase = ss.active.ftpPhase(imgObj, imgRef, fc, unwrap="numpy")      # the reference's default unwrapping

``ftpPhase`` is the demodulation of ``StereoFTP.getCloud`` (``active.py:675-737``; the same lines are
``StereoFTP_PhaseOnly.getPhase``, ``:2012-2074``): gray by the channel maximum, a row-wise FFT of the object image and of
the (virtual) reference image, the per-row band-pass around the carrier ``fc``, an inverse FFT and
``angle(ghat * conj(g0hat))`` -- optionally followed by the unwrapper the reference passes as ``unwrappingMethod``
(``unwrap="iir"``) or by what it runs when none is passed, ``np.unwrap`` along x and then along y (``unwrap="numpy"``,
``active.py:739-745``).
It is NOT ``StereoFTP``: building the virtual reference image (``undistort``, ``projectPoints``, ``remap``), finding the
central stripe, estimating ``fc`` and triangulating the phase into a cloud are cv2 calls in the reference and stay with
the caller.

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

All of them are raised before any native call.  An image with no rows or no columns gives an empty array.
"""
import ctypes
import numbers

import numpy as np

from . import _native
from .passive import _is_device_tensor
from .unwrapping import _c_double

__all__ = ["ftpPhase", "MAX_WIDTH"]

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


def _raise_native(e):
    if e.code in (-1, -5):          # SSAMD_EINVAL, SSAMD_ELIMIT
        raise ValueError(e.message) from None
    raise e


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
    if dev:
        import torch
        out = torch.empty((h, w), dtype=torch.float64, device=obj.device)
        if h == 0 or w == 0:
            return out
        with torch.cuda.device(obj.device):
            stream = torch.cuda.current_stream(obj.device).cuda_stream
            try:
                _native.check(_native.lib().ssamd_ftp_phase_device(obj.data_ptr(), ch_obj, ref.data_ptr(), ch_ref, h, w,
                                                                   fmin.ctypes.data, fmax.ctypes.data, uw, t, out.data_ptr(),
                                                                   ctypes.c_void_p(stream)))
            except _native.NativeError as e:
                _raise_native(e)
        return out
    out = np.empty((h, w), dtype=np.float64)
    if h == 0 or w == 0:
        return out
    try:
        _native.check(_native.lib().ssamd_ftp_phase(obj.ctypes.data, ch_obj, ref.ctypes.data, ch_ref, h, w, fmin.ctypes.data,
                                                    fmax.ctypes.data, uw, t, out.ctypes.data, -1))
    except _native.NativeError as e:
        _raise_native(e)
    return out
