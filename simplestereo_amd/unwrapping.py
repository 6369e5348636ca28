"""
unwrapping
==========
Phase unwrapping with the API of ``simplestereo.unwrapping`` (reference
``simplestereo/unwrapping.py``), executed by a HIP wavefront kernel on an AMD
MI355X through the C ABI of ``libssamd.so`` (``ssamd_iir_unwrap``,
``include/ssamd.h``).

    import simplestereo_amd as ss
    unwrapped = ss.unwrapping.infiniteImpulseResponse(phase, tau=0.8)

``infiniteImpulseResponse`` returns the reference's map bit for bit (fp64,
same operands in the same order, no contraction, a true division), with the
reference's checks in its order:

=====================================  ===========================================
condition                              exception (reference ``_unwrapping.cpp`` line)
=====================================  ===========================================
phase not an ndarray / tau not a number ``ValueError("Invalid input format!")`` (63)
phase not 2-D                          ``ValueError("Wrong phase dimensions!")`` (68)
tau < 0 or tau > 1                     ``ValueError("Wrong tau value!")`` (72)
=====================================  ===========================================

(int and bool tau are accepted; a NaN tau passes the check and gives a NaN map,
as in the reference.)

Documented deviations that turn undefined behaviour of the reference into
defined behaviour: a non-float64 ndarray raises ``TypeError`` (the reference
reads any buffer as doubles: out of bounds for float32); an array with no rows
returns an empty array (the reference reads row 0 of it); non-contiguous input
is made contiguous first; calls never corrupt the heap and may be repeated
(the reference's flag allocation, ``_unwrapping.cpp:80-93``, writes past its
first row, and ``:78`` steals a dtype reference).

Extensions (not in the reference): a CUDA/HIP ``torch.float64`` tensor
``[h, w]`` gives a tensor on the same device, computed on its current stream;
``infiniteImpulseResponseBatch`` unwraps ``[n, h, w]`` maps (host or device) in
one launch, one workgroup per map.
"""
import ctypes

import numpy as np

from . import _native
from .passive import _is_device_tensor

__all__ = ["infiniteImpulseResponse", "infiniteImpulseResponseBatch"]


def _c_double(v):
    """PyArg_ParseTuple 'd': a float, an int (bool included) or anything with __float__ / __index__; not a string."""
    if isinstance(v, (str, bytes, bytearray)):
        raise ValueError("Invalid input format!")
    try:
        return float(v)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("Invalid input format!") from None


def _check(phase, tau, ndim):
    """The reference's checks (_unwrapping.cpp:62-74) in its order; returns tau as a float."""
    if not (isinstance(phase, np.ndarray) or _is_device_tensor(phase)):
        raise ValueError("Invalid input format!")                 # "O!" with PyArray_Type
    t = _c_double(tau)
    if phase.ndim != ndim:
        raise ValueError("Wrong phase dimensions!")
    if t < 0 or t > 1:
        raise ValueError("Wrong tau value!")
    return t


def _raise_native(e):
    if e.code == -1:          # SSAMD_EINVAL
        raise ValueError(e.message) from None
    raise e


def _run(phase, tau, ndim):
    t = _check(phase, tau, ndim)
    shape = tuple(int(s) for s in phase.shape)
    n, h, w = (1,) + shape if ndim == 2 else shape
    if _is_device_tensor(phase):
        import torch
        if phase.dtype != torch.float64:
            raise TypeError("phase must be a float64 tensor")
        src = phase.contiguous()
        out = torch.empty(shape, dtype=torch.float64, device=src.device)
        if n == 0 or h == 0 or w == 0:
            return out
        with torch.cuda.device(src.device):
            stream = torch.cuda.current_stream(src.device).cuda_stream
            try:
                _native.check(_native.lib().ssamd_iir_unwrap_device(src.data_ptr(), n, h, w, t, out.data_ptr(),
                                                                    ctypes.c_void_p(stream)))
            except _native.NativeError as e:
                _raise_native(e)
        return out
    if phase.dtype != np.float64:
        raise TypeError("phase must be a float64 array (the reference reads any buffer as doubles)")
    src = np.ascontiguousarray(phase)
    out = np.empty(shape, dtype=np.float64)
    if n == 0 or h == 0 or w == 0:
        return out
    try:
        _native.check(_native.lib().ssamd_iir_unwrap(src.ctypes.data, n, h, w, t, out.ctypes.data, -1))
    except _native.NativeError as e:
        _raise_native(e)
    return out


def infiniteImpulseResponse(phase, tau=1):
    """
    Unwrap a 2D phase map.

    Method from "Noise robust linear dynamic system for
    phase unwrapping and smoothing", Estrada et al, 2011,
    DOI: 10.1364/OE.19.005126

    Parameters
    ----------
    phase : ndarray
        A 2D float64 array containing the wrapped phase values (or a CUDA/HIP
        ``torch.float64`` tensor ``[h, w]``).
    tau : float, optional
        Noise regularization parameter. Accept values from 0 to 1.
        Lower values used for higher error.
        Default to 1.

    Returns
    -------
    ndarray
        Unwrapped phase, a new float64 array of the same shape (a tensor on the
        input's device for a tensor input).
    """
    return _run(phase, tau, 2)


def infiniteImpulseResponseBatch(phases, tau=1):
    """``infiniteImpulseResponse`` of every map of ``phases`` ([n, h, w] float64, host array or device tensor) in one
    launch; returns [n, h, w], map k equal to ``infiniteImpulseResponse(phases[k], tau)``."""
    return _run(phases, tau, 3)
