"""
unwrapping
==========
Phase unwrapping with the API of ``simplestereo.unwrapping`` (reference
``simplestereo/unwrapping.py``), executed by HIP kernels on an AMD MI355X
through the C ABI of ``libssamd.so`` (``include/ssamd.h``).

    import simplestereo_amd as ss
    unwrapped = ss.unwrapping.infiniteImpulseResponse(phase, tau=0.8)
    unwrapped = ss.unwrapping.unwrap2D(phase)          # the reference's default

=================================  ==========================  ==============================================
function                           native entry point          equal, bit for bit, to
=================================  ==========================  ==============================================
``infiniteImpulseResponse``        ``ssamd_iir_unwrap``        the reference's ``_unwrapping`` extension
``infiniteImpulseResponseBatch``   ``ssamd_iir_unwrap``        the same, per map of ``[n, h, w]``
``unwrap``                         ``ssamd_np_unwrap``         ``np.unwrap(p, discont, axis, period=period)``
``unwrap2D``                       ``ssamd_np_unwrap_xy``      ``np.unwrap(np.unwrap(p, discont=np.pi, axis=-1),
                                                               discont=np.pi, axis=-2)``: what every ``getCloud``
                                                               of the reference runs when no unwrapping method
                                                               is passed (``active.py:739-745``)
=================================  ==========================  ==============================================

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

``unwrap`` has ``np.unwrap``'s signature and arithmetic on float64 data
(``csrc/np_unwrap_kernels.hip.h``; the running sum is sequential, as numpy's,
because its rounding is observable).  Its checks, all before any native call:

=====================================  ===========================================
condition                              exception
=====================================  ===========================================
p neither ndarray nor CUDA/HIP tensor  ``TypeError``
p not float64                          ``TypeError`` (deviation: numpy computes
                                       float32 in float32; this path is fp64 only)
p 0-dimensional                        ``ValueError`` (as ``np.unwrap``, through ``diff``)
axis not an integer                    ``TypeError``
axis out of range                      ``numpy.exceptions.AxisError`` (numpy's own:
                                       a ``ValueError`` and an ``IndexError``)
period not a finite number > 0         ``ValueError`` (deviation: numpy returns NaN
                                       or sign-flipped intervals)
discont not ``None`` and not a number  ``ValueError``
=====================================  ===========================================

``discont=None`` means ``period / 2``; any other float, NaN included, is passed
through.  Empty arrays give empty arrays.  ``unwrap2D`` takes ``[h, w]`` or
``[n, h, w]`` (``ValueError`` otherwise).

Extensions (not in the reference): a CUDA/HIP ``torch.float64`` tensor
``[h, w]`` gives a tensor on the same device, computed on its current stream;
``infiniteImpulseResponseBatch`` unwraps ``[n, h, w]`` maps (host or device) in
one launch, one workgroup per map.
"""
import operator

import numpy as np

from . import _native
from ._native import c_double as _c_double, is_device_tensor as _is_device_tensor

__all__ = ["infiniteImpulseResponse", "infiniteImpulseResponseBatch", "unwrap", "unwrap2D"]


_INVALID = (_native.EINVAL, _native.ELIMIT)          # np.unwrap's forms: both are the caller's to fix


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


def _run(phase, tau, ndim):
    t = _check(phase, tau, ndim)
    shape = tuple(int(s) for s in phase.shape)
    n, h, w = (1,) + shape if ndim == 2 else shape
    if _is_device_tensor(phase):
        import torch
        if phase.dtype != torch.float64:
            raise TypeError("phase must be a float64 tensor")
    elif phase.dtype != np.float64:
        raise TypeError("phase must be a float64 array (the reference reads any buffer as doubles)")
    return _native.run("ssamd_iir_unwrap", (phase,), shape, lambda src, out: (src, n, h, w, t, out), (_native.EINVAL,))


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


def _fp64_input(p, name):
    """TypeError unless p is a float64 ndarray or device tensor"""
    dev = _is_device_tensor(p)
    if not (dev or isinstance(p, np.ndarray)):
        raise TypeError("%s must be a float64 ndarray or a CUDA/HIP torch.float64 tensor" % name)
    if dev:
        import torch
        if p.dtype != torch.float64:
            raise TypeError("%s must be a float64 tensor (this path is fp64 only)" % name)
    elif p.dtype != np.float64:
        raise TypeError("%s must be a float64 array (this path is fp64 only)" % name)


def unwrap(p, discont=None, axis=-1, *, period=2 * np.pi):
    """
    Unwrap by taking the complement of large deltas with respect to the period: ``np.unwrap`` on the device.

    Equal to ``np.unwrap(p, discont, axis, period=period)`` bit for bit (NaN where numpy has NaN) for float64 data.

    Parameters
    ----------
    p : ndarray or CUDA/HIP tensor, float64
        Any number of dimensions >= 1; made contiguous first if it is not.
    discont : float, optional
        Maximum discontinuity between values; ``None`` (the default) is ``period / 2``.  NaN is passed through.
    axis : int, optional
        Axis along which to unwrap, negative values count from the last.  Default -1.
        Out of range raises ``numpy.exceptions.AxisError``.
    period : float, optional
        Size of the range over which the input wraps, a finite number > 0.  Default ``2 pi``.

    Returns
    -------
    ndarray or tensor
        float64, the shape of ``p``: a new array, or a tensor on the input's device computed on its current stream.
    """
    if isinstance(p, np.generic):                      # a numpy scalar is a 0-d array to numpy
        p = np.asarray(p)
    _fp64_input(p, "p")
    if p.ndim == 0:
        raise ValueError("diff requires input that is at least one dimensional")
    ax = operator.index(axis)
    if not -p.ndim <= ax < p.ndim:
        raise np.exceptions.AxisError(ax, p.ndim)
    ax %= p.ndim
    try:
        per = _c_double(period)
        dis = None if discont is None else _c_double(discont)
    except ValueError:
        raise ValueError("period and discont must be numbers") from None
    if not (np.isfinite(per) and per > 0):
        raise ValueError("period must be a finite positive number")
    if dis is None:
        dis = per / 2
    shape = tuple(int(s) for s in p.shape)
    outer = int(np.prod(shape[:ax], dtype=object)) if ax else 1
    inner = int(np.prod(shape[ax + 1:], dtype=object)) if ax + 1 < len(shape) else 1
    n = shape[ax]
    return _native.run("ssamd_np_unwrap", (p,), shape, lambda src, out: (src, outer, n, inner, dis, per, out), _INVALID)


def unwrap2D(phase):
    """
    The reference's default unwrapping of a phase map (``active.py:739-745``): ``np.unwrap`` with ``discont=np.pi`` along
    x (the last axis), then along y, in two launches on one stream.

    ``phase`` is ``[h, w]`` or ``[n, h, w]`` float64, a host array or a CUDA/HIP tensor; every map of a batch is unwrapped on
    its own.  Returns the same shape, equal bit for bit to
    ``np.unwrap(np.unwrap(phase, discont=np.pi, axis=-1), discont=np.pi, axis=-2)``.
    """
    _fp64_input(phase, "phase")
    if phase.ndim not in (2, 3):
        raise ValueError("phase must be [h, w] or [n, h, w]")
    shape = tuple(int(s) for s in phase.shape)
    if max(shape) > 2 ** 31 - 1:
        raise ValueError("phase extents beyond 2^31 - 1 are not supported")
    n, h, w = (1,) + shape if phase.ndim == 2 else shape
    return _native.run("ssamd_np_unwrap_xy", (phase,), shape, lambda src, out: (src, n, h, w, out), _INVALID)
