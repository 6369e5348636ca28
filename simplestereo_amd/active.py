"""
active
======
Fourier-transform profilometry of ``simplestereo.active`` (reference ``simplestereo/active.py``): ``StereoFTP``, camera
frame in, point cloud out, and the steps it is made of -- the central stripe, the virtual reference image, the demodulation
and the triangulation of the unwrapped phase -- each per-pixel step executed by one HIP kernel on an AMD MI355X through the C
ABI of ``libssamd.so`` (``ssamd_ftp_phase``, ``ssamd_ftp_cloud``: ``include/ssamd.h``; ``ssamd_ftp_reference``,
``ssamd_stripe_centroids``: ``include/ssamd_active.h``; ``ssamd_ftp_carrier_phase``, ``ssamd_ftp_mapping_cloud``:
``include/ssamd_ftp_mapping.h``) -- and two more structured-light methods, Gray code (``GrayCode``) and phase shifting with
heterodyne unwrapping (``PhaseShift``).  No cv2 call anywhere.

    import simplestereo_amd as ss
    ftp = ss.active.StereoFTP(rig, ss.active.buildFringe(period, stripeColor="r"), period)
    cloud = ftp.getCloud(imgObj)                                        # float64 [H, W, 3], on the device if imgObj is

    stripe = ss.active.findCentralStripe(imgObj, "r", 0.5)              # float64 [H, 2] on the host, or None
    imgRef = ss.active.ftpReference(fringe, rig, z_plane, roi)          # uint8 [h, w]: the fringe as seen on the plane
    phase = ss.active.ftpPhase(imgObj, imgRef, fc, radius_factor=0.5, unwrap="iir", tau=0.8)
    phase = ss.active.ftpPhase(imgObj, imgRef, fc, unwrap="numpy")      # the reference's default unwrapping
    k = ss.active.ftpFringeOrder(phase, stripe_indexes, rig, z_plane, period, stripeCentralPeak)
    cloud = ss.active.ftpCloud(phase, rig, z_plane, period, k)         # float64 [H, W, 3], on the device if phase is

    cloud = ss.active.StereoFTP_Mapping(rig, fringe, period).getCloud(imgObj)       # no reference plane
    phase = ss.active.ftpCarrierPhase(imgObj, fc, unwrap="numpy")       # the phase of one image, carrier included
    theta = ss.active.ftpStripePhase(phase, stripe)                     # float: its mean along the stripe, bilinear
    cloud = ss.active.ftpMappingCloud(phase, rig, period, stripeCentralPeak, theta)
    phase, ph_obj, ph_ref = ss.active.StereoFTP_PhaseOnly(rig, fringe, period).getPhase(imgObj)

    points = ss.active.GrayCode(rig).getCloud(images)                   # float64 (n, 1, 3); images uint8 [N, H, W] or paths
    proj = ss.active.grayCodeDecode(images, rig.res2, white_thr=5)      # int32 [H, W, 2]: (xDec, yDec) or (-1, -1)

    points = ss.active.GrayCodeStereo(rig2cam, projRes).getCloud((stack1, stack2))  # float64 (n, 1, 3): two cameras, one projector
    pairs = ss.active.grayCodeMatch(proj1, proj2, projRes, reduce="mean")           # float64 [Hp, Wp, 4]: (x1, y1, x2, y2) or NaN
    points = ss.active.stereoTriangulate(rig2cam, points1, points2)                 # float64 (n, 1, 3): any camera-camera couples

    patterns = ss.active.phaseShiftPattern(periods, rig.res2)           # uint8 [4 (nx + ny), Hp, Wp]
    cloud = ss.active.PhaseShift(rig, periods).getCloud(images)         # float64 [H, W, 3], NaN where masked
    proj = ss.active.phaseShiftDecode(images, periods, rig.res2)        # float64 [H, W, 2]: (px, py)
    points = ss.StructuredLightRig(rig).triangulate(camPoints, proj)    # float64 (n, 1, 3): any correspondences

``ftpPhase`` is the demodulation of ``StereoFTP.getCloud`` (``active.py:675-737``; the same lines are
``StereoFTP_PhaseOnly.getPhase``, ``:2012-2074``): gray by the channel maximum, a row-wise FFT of the object image and of
the (virtual) reference image, the per-row band-pass around the carrier ``fc``, an inverse FFT and
``angle(ghat * conj(g0hat))`` -- optionally followed by the unwrapper the reference passes as ``unwrappingMethod``
(``unwrap="iir"``) or by what it runs when none is passed, ``np.unwrap`` along x and then along y (``unwrap="numpy"``,
``active.py:739-745``).
Its inputs come from ``ftpReference`` (the virtual reference image of ``_getProjectorMapping``, ``active.py:459-490``:
``cv2.projectPoints`` and ``cv2.remap(INTER_CUBIC)`` there, one HIP kernel here) and, for ``fc``, from
``StereoFTP._calculateCameraFrequency``.

``ftpCloud`` is the triangulation that ends ``StereoFTP.getCloud`` (``active.py:776-841``, with the projector coordinates
of ``_getProjectorMapping``, ``:463-485``): ``cv2.projectPoints`` of every pixel centre onto the projector, phase to projector
column, the epipolar line, ``cv2.undistortPoints``, two rectifying homographies, disparity to depth and the common
rotation undone -- per pixel, in fp64, in one kernel, so that camera frame -> phase -> unwrapped phase -> cloud stays in HBM.
``ftpFringeOrder`` is the one step between the two that needs the central stripe (``active.py:779-788``); ``ftpGeometry``
packs what both read from the rig.

``StereoFTP`` composes them in the reference's order (``active.py:608-841``): ``cv2.undistort`` of the frame (a bilinear
remap on the maps of ``initUndistortRectifyMap``), ``findCentralStripe`` (per-row centroids by one HIP kernel; only the H
centroids come to the host), ``_triangulate`` and ``_calculateCameraFrequency`` (O(H) numpy on the host: ``z_plane``,
``fc``), ``ftpReference``, ``ftpPhase``, ``ftpFringeOrder``, ``ftpCloud``.  Where the reference calls cv2, OpenCV's published
arithmetic is restated; parity with cv2 itself is pinned only where cv2 is installed (``tests/test_cv2_pins_ftp.py``): the
bicubic weight table (``_rigs._cubic_table`` lists its choices), ``cv2.undistort``, the float32 roundings of
``_calculateCameraFrequency``.

``StereoFTP_Mapping`` is the classic method without a reference plane (``active.py:1266-1450``; C ABI in
``include/ssamd_ftp_mapping.h``): ``ftpCarrierPhase`` (``np.angle(ifft(bandpass(fft(gray))))`` of the object image alone, the
one-image form of ``ftpPhase``'s kernel), ``ftpStripePhase`` (the phase at the central stripe, ``map_coordinates`` restated on
the host) and ``ftpMappingCloud`` (phase to projector column, the epipolar line of the fundamental matrix and the triangulation
``ftpCloud`` ends with, per pixel in one kernel; ``ftpMappingGeometry`` packs what it reads).  ``StereoFTP_PhaseOnly.getPhase``
(``:1950-2074``) returns the three wrapped maps of the demodulation.  ``StereoFTPAnaglyph`` stays out: its ``convertGrayscale``
makes a float64 fringe, which takes ``cv2.remap(INTER_CUBIC)`` down OpenCV's floating-point path, and the reference marks the
class as work in progress.

``GrayCode`` (alias ``GrayCodeSingle``) is the reference's other structured-light method (``active.py:1130-1263``; C ABI in
``include/ssamd_graycode.h``).  There ``getCloud`` calls ``cv2.structured_light_GrayCodePattern.getProjPixel`` once per camera
pixel from a Python double loop; here three HIP kernels do the work: ``graycode_decode_kernel`` (``cv2.undistort`` of every
pattern image fused in, ``getProjPixel`` for every pixel, valid pixels counted per block), ``graycode_scan_kernel`` (where each
block's points start) and ``graycode_cloud_kernel`` (the triangulation ``ftpCloud`` ends with, by the same device function,
written compacted in raster order, or dense with NaN).  ``grayCodeDecode`` is the decode on its own; ``grayCodePattern`` and
``generateGrayCodeImgs`` make the pattern images.  OpenCV's published algorithm is restated (``tests/_graycode_ref.py``);
parity with cv2 itself is pinned only where ``cv2.structured_light`` is installed (``tests/test_cv2_pins_graycode.py``).
``roi`` is read as the reference's loops read it, ``range(roi_y, roi_h)`` and ``range(roi_x, roi_w)``: (x, y, x_end, y_end).
``GrayCodeDouble`` stays out: the reference's version cannot run (it indexes a projector-shaped array with camera coordinates,
adds 0.5 to an integer array in place and uses a ``self.R_inv`` it never defines); ``grayCodeDecode`` of the two cameras' stacks
is the piece to write one's own from.

``GrayCodeStereo`` is what that class sets out to do -- conventional active stereo, two calibrated cameras and one uncalibrated
projector (``active.py:1463-1608``; C ABI in ``include/ssamd_graycode_stereo.h``) -- under a name of its own, since it is no
drop-in for code that never ran.  Its loops are kept, with the indices the right way round: each camera's stack is decoded
(``grayCodeDecode``, the maps of ``cv2.undistort(img, K_i, distCoeffs_i)`` fused in), each camera's decoded map is inverted into a
projector-shaped table (``graycode_scatter_kernel``: a scatter with integer atomics, ``reduce="last"`` the reference's
overwriting loop as an atomic max on the raster index, ``reduce="mean"`` the exact centroid from 64-bit integer sums), a projector
pixel seen by BOTH cameras gives a couple of pixel centres (``graycode_match_kernel``; ``grayCodeMatch`` is scatter and match on
their own), and the couples are triangulated camera against camera (``graycode_stereo_cloud_kernel``: ``Rectify1``, ``Rectify2``,
``baseline * (p1 / |disparity|)``, the common rotation undone, ``active.py:1594-1606`` -- the end of ``ftpCloud``'s triangulation,
by the same device function, without ``undistortPoints``; ``stereoTriangulate`` is that step for couples of any origin).  No
float atomics: every result is the same bytes on every run.  A couple with zero disparity gives inf / NaN, as in the reference.

``PhaseShift`` is phase shifting with heterodyne unwrapping [Reich 1997], the third decoding method of the reference, which
writes it out in ``calibration.phaseShift`` (``calibration.py:656-687`` and ``:726-738``; C ABI in
``include/ssamd_structured_light.h``) and uses it on chessboard corners only.  ``phaseShiftDecode`` runs those three closures --
the four-step wrapped phase, the period-to-period ``unwrap``, ``getProjCoord`` -- on every camera pixel
(``phaseshift_decode_kernel``: a dense correspondence map), ``phaseShiftPattern`` makes the images with ``buildFringe``, and
``PhaseShift.getCloud`` ends with ``StructuredLightRig.triangulate`` (``sl_triangulate_kernel``: the reference's general entry
point for correspondences of any origin, by the device function ``ftpCloud`` ends with) on the pixel grid.  Camera pixels and
projector coordinates carry no half-pixel offsets there, the convention of that calibration routine.

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

``ftpReference``, ``findCentralStripe`` and ``StereoFTP.getCloud``:

=========================================================  =======================
condition                                                  exception
=========================================================  =======================
the fringe, image or frame neither ndarray nor CUDA/HIP    ``TypeError``
tensor, or not uint8
the fringe not [Hp, Wp] or [Hp, Wp, 3], or without pixels  ``ValueError``
``z_plane`` not a finite number; ``roi`` outside ``res1``  ``ValueError``
``sensitivity`` outside [0, 1]                             ``ValueError("Threshold must be in the interval [0,1]!")``
``color`` not 'b', 'g', 'r', 'blue', 'green', 'red'        ``ValueError("Color value not permitted!")``
the image of ``findCentralStripe`` not [H, W, 3]           ``ValueError``
fewer than two rows with a stripe (scipy's error)          ``ValueError``
``interpolation`` other than 'linear' without scipy        ``NotImplementedError``
a frame that is not 3-D                                    ``ValueError("image must be a BGR color image!")``
a frame that is not of the rig's ``res1``                  ``ValueError``
no row of the frame holds a stripe                         ``ValueError("Central stripe not found in image!")``
``plot=True``                                              ``NotImplementedError``
=========================================================  =======================

``ftpCarrierPhase`` raises what ``ftpPhase`` raises (first table); ``StereoFTP_Mapping.getCloud`` and
``StereoFTP_PhaseOnly.getPhase`` what ``StereoFTP.getCloud`` raises.  ``ftpStripePhase``, ``ftpMappingGeometry`` and
``ftpMappingCloud``:

=========================================================  =======================
condition                                                  exception
=========================================================  =======================
the phase neither ndarray nor CUDA/HIP tensor, or not      ``TypeError``
float64
the phase not [H, W], without pixels (``ftpStripePhase``)  ``ValueError``
or (W, H) not the ``roi``'s (``ftpMappingCloud``)
``stripe`` not a finite float array [n >= 1, 2]            ``ValueError``
``roi`` not four non-negative integers inside ``res1``     ``ValueError``
``period``, ``stripeCentralPeak`` or ``theta_shift`` not   ``ValueError``
a finite number, or ``period == 0``
``distCoeffs2`` with a tilted sensor (tauX, tauY)          ``NotImplementedError``
an ``ftpGeometry`` result in place of the rig, or a        ``ValueError``
packed geometry together with ``period`` or ``roi``
=========================================================  =======================

``grayCodePattern``, ``generateGrayCodeImgs``, ``grayCodeDecode``, ``GrayCode`` and ``GrayCode.getCloud``:

=========================================================  =======================
condition                                                  exception
=========================================================  =======================
a resolution (``rig.res2`` too) that is not two integers   ``ValueError``
in 1 .. 65536
``images`` neither ndarray, CUDA/HIP tensor nor a list or  ``TypeError``
tuple of ndarrays (of paths too for ``getCloud``), or not
uint8
``images`` not [M, Hc, Wc], a listed image not [Hc, Wc]    ``ValueError``
fewer images than the projector has patterns               ``ValueError``
``white_thr`` not an integer in 0 .. 256                   ``ValueError``
``maps`` not a pair, a map not [Hc, Wc]                    ``ValueError``
a map neither ndarray nor tensor, not float32, or on a     ``TypeError``
device the images are not on
``roi`` not four integers, a negative origin, or a         ``ValueError``
non-empty region reaching outside the image
``getCloud``: an image that is not of ``res1``             ``ValueError("Image size of {name or index} is mismatch!")``
``getCloud``: a file that is not 8-bit single-channel      ``ValueError`` (pass arrays)
``distCoeffs2`` with a tilted sensor (tauX, tauY)          ``NotImplementedError``
PIL absent: ``generateGrayCodeImgs``, a list of paths      ``ImportError``
=========================================================  =======================

``grayCodeMatch``, ``stereoTriangulate``, ``GrayCodeStereo`` and ``GrayCodeStereo.getCloud`` (each stack, ``white_thr`` and each
``roi`` as in the table above):

=========================================================  =======================
condition                                                  exception
=========================================================  =======================
``projRes`` not two integers in 1 .. 65536, or of 2^31     ``ValueError``
pixels or more
``reduce`` neither ``"last"`` nor ``"mean"``               ``ValueError``
a decoded map neither ndarray nor CUDA/HIP tensor, or not  ``TypeError``
int32
a decoded map not [h, w, 2]                                ``ValueError``
an origin not two integers >= 0; a map of 2^31 pixels or   ``ValueError``
more, or reaching that far from the origin
one input on the host and one on a device, or on two       ``TypeError``
devices (maps, points, stacks)
``rig`` not a ``StereoRig``                                ``ValueError("Invalid argument!")``
points neither ndarray nor tensor, or not of a real dtype  ``TypeError``
points whose last dimension is not 2, or of two counts     ``ValueError``
a rig whose geometry is not finite                         ``ValueError``
``images`` neither (stack1, stack2) nor a sequence of      ``TypeError``
(path1, path2) couples
``getCloud``: an image not of ``res1`` / ``res2``          ``ValueError("Image size of {name or index} is mismatch!")``
=========================================================  =======================

``phaseShiftPattern``, ``phaseShiftDecode``, ``PhaseShift`` and ``PhaseShift.getCloud`` (images, maps and the resolution as in the
table above):

=========================================================  =======================
condition                                                  exception
=========================================================  =======================
``periods`` not a pair of sequences of 1 .. 8              ``ValueError``
(``MAX_PERIODS``) finite positive numbers
fewer images than ``4 * (nx + ny)``                        ``ValueError``
``min_modulation`` neither ``None`` nor a number >= 0      ``ValueError``
``roi`` not four non-negative integers (x, y, width,       ``ValueError``
height) inside the image
``rig`` not a ``StereoRig``                                ``ValueError("Invalid argument!")``
``getCloud``: an image that is not of ``res1``             ``ValueError("Image size of {index} is mismatch!")``
``getCloud``: a rig whose geometry is not finite           ``ValueError``
``distCoeffs2`` with a tilted sensor (tauX, tauY)          ``NotImplementedError``
=========================================================  =======================

All of them are raised before any native call.  An image or a phase map with no rows or no columns gives an empty array;
``findCentralStripe`` of such an image is ``None``; an empty ``roi`` gives ``(0, 1, 3)`` points.
"""
import ctypes
import math
import numbers
import os

import numpy as np

from . import _native
from ._rigs import (INTER_LINEAR, NGEOM, StereoRig, StructuredLightRig, _cached_maps, _dist_vector, _distort, _low_level_rectify, _r_inv4, _remap,
                    _triangulation_geom, _triangulation_geometry, _undistort_device, _undistort_points)
from ._native import c_double as _c_double, is_device_tensor as _is_device_tensor

__all__ = ["ftpPhase", "ftpCloud", "ftpFringeOrder", "ftpGeometry", "FtpGeometry", "MAX_WIDTH", "ftpReference",
           "findCentralStripe", "buildFringe", "StereoFTP", "grayCodePattern", "generateGrayCodeImgs", "grayCodeDecode", "GrayCode",
           "GrayCodeSingle", "MAX_PROJECTOR", "ftpCarrierPhase", "ftpStripePhase", "ftpMappingCloud", "ftpMappingGeometry",
           "FtpMappingGeometry", "StereoFTP_Mapping", "StereoFTP_PhaseOnly", "phaseShiftPattern", "phaseShiftDecode", "PhaseShift",
           "MAX_PERIODS", "grayCodeMatch", "stereoTriangulate", "GrayCodeStereo"]

MAX_WIDTH = 8192          # SSAMD_FTP_MAX_W: twiddle table, gray rows and a chunk of bins of one row in 160 KiB of LDS
MAX_PROJECTOR = 65536     # Gray code: at most 16 bits per projector axis, 64 pattern images


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


def _unwrap_mode(unwrap, tau, w):
    """The checks ``ftpPhase`` and ``ftpCarrierPhase`` end with -> (the library's ``unwrap`` code, tau)"""
    if unwrap is not None and not (isinstance(unwrap, str) and unwrap in ("iir", "numpy")):
        raise ValueError('unwrap must be None, "iir" or "numpy"')
    t = 1.0
    if unwrap == "iir":
        t = _c_double(tau)
        if t < 0 or t > 1:
            raise ValueError("Wrong tau value!")
    if w > MAX_WIDTH:
        raise ValueError("rows wider than %d columns are not supported (width %d)" % (MAX_WIDTH, w))
    return {None: 0, "iir": 1, "numpy": 2}[unwrap], t


def ftpPhase(imgObj, imgRef, fc, radius_factor=0.5, unwrap=None, tau=1):
    """
    Phase of a fringe image against a reference fringe image by Fourier-transform profilometry.

    The demodulation of the reference's ``StereoFTP.getCloud`` (``active.py:675-737``): for every image row, the spectrum
    of the object image and of the reference image is cut to the band ``[fc - radius_factor*fc, fc + radius_factor*fc]``
    (bins of ``np.fft.fftfreq(W)``, bounds included), transformed back, and the phase is
    ``angle(ghat * conj(g0hat))``.  It is not ``StereoFTP`` but one step of :class:`StereoFTP`: called on its own, the
    reference image is :func:`ftpReference`'s and ``fc`` and the triangulation of the phase are the caller's.

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
    uw, t = _unwrap_mode(unwrap, tau, w)
    return _native.run("ssamd_ftp_phase", (obj, ref), (h, w),
                       lambda o, r, out: (o, ch_obj, r, ch_ref, h, w, fmin.ctypes.data, fmax.ctypes.data, uw, t, out), _INVALID)


def ftpCarrierPhase(img, fc, radius_factor=0.5, unwrap=None, tau=1):
    """
    Phase of one fringe image by Fourier-transform profilometry: ``np.angle(ifft(bandpass(fft(gray))))``.

    The demodulation of the reference's ``StereoFTP_Mapping.getCloud`` (``active.py:1354-1401``) and the second and third
    result of ``StereoFTP_PhaseOnly.getPhase`` (``:2067-2074``): :func:`ftpPhase` without a reference image -- the same
    band, the same band-limited direct DFT in fp64 (``ftp_carrier_kernel``), the angle of ``ghat`` itself.  The carrier is
    still in it: along a row the phase grows by about ``2 * pi * fc`` per pixel, so it is the unwrapped map that is of use.

    Parameters
    ----------
    img : ndarray or CUDA/HIP tensor, uint8
        ``[H, W]`` gray or ``[H, W, 3]`` BGR (reduced by the channel maximum, the reference's ``convertGrayscale``).
    fc, radius_factor, unwrap, tau
        As in :func:`ftpPhase`.

    Returns
    -------
    ndarray or tensor
        float64 ``[H, W]``: a new array, or a tensor on the image's device computed on its current stream.  A row whose band
        holds no bin is 0.0.
    """
    src, h, w, ch = _image(img, "img")
    fmin, fmax = _band(fc, radius_factor, h)
    uw, t = _unwrap_mode(unwrap, tau, w)
    return _native.run("ssamd_ftp_carrier_phase", (src,), (h, w),
                       lambda i, out: (i, ch, h, w, fmin.ctypes.data, fmax.ctypes.data, uw, t, out), _INVALID)


# ------------------------------------------------------------------------------------------------ phase -> point cloud
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
    g = _triangulation_geom(rig, dist, rect1, rect2, np.linalg.inv(common))
    g[0:9] = M.ravel()
    g[9:12] = T
    g[37:39] = ep[:2]
    g[39] = 2 * np.pi * fp
    if not np.isfinite(g).all():
        raise ValueError("the rig, z_plane and period give a geometry that is not finite")
    return FtpGeometry(g, box, fp)


def _geometry(rig, z_plane, period, roi):
    if isinstance(rig, FtpGeometry):
        if z_plane is not None or period is not None or roi is not None:
            raise ValueError("with a packed geometry in place of the rig, z_plane, period and roi are the geometry's: pass None")
        return rig
    return ftpGeometry(rig, z_plane, period, roi)


def _phase_dims(phase):
    """(H, W) of a float64 [H, W] array or device tensor"""
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
    return int(phase.shape[0]), int(phase.shape[1])


def _phase_map(phase, box):
    """-> (map, is it on a device), checked against the roi"""
    h, w = _phase_dims(phase)
    if (w, h) != (box[2], box[3]):
        raise ValueError("phaseUnwrapped is %d x %d but the roi is %d x %d (width x height)" % (w, h, box[2], box[3]))
    return phase, _is_device_tensor(phase)


def _cloud_phase(phase, box):
    """The checked map as the cloud kernels read it: a tensor contiguous and, for their 16-byte loads of two phases, aligned"""
    phase, dev = _phase_map(phase, box)
    if dev:
        phase = phase.contiguous()
        if phase.data_ptr() % 16:
            phase = phase.clone()     # a view at an odd storage offset
    return phase


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
    a half rounded down.  A step of :class:`StereoFTP`; on its own, the stripe is :func:`findCentralStripe`'s and ``z_plane``
    and ``stripeCentralPeak`` are the caller's.

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
    fp64 throughout (``ftp_cloud_kernel``).  A step of :class:`StereoFTP`; on its own, the phase and ``k`` come from
    ``ftpPhase`` and ``ftpFringeOrder`` and ``z_plane`` is the caller's.  Not bit-identical to cv2 (another operation order).

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
    phase = _cloud_phase(phaseUnwrapped, G.roi)
    x0, y0, w, h = G.roi
    return _native.run("ssamd_ftp_cloud", (phase,), (h, w, 3), lambda src, out: (src, h, w, x0, y0, G.geom.ctypes.data, order, out), _INVALID)


# ------------------------------------------------------------------------------------------------ the front end: StereoFTP
def _getCentralPeak(length, period, shift=0):
    """Column of the brightest pixel of the central stripe of a :func:`buildFringe` fringe (``active.py:67-84``)."""
    k = (length / 2) // period
    return period * (k - shift / (2 * np.pi))


_STRIPE_CHANNEL = {"b": 0, "blue": 0, "g": 1, "green": 1, "r": 2, "red": 2}


def buildFringe(period, shift=0, dims=(1280, 720), vertical=False, stripeColor=None, dtype=np.uint8):
    """
    Build a sinusoidal fringe image (the reference's ``buildFringe``, ``active.py:87-148``, the same formulas bit for bit).

    Parameters
    ----------
    period : float
        Fringe period along the x axis, in pixels.
    shift : float, optional
        Shift of the cosine's argument, in pixels.  Default 0.
    dims : tuple, optional
        Image dimensions as (width, height).  Default (1280, 720).
    vertical : bool, optional
        Build the fringe along the vertical.  Default False.
    stripeColor : str, optional
        'blue', 'green', 'red' (or 'b', 'g', 'r'): the central period keeps that channel only, and the image is BGR.
        Default None: a gray image without stripe.
    dtype : numpy.dtype, optional
        An integer type scales the fringe to its maximum.  Default ``np.uint8``.

    Returns
    -------
    numpy.ndarray
        ``[height, width]``, or ``[height, width, 3]`` with a stripe.
    """
    if vertical is True:
        dims = (dims[1], dims[0])
    row = ((1 + np.cos(2 * np.pi * (1 / period) * (np.arange(dims[0], dtype=float) + shift))) / 2)[np.newaxis, :]
    if np.dtype(dtype).char in np.typecodes["AllInteger"]:
        row *= np.iinfo(dtype).max
    if stripeColor is not None:
        if stripeColor not in _STRIPE_CHANNEL:
            raise ValueError("stripeColor value not permitted!")
        row = np.repeat(row[:, :, np.newaxis], 3, axis=2)
        peak = _getCentralPeak(dims[0], period, shift)
        left = int(peak - period / 2)
        right = int(left + period)
        keep = _STRIPE_CHANNEL[stripeColor]
        for ch in range(3):
            if ch != keep:
                row[0, left:right, ch] = 0
    full = np.repeat(row.astype(dtype), dims[1], axis=0)
    if vertical is True:
        full = np.rot90(full, k=3, axes=(0, 1))
    return full


def _gray(img):
    """``StereoFTP.convertGrayscale`` of a checked image: the channel maximum of BGR, a gray image as it is"""
    if img.ndim == 2:
        return img
    return img.amax(dim=2) if _is_device_tensor(img) else np.max(img, axis=2)


def ftpReference(fringe, rig, z_plane=None, roi=None, period=None):
    """
    Virtual reference image: the fringe as the camera would see it on the reference plane at ``z_plane``.

    The integer-grid half of the reference's ``StereoFTP._getProjectorMapping`` (``active.py:459-490``): for every camera
    pixel ``(x, y)`` of the roi -- integer coordinates, no ``+ 0.5`` -- ``cv2.projectPoints`` onto the projector with
    ``z_plane * R.dot(inv(K1))`` as the 3x3 rotation (the operations of ``ftpCloud``, fp64), the two coordinates rounded to
    float32, and ``cv2.remap(fringe, mapx, mapy, INTER_CUBIC)`` with a constant border 0 in OpenCV's published 8-bit
    arithmetic: 1/32-pixel fractions, 4 x 4 taps with the 15-bit integer weights of ``initInterTab2D`` (restated in
    ``_rigs._cubic_table``, where every choice is listed), ``clip((sum + (1 << 14)) >> 15, 0, 255)``.  Pixels whose map
    coordinates are not finite, or lie wholly outside the fringe, are 0.  One HIP kernel (``ftp_reference_kernel``); equal
    byte for byte to ``_rigs._remap(fringe, mapx, mapy, INTER_CUBIC)`` on the maps of the numpy restatement.  Parity with
    cv2 itself is not pinned.

    Parameters
    ----------
    fringe : ndarray or CUDA/HIP tensor, uint8
        ``[Hp, Wp]`` gray or ``[Hp, Wp, 3]`` BGR (reduced by the channel maximum, ``convertGrayscale``), at least one pixel.
    rig : StereoRig
        Camera in position 1, projector in position 2 -- or an :func:`ftpGeometry` result, with ``z_plane`` and ``roi`` left
        ``None``.
    z_plane : float
        Distance of the reference plane from the camera.
    roi : (x, y, width, height), optional
        Region of the camera image to build.  Default: the whole ``rig.res1``.
    period : optional
        Not read (the reference image does not depend on it); accepted so that the arguments of ``ftpCloud`` can be passed.

    Returns
    -------
    ndarray or tensor
        uint8 ``[height, width]``: a new array, or a tensor on the fringe's device computed on its current stream.
    """
    if isinstance(rig, FtpGeometry):
        if z_plane is not None or roi is not None:
            raise ValueError("with a packed geometry in place of the rig, z_plane and roi are the geometry's: pass None")
        G = rig
    else:
        G = ftpGeometry(rig, z_plane, 1.0, roi)
    fr, hp, wp, _ = _image(fringe, "fringe")
    if hp == 0 or wp == 0:
        raise ValueError("fringe must have at least one pixel")
    fr = _gray(fr)
    x0, y0, w, h = G.roi
    return _native.run("ssamd_ftp_reference", (fr,), (h, w),
                       lambda src, out: (src, hp, wp, h, w, x0, y0, G.geom.ctypes.data, out), _INVALID, dtype=np.uint8)


def _fill_linear(y, x):
    """``scipy.interpolate.interp1d(y[valid], x[valid], kind="linear", fill_value="extrapolate")(y)`` in numpy, scipy's own
    formula (``interp1d._call_linear``): every row -- the valid ones too -- is ``slope * (y - y_lo) + x_lo`` on the pair of
    knots around it (the first or last pair outside them), so a valid row may differ from its centroid in the last bit."""
    valid = ~np.isnan(x)
    ky, kx = y[valid], x[valid]
    if ky.size < 2:
        raise ValueError("x and y arrays must have at least 2 entries")          # scipy's message
    hi = np.searchsorted(ky, y).clip(1, ky.size - 1).astype(int)
    lo = hi - 1
    slope = (kx[hi] - kx[lo]) / (ky[hi] - ky[lo])
    return slope * (y - ky[lo]) + kx[lo]


def findCentralStripe(image, color="r", sensitivity=0.5, interpolation="linear"):
    """
    Find the coordinates of a coloured vertical stripe in the image, with subpixel accuracy along x (the reference's
    ``findCentralStripe``, ``active.py:272-345``).

    Per row, the chosen channel is zeroed where ``value < 255 * sensitivity`` and the centroid ``sum(v * x) / sum(v)`` is
    taken: one HIP kernel (``stripe_centroid_kernel``), exact integer sums and one fp64 division, numpy's result bit for
    bit; only the H centroids come to the host.  Rows without stripe are filled by linear interpolation over the rows,
    extrapolated at both ends: scipy's ``interp1d`` formula restated in numpy (``_fill_linear``), bit for bit.

    Parameters
    ----------
    image : ndarray or CUDA/HIP tensor, uint8 ``[H, W, 3]``
        BGR image with a coloured vertical stripe.
    color : str, optional
        'blue', 'green' or 'red' (or 'b', 'g', 'r').  Default 'r'.
    sensitivity : float, optional
        Sensitivity of the colour match in [0, 1].  Default 0.5.
    interpolation : str, optional
        ``kind`` of ``scipy.interpolate.interp1d``.  ``'linear'`` needs no scipy; any other kind is handed to scipy and is
        ``NotImplementedError`` where scipy is not installed.

    Returns
    -------
    numpy.ndarray or None
        float64 ``[H, 2]``: (x, y) of the stripe centre in every row (y = row + 0.5), on the host; ``None`` when no row
        holds a stripe.
    """
    if not (sensitivity >= 0 and sensitivity <= 1):
        raise ValueError("Threshold must be in the interval [0,1]!")
    img, h, w, ch = _image(image, "image")
    if ch != 3:
        raise ValueError("image must be [H, W, 3] (BGR)")
    if not isinstance(color, str) or color not in _STRIPE_CHANNEL:
        raise ValueError("Color value not permitted!")
    # uint8 < fp64 product (active.py:319-320) <=> uint8 < ceil(product): the integer threshold the kernel compares with
    threshold = int(np.ceil(255 * float(sensitivity)))
    if w == 0:
        return None
    x = _native.run("ssamd_stripe_centroids", (img,), (h,),
                    lambda src, out: (src, h, w, _STRIPE_CHANNEL[color], threshold, out), _INVALID)
    if _is_device_tensor(x):
        x = x.cpu().numpy()
    if np.isnan(x).all():
        return None
    y = np.arange(0.5, h, 1)
    if interpolation == "linear":
        x = _fill_linear(y, x)
    else:
        try:
            from scipy.interpolate import interp1d
        except ImportError:
            raise NotImplementedError("interpolation=%r needs scipy, which is not installed: only 'linear' is built in"
                                      % (interpolation,)) from None
        valid = ~np.isnan(x)
        x = interp1d(y[valid], x[valid], kind=interpolation, fill_value="extrapolate")(y)
    return np.vstack((x, y)).T


def _project_points(P, R, T, K, dist):
    """``cv2.projectPoints(P [n, 3], R (3x3), T, K, dist)`` -> [n, 2], the published camera model in fp64 numpy"""
    X = P.dot(np.asarray(R, dtype=np.float64).T) + np.asarray(T, dtype=np.float64).reshape(1, 3)
    xd, yd = _distort(X[:, 0] / X[:, 2], X[:, 1] / X[:, 2], _dist_vector(dist))
    return np.stack([K[0, 0] * xd + K[0, 2], K[1, 1] * yd + K[1, 2]], axis=1)


def _perspective(pts, H):
    """``cv2.perspectiveTransform`` of [n, 2] points with a 3x3 matrix"""
    q = np.hstack((pts, np.ones((pts.shape[0], 1)))).dot(H.T)
    return q[:, :2] / q[:, 2:]


class StereoFTP:
    """
    Manager of the Stereo Fourier Transform Profilometry (the reference's ``StereoFTP``, ``active.py:351-841``): camera
    frame in, point cloud out, with no cv2 call.

    Parameters
    ----------
    stereoRig : StereoRig
        Camera in position 1 (world origin), projector in position 2.
    fringe : numpy.ndarray
        BGR image projected by the projector (:func:`buildFringe` with a ``stripeColor``), uint8.
    period : float
        Period of the fringe, in pixels.
    shift : float, optional
        Shift used to build the fringe.  Default 0.
    stripeColor : str, optional
        Colour of the central stripe: 'blue', 'green', 'red' or 'b', 'g', 'r'.  Default 'red'.
    stripeSensitivity : float, optional
        Sensitivity to find the stripe, see :func:`findCentralStripe`.  Default 0.5.

    The attributes are the reference's: ``fringe`` (gray), ``fringeDims``, ``fp``, ``stripeCentralPeak``, ``F``,
    ``Rectify1``, ``Rectify2``, ``ep``, ``R_inv``.  The gray fringe and the undistortion maps of the camera go to a device
    once per instance, the bicubic weight table once per device.
    """

    def __init__(self, stereoRig, fringe, period, shift=0, stripeColor="red", stripeSensitivity=0.5):
        self.stereoRig = stereoRig
        self.fringe = self.convertGrayscale(fringe)
        self.fringeDims = fringe.shape[:2][::-1]
        self.period = period
        self.fp = 1 / period
        self.stripeColor = stripeColor
        self.stripeSensitivity = stripeSensitivity
        self.stripeCentralPeak = _getCentralPeak(self.fringeDims[0], period, shift)
        self.F = self.stereoRig.getFundamentalMatrix()
        self.Rectify1, self.Rectify2, commonR = _low_level_rectify(stereoRig)
        ep = self.stereoRig.intrinsic2.dot(self.stereoRig.T)
        self.ep = ep / ep[2]
        self.R_inv = _r_inv4(commonR)
        self._cache = {}                 # _cached_maps' entries, and per device (gray fringe, mapx, mapy) tensors

    @staticmethod
    def convertGrayscale(img):
        """Grayscale by the channel maximum: the stripe (0, 0, 255) becomes white, which the FFT needs."""
        return np.max(img, axis=2)

    def _device_state(self, device):
        if str(device) not in self._cache:
            import torch
            self._cache[str(device)] = ((torch.from_numpy(np.ascontiguousarray(self.fringe)).to(device),)
                                        + _cached_maps(self._cache, self.stereoRig, device))
        return self._cache[str(device)]

    def _host_maps(self):
        return _cached_maps(self._cache, self.stereoRig)

    def _undistort(self, img):
        """``cv2.undistort(img, K1, distCoeffs1)``: the float32 maps of ``initUndistortRectifyMap(K1, D1, I, K1, res1)`` and a
        bilinear remap with a constant border 0 -- ``remap_bgr_kernel`` on a device frame, ``_rigs._remap`` on a host frame
        (the same bytes).  Parity with cv2 is not pinned."""
        if not _is_device_tensor(img):
            mx, my = self._host_maps()
            return _remap(img, mx, my, INTER_LINEAR)
        return _undistort_device(self._cache, self.stereoRig, img)

    def _triangulate(self, camPoints, p_x, roi):
        """
        For each undistorted camera point and the projector column ``p_x`` it corresponds to, the 3-D point
        (``active.py:561-605``), O(n) numpy on the host: the projector row from the epipolar line of ``F``, the camera point
        through ``Rectify1``, the projector point through ``cv2.undistortPoints(P=K2)`` (``_rigs._undistort_points``) and
        ``Rectify2``, ``baseline / |disparity|`` and the common rotation undone.  fp64 throughout, as the reference is for
        its float64 stripe; ``camPoints`` is not modified (the reference adds the roi offset in place).  Parity with cv2 is
        not pinned.
        """
        rig = self.stereoRig
        cam = np.array(camPoints, dtype=np.float64).reshape(-1, 2)
        n = cam.shape[0]
        cam[:, 0] += roi[0]
        cam[:, 1] += roi[1]
        lines = np.hstack((cam, np.ones((n, 1)))).dot(self.F.T)
        p_x = np.full((n,), p_x, dtype=np.float64) if np.isscalar(p_x) else np.asarray(p_x, dtype=np.float64).flatten()
        p_y = -(lines[:, 0] * p_x + lines[:, 2]) / lines[:, 1]
        pc = _perspective(cam, self.Rectify1)
        pp = _undistort_points(np.stack([p_x, p_y], axis=1), rig.intrinsic2, rig.distCoeffs2, R=rig.intrinsic2)
        pp = _perspective(pp, self.Rectify2)
        disparity = np.abs(pp[:, [0]] - pc[:, [0]])
        pw = rig.getBaseline() * (np.hstack((pc, np.ones((n, 1)))) / disparity)
        return pw.dot(np.ascontiguousarray(self.R_inv[:3, :3]).T)

    def _calculateCameraFrequency(self, objPoints):
        """
        Carrier frequency on the camera of each object point (``active.py:495-559``), O(n) numpy on the host: the point on
        the projector, two points half a period to either side, back to the plane at the point's depth, onto the camera;
        ``1 / Tc`` with ``Tc`` from the first Euclid theorem.  The reference's dtypes are kept where they are observable:
        ``objPoints`` is cast to float32, and because cv2 returns float32 for float32 input, ``pCenter``
        (``cv2.projectPoints``) and the undistorted points (``cv2.undistortPoints``) are computed in fp64 and rounded to
        float32 at those two places.  Parity with cv2 is not pinned.
        """
        rig = self.stereoRig
        Ac, Ap = np.asarray(rig.intrinsic1, dtype=np.float64), np.asarray(rig.intrinsic2, dtype=np.float64)
        R, T = np.asarray(rig.R, dtype=np.float64), np.asarray(rig.T, dtype=np.float64)
        Op = (-np.linalg.inv(R).dot(T)).flatten()
        obj = np.asarray(objPoints).reshape(-1, 3).astype(np.float32)
        n = obj.shape[0]
        pCenter = _project_points(obj.astype(np.float64), R, T, Ap, rig.distCoeffs2).astype(np.float32)
        half = np.float32((1 / self.fp) / 2)
        points = np.vstack((np.stack([pCenter[:, 0] - half, pCenter[:, 1]], axis=1),
                            np.stack([pCenter[:, 0] + half, pCenter[:, 1]], axis=1)))
        und = _undistort_points(points.astype(np.float64), Ap, rig.distCoeffs2, R=Ap).astype(np.float32)
        pp = np.hstack((und, np.ones((2 * n, 1), dtype=np.float32)))
        z = np.tile(obj[:, 2].reshape(-1, 1), (2, 1))
        hh = np.linalg.inv(Ap.dot(R)).dot(pp.T).T
        s = (z - Op[2]) / hh[:, [2]]
        pw = s * hh + Op.reshape(1, 3)
        pc = _project_points(pw, np.eye(3), np.zeros(3), Ac, rig.distCoeffs1)
        a, b = pc[:n], pc[n:]
        Tc = ((a[:, 0] - b[:, 0]) ** 2 + (a[:, 1] - b[:, 1]) ** 2) / np.abs(a[:, 0] - b[:, 0])
        return 1 / Tc

    def _frame(self, imgObj, roi):
        """The checks and the first four steps of ``getCloud``: -> (undistorted roi cut, roi, stripe, stripe_indexes)"""
        if not (_is_device_tensor(imgObj) or isinstance(imgObj, np.ndarray)):
            raise TypeError("imgObj must be a uint8 ndarray or a CUDA/HIP torch.uint8 tensor")
        if imgObj.ndim != 3:
            raise ValueError("image must be a BGR color image!")
        img, h, w, _ = _image(imgObj, "imgObj")
        widthC, heightC = (int(v) for v in self.stereoRig.res1)
        if (w, h) != (widthC, heightC):
            raise ValueError("imgObj is %d x %d but the camera resolution is %d x %d (width x height)" % (w, h, widthC, heightC))
        box = _roi(roi, self.stereoRig.res1)
        cut = self._undistort(img)[box[1]:box[1] + box[3], box[0]:box[0] + box[2]]
        stripe = findCentralStripe(cut, self.stripeColor, self.stripeSensitivity)
        if stripe is None:
            raise ValueError("Central stripe not found in image!")
        return cut, box, stripe, np.ceil(stripe - 0.5).astype(np.int64)

    def getCloud(self, imgObj, radius_factor=0.5, roi=None, unwrappingMethod=None, plot=False):
        """
        Process a camera frame and get the point cloud (``active.py:608-841``).

        The reference's steps in its order: ``cv2.undistort`` of the frame (bilinear remap on the maps of
        ``initUndistortRectifyMap(K1, D1, I, K1)``), the roi cut, :func:`findCentralStripe`, the stripe's pixel indexes,
        ``_triangulate`` of the stripe -> ``z_plane`` (its mean depth), ``_calculateCameraFrequency`` -> ``fc``,
        :func:`ftpReference`, :func:`ftpPhase`, :func:`ftpFringeOrder`, :func:`ftpCloud`.  With a device tensor the frame,
        the reference image, the phase and the cloud stay on the device: what crosses to the host are the H stripe
        centroids and the H phase values at the stripe.

        Parameters
        ----------
        imgObj : ndarray or CUDA/HIP tensor, uint8 ``[H, W, 3]``
            BGR frame of the camera, of the rig's ``res1``.
        radius_factor : float, optional
            Radius factor of the pass band.  Default 0.5.
        roi : (x, y, width, height), optional
            Region of interest.  Default None: the whole frame.
        unwrappingMethod : callable, optional
            Takes the wrapped phase (an array or tensor like the frame) and returns it unwrapped, e.g.
            ``ss.unwrapping.infiniteImpulseResponse``.  Default None: ``np.unwrap`` along x, then y (``unwrap="numpy"``).
        plot : bool, optional
            ``True`` is ``NotImplementedError``: there is no display here.

        Returns
        -------
        ndarray or tensor
            float64 ``[height, width, 3]`` of the frame or the roi: an ndarray for a host frame, a tensor on the frame's
            device for a device frame.
        """
        if plot:
            raise NotImplementedError("plot=True needs cv2 windows and matplotlib, which this package does not use")
        cut, box, stripe, stripe_indexes = self._frame(imgObj, roi)
        stripe_world = self._triangulate(stripe, self.stripeCentralPeak, box)
        z_plane = np.mean(stripe_world[:, 2])
        fc = self._calculateCameraFrequency(stripe_world)
        G = ftpGeometry(self.stereoRig, z_plane, self.period, box)
        fringe = self._device_state(cut.device)[0] if _is_device_tensor(cut) else self.fringe
        imgRef = ftpReference(fringe, G)
        if unwrappingMethod is None:
            phase = ftpPhase(cut, imgRef, fc, radius_factor, unwrap="numpy")
        else:
            phase = unwrappingMethod(ftpPhase(cut, imgRef, fc, radius_factor))
        k = ftpFringeOrder(phase, stripe_indexes, G, stripeCentralPeak=self.stripeCentralPeak)
        return ftpCloud(phase, G, k=k)


# ------------------------------------------------------------------------------------------------ FTP without a reference plane
def ftpStripePhase(phaseUnwrapped, stripe):
    """
    Mean of the phase map along the central stripe, sampled bilinearly: ``theta_shift`` of ``StereoFTP_Mapping.getCloud``
    (``active.py:1431-1432``), ``np.mean(scipy.ndimage.map_coordinates(phase, (y, x), order=1))``.

    scipy's linear spline with ``mode='constant'`` restated in numpy on the 4 n neighbours: with ``i = floor(c)`` and
    ``t = c - i`` on each axis, ``((1-ty)(1-tx)) v00 + ((1-ty) tx) v01 + (ty (1-tx)) v10 + (ty tx) v11``; a point strictly
    outside ``[0, n - 1]`` on either axis contributes 0.0.  O(H) work on the host; of a device map the 4 n neighbours are
    read with one indexed read and one small copy.

    Parameters
    ----------
    phaseUnwrapped : ndarray or CUDA/HIP tensor, float64 ``[H, W]``
    stripe : float array ``[n >= 1, 2]``
        (x, y) of the stripe in the coordinates of the map's array indexes, as :func:`findCentralStripe` returns them
        (row ``r`` has ``y = r + 0.5``: the reference samples there).

    Returns
    -------
    float
    """
    dev = _is_device_tensor(phaseUnwrapped)
    h, w = _phase_dims(phaseUnwrapped)
    try:
        pts = np.asarray(stripe, dtype=np.float64)
    except (TypeError, ValueError):
        pts = np.zeros(0)
    if pts.ndim != 2 or pts.shape[1] != 2 or pts.shape[0] < 1 or not np.isfinite(pts).all():
        raise ValueError("stripe must be a finite float array [n >= 1, 2] of (x, y)")
    if h == 0 or w == 0:
        raise ValueError("phaseUnwrapped has no pixels")
    x, y = pts[:, 0], pts[:, 1]
    inside = (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
    xc, yc = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
    fx, fy = np.floor(xc), np.floor(yc)
    tx, ty = xc - fx, yc - fy
    ix0, iy0 = fx.astype(np.int64), fy.astype(np.int64)
    ix1, iy1 = np.minimum(ix0 + 1, w - 1), np.minimum(iy0 + 1, h - 1)          # (weight 0 where clipped)
    rows, cols = np.stack([iy0, iy0, iy1, iy1]), np.stack([ix0, ix1, ix0, ix1])
    if dev:
        import torch
        v = phaseUnwrapped[torch.from_numpy(rows).to(phaseUnwrapped.device), torch.from_numpy(cols).to(phaseUnwrapped.device)].cpu().numpy()
    else:
        v = phaseUnwrapped[rows, cols]
    val = ((((1 - ty) * (1 - tx)) * v[0] + ((1 - ty) * tx) * v[1]) + (ty * (1 - tx)) * v[2]) + (ty * tx) * v[3]
    return float(np.mean(np.where(inside, val, 0.0)))


class FtpMappingGeometry(FtpGeometry):
    """What ``ftpMappingCloud`` reads from a rig and a fringe period: ``geom`` (the ``SSAMD_FTP_CLOUD_NGEOM`` doubles with
    only the triangulation's entries and ``2 pi fp`` filled in), ``F`` (float64 [9], the fundamental matrix row by row) and
    ``roi = (x, y, w, h)``."""
    __slots__ = ("F",)

    def __init__(self, geom, roi, fp, F):
        super().__init__(geom, roi, fp)
        self.F = F


def ftpMappingGeometry(rig, period, roi=None):
    """
    Pack the geometry of :func:`ftpMappingCloud`: build it once per rig and pass it in place of ``rig``.

    What ``GrayCode`` packs -- K2, ``distCoeffs2``, the rectifying transforms and the common orientation of
    ``_lowLevelRectify``, its inverse, ``rig.getBaseline()`` -- plus ``2 * pi * fp`` with ``fp = 1 / period`` and
    ``rig.getFundamentalMatrix()``.  No reference plane and no epipole: a rig with ``T[2] == 0`` is fine.

    Returns
    -------
    FtpMappingGeometry
        ``.geom`` float64 [68], ``.F`` float64 [9], ``.roi`` (x, y, width, height).
    """
    per = _finite(period, "period")
    if per == 0:
        raise ValueError("period must not be 0")
    box = _roi(roi, rig.res1)
    dist = _dist_vector(rig.distCoeffs2)                      # NotImplementedError for a tilted sensor
    rect1, rect2, common = _low_level_rectify(rig)
    fp = 1 / per
    g = _triangulation_geom(rig, dist, rect1, rect2, np.linalg.inv(common))
    g[39] = 2 * np.pi * fp
    F = np.ascontiguousarray(np.asarray(rig.getFundamentalMatrix(), dtype=np.float64).reshape(9))
    if not (np.isfinite(g).all() and np.isfinite(F).all()):
        raise ValueError("the rig and period give a geometry that is not finite")
    return FtpMappingGeometry(g, box, fp, F)


def ftpMappingCloud(phaseUnwrapped, rig, period=None, stripeCentralPeak=None, theta_shift=0.0, roi=None):
    """
    Point cloud of the unwrapped phase of an object image alone: the per-pixel ``_triangulate`` that ends the reference's
    ``StereoFTP_Mapping.getCloud`` (``active.py:1436-1447`` with ``:561-605``).

    For every camera pixel centre ``(x + 0.5, y + 0.5)`` (plus the roi origin): the projector column
    ``(phase - theta_shift) / (2 pi fp) + stripeCentralPeak + 0.5``, the projector row on the pixel's epipolar line (the
    fundamental matrix), ``cv2.undistortPoints`` with ``P = K2`` (five iterations), the two rectifying homographies,
    ``baseline / |disparity|`` and the common rotation undone.  One HIP kernel, fp64 throughout (``ftp_mapping_cloud_kernel``),
    ending with the device function ``ftpCloud`` and ``GrayCode`` end with.  Not bit-identical to cv2 (another operation
    order); equal bit for bit to the numpy restatement ``tests/_ftp_mapping_ref.py``.

    Parameters
    ----------
    phaseUnwrapped : ndarray or CUDA/HIP tensor, float64 ``[H, W]``
        A tensor is made contiguous and the work goes on its device's current stream.
    rig : StereoRig
        Camera in position 1, projector in position 2 -- or an :func:`ftpMappingGeometry` result, with ``period`` and ``roi``
        left ``None``.
    period : float
        Fringe period on the projector image, in pixels.
    stripeCentralPeak : float
        Column of the central stripe's peak on the projector image.
    theta_shift : float, optional
        The phase at the central stripe (:func:`ftpStripePhase`), subtracted from the map.  Default 0.0.
    roi : (x, y, width, height), optional
        Region of the camera image the map covers; (width, height) must be the map's.  Default: the whole ``rig.res1``.

    Returns
    -------
    ndarray or tensor
        float64 ``[H, W, 3]`` in the camera's coordinate system.  A pixel with a non-finite phase holds the non-finite values
        the formulas give there.
    """
    if isinstance(rig, FtpMappingGeometry):
        if period is not None or roi is not None:
            raise ValueError("with a packed geometry in place of the rig, period and roi are the geometry's: pass None")
        G = rig
    elif isinstance(rig, FtpGeometry):
        raise ValueError("ftpMappingCloud takes the geometry of ftpMappingGeometry, not ftpGeometry's")
    else:
        G = ftpMappingGeometry(rig, period, roi)
    peak = _finite(stripeCentralPeak, "stripeCentralPeak")
    theta = _finite(theta_shift, "theta_shift")
    phase = _cloud_phase(phaseUnwrapped, G.roi)
    x0, y0, w, h = G.roi
    gp, Fp = (a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) for a in (G.geom, G.F))
    return _native.run("ssamd_ftp_mapping_cloud", (phase,), (h, w, 3), lambda src, out: (src, h, w, x0, y0, gp, Fp, theta, peak, out), _INVALID)


class StereoFTP_Mapping(StereoFTP):
    """
    Classic Fourier Transform Profilometry (the reference's ``StereoFTP_Mapping``, ``active.py:1266-1450``): no virtual
    reference plane; the phase of the object image alone is mapped to a projector column and every pixel is triangulated
    through the fundamental matrix.  Constructor and attributes are :class:`StereoFTP`'s.
    """

    def getCloud(self, imgObj, radius_factor=0.5, roi=None, unwrappingMethod=None, plot=False):
        """
        Process a camera frame and get the point cloud (``active.py:1288-1450``).

        The reference's steps in its order: ``cv2.undistort`` of the frame and the roi cut, :func:`findCentralStripe`,
        ``_triangulate`` of the stripe, ``_calculateCameraFrequency`` -> ``fc``, :func:`ftpCarrierPhase` unwrapped
        (``np.unwrap`` along x, then y, or ``unwrappingMethod`` of the wrapped map), :func:`ftpStripePhase`,
        :func:`ftpMappingCloud`.  With a device tensor the frame, the phase and the cloud stay on the device: what crosses to
        the host are the H stripe centroids and the 4 H phase values around the stripe.

        With a ``roi`` whose origin is not (0, 0) the reference's ``_triangulate`` adds the roi offset to the stripe in
        place, so its ``map_coordinates`` then samples the cut phase map at shifted coordinates; here the stripe is sampled
        where it is.

        Parameters and result as :meth:`StereoFTP.getCloud`.
        """
        if plot:
            raise NotImplementedError("plot=True needs cv2 windows and matplotlib, which this package does not use")
        cut, box, stripe, _ = self._frame(imgObj, roi)
        stripe_world = self._triangulate(stripe, self.stripeCentralPeak, box)
        fc = self._calculateCameraFrequency(stripe_world)
        if unwrappingMethod is None:
            phase = ftpCarrierPhase(cut, fc, radius_factor, unwrap="numpy")
        else:
            phase = unwrappingMethod(ftpCarrierPhase(cut, fc, radius_factor))
        theta_shift = ftpStripePhase(phase, stripe)
        G = ftpMappingGeometry(self.stereoRig, self.period, box)
        return ftpMappingCloud(phase, G, stripeCentralPeak=self.stripeCentralPeak, theta_shift=theta_shift)


class StereoFTP_PhaseOnly(StereoFTP):
    """
    The demodulation of :class:`StereoFTP` on its own (the reference's ``StereoFTP_PhaseOnly``, ``active.py:1453-2074``): the
    wrapped phase against the virtual reference plane, and the wrapped phases of the object and of the reference image.
    Constructor and attributes are :class:`StereoFTP`'s.
    """

    def getPhase(self, imgObj, radius_factor=0.5, roi=None, plot=False):
        """
        Process a camera frame and get its phase (``active.py:1950-2074``).

        The reference's steps in its order: ``cv2.undistort`` of the frame and the roi cut, :func:`findCentralStripe`, the
        stripe through ``cv2.undistortPoints(K1, distCoeffs1, P=K1)`` once more (as the reference does), ``_triangulate``,
        ``_calculateCameraFrequency`` -> ``fc``, ``z_plane`` = the smallest stripe depth, :func:`ftpReference`,
        :func:`ftpPhase` and :func:`ftpCarrierPhase` of the frame and of the reference image.  ``roi=None`` is the whole frame
        (an ``UnboundLocalError`` in the reference); a frame without stripe is ``ValueError`` (``AttributeError`` there).

        Returns
        -------
        tuple of three ndarrays or tensors, float64 ``[height, width]``, all wrapped
            ``angle(ghat * conj(g0hat))``, ``angle(ghat)``, ``angle(g0hat)``.
        """
        if plot:
            raise NotImplementedError("plot=True needs cv2 windows and matplotlib, which this package does not use")
        cut, box, stripe, _ = self._frame(imgObj, roi)
        rig = self.stereoRig
        stripe_cam = _undistort_points(stripe, rig.intrinsic1, rig.distCoeffs1, R=rig.intrinsic1)
        stripe_world = self._triangulate(stripe_cam, self.stripeCentralPeak, box)
        fc = self._calculateCameraFrequency(stripe_world)
        z_plane = np.min(stripe_world[:, 2])
        G = ftpGeometry(rig, z_plane, self.period, box)
        fringe = self._device_state(cut.device)[0] if _is_device_tensor(cut) else self.fringe
        imgRef = ftpReference(fringe, G)
        return (ftpPhase(cut, imgRef, fc, radius_factor), ftpCarrierPhase(cut, fc, radius_factor),
                ftpCarrierPhase(imgRef, fc, radius_factor))


# ------------------------------------------------------------------------------------------------ Gray code
def _integer(v):
    return isinstance(v, (numbers.Integral, np.integer)) and not isinstance(v, (bool, np.bool_))


def _gray_bits(n):
    """``ceil(log(double(n)) / log(2.0))`` as OpenCV computes it: the bits of a Gray code over ``n`` positions"""
    return int(math.ceil(math.log(float(n)) / math.log(2.0)))


def _proj_res(resolution):
    """-> (width, height, ncol, nrow) of a projector"""
    try:
        vals = tuple(resolution)
    except TypeError:
        vals = ()
    if len(vals) != 2 or not all(_integer(v) for v in vals) or not all(1 <= int(v) <= MAX_PROJECTOR for v in vals):
        raise ValueError("the projector resolution must be (width, height), two integers in 1 .. %d" % MAX_PROJECTOR)
    w, h = int(vals[0]), int(vals[1])
    return w, h, _gray_bits(w), _gray_bits(h)


def grayCodePattern(resolution):
    """
    The Gray-code pattern images of a projector: ``cv2.structured_light_GrayCodePattern.create(width, height).generate()``.

    ``ncol = ceil(log(width) / log(2))`` column bits and ``nrow`` row bits likewise (in double, as OpenCV computes them);
    ``N = 2 * ncol + 2 * nrow`` images.  The column images come first, most significant bit first: image ``2 * (ncol - 1 - k)``
    holds bit k of ``j ^ (j >> 1)`` of column j as 0 / 255 and image ``2 * (ncol - 1 - k) + 1`` its inverse; the row images
    follow from index ``2 * ncol`` in the same way for row i.  numpy on the host: O(N W H) once per rig.

    Parameters
    ----------
    resolution : (width, height)
        Of the projector, each 1 .. 65536.

    Returns
    -------
    numpy.ndarray
        uint8 ``[N, height, width]``.
    """
    w, h, ncol, nrow = _proj_res(resolution)
    out = np.empty((2 * (ncol + nrow), h, w), np.uint8)
    for first, nbits, length, along_x in ((0, ncol, w, True), (2 * ncol, nrow, h, False)):
        j = np.arange(length, dtype=np.int64)
        gray = j ^ (j >> 1)
        for k in range(nbits):
            line = (((gray >> k) & 1) * 255).astype(np.uint8)
            line = line[None, :] if along_x else line[:, None]
            out[first + 2 * (nbits - 1 - k)] = line
            out[first + 2 * (nbits - 1 - k) + 1] = 255 - line
    return out


def generateGrayCodeImgs(targetDir, resolution):
    """
    Generate the Gray-code images and save them as PNG (the reference's ``generateGrayCodeImgs``, ``active.py:23-64``).

    Writes ``0.png`` .. ``N-1.png`` (:func:`grayCodePattern`: each image is followed by its inverse, the vertical stripes come
    first) and a ``black.png`` and a ``white.png`` for threshold calibration.  Written with PIL.

    Parameters
    ----------
    targetDir : str
        Directory to write to; created if it does not exist.
    resolution : (width, height)
        Of the projector.

    Returns
    -------
    int
        Number of patterns N (black and white not counted).
    """
    imgs = grayCodePattern(resolution)
    try:
        from PIL import Image
    except ImportError:
        raise ImportError("generateGrayCodeImgs writes PNG files with PIL (the pillow package), which is not installed") from None
    if not os.path.exists(targetDir):
        os.mkdir(targetDir)
    for i in range(imgs.shape[0]):
        Image.fromarray(imgs[i]).save(os.path.join(targetDir, str(i) + ".png"))
    h, w = (int(resolution[1]), int(resolution[0]))
    Image.fromarray(np.zeros((h, w), np.uint8)).save(os.path.join(targetDir, "black.png"))
    Image.fromarray(np.full((h, w), 255, np.uint8)).save(os.path.join(targetDir, "white.png"))
    return int(imgs.shape[0])


def _gray_stack(images, size=None):
    """-> (contiguous uint8 stack [M, Hc, Wc], is it on a device).  A sequence of [Hc, Wc] host arrays is stacked on the host;
    with ``size = (width, height)`` every plane must be of that size (the reference's check and message, ``active.py:1205-1206``)."""
    dev = _is_device_tensor(images)
    if dev or isinstance(images, np.ndarray):
        if dev:
            import torch
            if images.dtype != torch.uint8:
                raise TypeError("images must be a uint8 tensor")
        elif images.dtype != np.uint8:
            raise TypeError("images must be a uint8 array")
        if images.ndim != 3:
            raise ValueError("images must be [M, Hc, Wc]: one gray image per pattern")
        if size is not None and (int(images.shape[2]), int(images.shape[1])) != size:
            raise ValueError("Image size of 0 is mismatch!")
        return (images.contiguous() if dev else np.ascontiguousarray(images)), dev
    if isinstance(images, (str, bytes)) or not isinstance(images, (list, tuple)):
        raise TypeError("images must be a uint8 ndarray or CUDA/HIP tensor [M, Hc, Wc], or a sequence of [Hc, Wc] uint8 arrays")
    planes = []
    for i, img in enumerate(images):
        if not isinstance(img, np.ndarray) or img.dtype != np.uint8:
            raise TypeError("images[%d] must be a uint8 ndarray" % i)
        if img.ndim != 2:
            raise ValueError("images[%d] must be [Hc, Wc]: a gray image" % i)
        if (size is not None and (img.shape[1], img.shape[0]) != size) or (planes and img.shape != planes[0].shape):
            raise ValueError("Image size of %d is mismatch!" % i)
        planes.append(img)
    if not planes:
        return np.empty((0,) + ((size[1], size[0]) if size is not None else (0, 0)), np.uint8), False
    return np.ascontiguousarray(np.stack(planes)), False


def _gray_roi(roi, res):
    """-> (x, y, w, h) of the reference's loops ``range(roi_y, roi_h)`` / ``range(roi_x, roi_w)`` (``active.py:1221-1222``): the
    third and fourth entry are exclusive END coordinates; empty (w or h 0) when an end does not lie beyond its origin"""
    W, H = int(res[0]), int(res[1])
    if roi is None:
        return 0, 0, W, H
    try:
        vals = tuple(roi)
    except TypeError:
        vals = ()
    if len(vals) != 4 or not all(_integer(v) for v in vals):
        raise ValueError("roi must be four integers (x, y, x_end, y_end)")
    x, y, xe, ye = (int(v) for v in vals)
    if x < 0 or y < 0:
        raise ValueError("roi %s starts outside the image" % ((x, y, xe, ye),))
    w, h = max(xe - x, 0), max(ye - y, 0)
    if w and h and (xe > W or ye > H):
        raise ValueError("roi %s reaches outside the image (%d x %d)" % ((x, y, xe, ye), W, H))
    return x, y, w, h


def _white_thr(v):
    if not _integer(v) or not 0 <= int(v) <= 256:
        raise ValueError("white_thr must be an integer in 0 .. 256")
    return int(v)


def _gray_maps(maps, stack, dev):
    """-> (mapx, mapy) like the stack (host arrays, or tensors on its device), or (None, None)"""
    if maps is None:
        return None, None
    try:
        mx, my = maps
    except (TypeError, ValueError):
        raise ValueError("maps must be (mapx, mapy)") from None
    out = []
    for m, name in ((mx, "mapx"), (my, "mapy")):
        on_dev = _is_device_tensor(m)
        if not (on_dev or isinstance(m, np.ndarray)):
            raise TypeError("%s must be a float32 ndarray or CUDA/HIP tensor" % name)
        if on_dev:
            import torch
            if m.dtype != torch.float32:
                raise TypeError("%s must be float32" % name)
            if not dev or m.device != stack.device:
                raise TypeError("%s is on a device the images are not on" % name)
            m = m.contiguous()
        else:
            if m.dtype != np.float32:
                raise TypeError("%s must be float32" % name)
            m = np.ascontiguousarray(m)
        if tuple(m.shape) != tuple(stack.shape[1:]):
            raise ValueError("%s must be [Hc, Wc] like the images, %s" % (name, tuple(stack.shape[1:])))
        if dev and not on_dev:
            import torch
            m = torch.from_numpy(m).to(stack.device)
        out.append(m)
    return out[0], out[1]


def _ptr(a):
    return None if a is None else (a.data_ptr() if _is_device_tensor(a) else a.ctypes.data)


def _gray_blocks(h, w):
    return (h * w + _native.GRAYCODE_BLOCK - 1) // _native.GRAYCODE_BLOCK


def _stack_args(stack, n, mx, my, box):
    """The ten arguments every decoder of a plane stack begins with: the first ``n`` planes, the maps (or None) and the region"""
    x0, y0, w, h = box
    if h * w >= 1 << 31 or int(stack.shape[1]) * int(stack.shape[2]) >= 1 << 31:
        raise ValueError("images or regions of 2^31 pixels or more are not supported")
    return (_ptr(stack), n, int(stack.shape[1]), int(stack.shape[2]), _ptr(mx), _ptr(my), x0, y0, h, w)


def _gray_decode_args(stack, proj, thr, mx, my, box):
    pw, ph, ncol, nrow = proj
    n = 2 * (ncol + nrow)
    if int(stack.shape[0]) < n:
        raise ValueError("a %d x %d projector needs %d pattern images, got %d" % (pw, ph, n, int(stack.shape[0])))
    return _stack_args(stack, n, mx, my, box) + (ncol, nrow, pw, ph, thr)


def _gray_decode_device(stack, args, h, w):
    """-> (decoded int32 [h, w, 2], valid pixels per block int32 [nblocks]) on the stack's device and current stream"""
    import torch
    out = torch.empty((h, w, 2), dtype=torch.int32, device=stack.device)
    counts = torch.empty((_gray_blocks(h, w),), dtype=torch.int32, device=stack.device)
    if h * w:
        _native.call_on_stream(stack, _native.lib().ssamd_graycode_decode_device, *args, out.data_ptr(), counts.data_ptr(), invalid=_INVALID)
    return out, counts


def grayCodeDecode(images, projRes, white_thr=5, maps=None, roi=None):
    """
    Decode a stack of Gray-code images: ``cv2.structured_light_GrayCodePattern.getProjPixel`` for every pixel of the region,
    by one HIP kernel (``graycode_decode_kernel``).

    Per bit, with ``v1`` the pattern image and ``v2`` its inverse at the pixel: an error if ``|v1 - v2| < white_thr``; the Gray
    bit is 1 if ``v1 > v2``, else 0 (so ``v1 == v2`` gives 0); Gray -> binary is the MSB-first prefix XOR; after both codes, an
    error if ``xDec >= width or yDec >= height``.  ``black_thr`` plays no part in ``getProjPixel``.  A 1 x 1 projector has no
    pattern images; every pixel then decodes to (0, 0) without error.  The piece to build a ``GrayCodeDouble`` of one's own from.

    Parameters
    ----------
    images : ndarray or CUDA/HIP tensor uint8 ``[M, Hc, Wc]``, or a sequence of ``[Hc, Wc]`` uint8 arrays (stacked on the host)
        In the order of :func:`grayCodePattern`.  ``M >= N``; only the first N are read (the reference ignores extra images).
    projRes : (width, height)
        Of the projector, each 1 .. 65536.
    white_thr : int, optional
        0 .. 256.  Default 5.
    maps : (mapx, mapy), optional
        float32 ``[Hc, Wc]``: every image is sampled as ``cv2.remap(img, mapx, mapy, INTER_LINEAR)`` samples it (1/32-pixel
        fractions, ``(S + 512) >> 10``, border 0, non-finite coordinates 0) without the remapped images ever existing; the
        result equals remapping every image with that arithmetic and decoding, value for value.  Default: the images as they are.
    roi : (x, y, x_end, y_end), optional
        The region ``[y, y_end) x [x, x_end)``, as :meth:`GrayCode.getCloud` reads it.  Default: the whole image.

    Returns
    -------
    ndarray or tensor
        int32 ``[h, w, 2]``: ``(xDec, yDec)``, or ``(-1, -1)`` where ``getProjPixel`` reports an error.  A tensor on the images'
        device, computed on its current stream, for a tensor.
    """
    proj = _proj_res(projRes)
    thr = _white_thr(white_thr)
    stack, dev = _gray_stack(images)
    mx, my = _gray_maps(maps, stack, dev)
    box = _gray_roi(roi, (int(stack.shape[2]), int(stack.shape[1])))
    args = _gray_decode_args(stack, proj, thr, mx, my, box)
    h, w = box[3], box[2]
    if dev:
        return _gray_decode_device(stack, args, h, w)[0]
    out = np.empty((h, w, 2), np.int32)
    if h * w:
        _native.check(_native.lib().ssamd_graycode_decode(*args, out.ctypes.data, None, -1), _INVALID)
    return out


def _gray_load(paths, count, size):
    """The first ``count`` files as uint8 planes of ``size`` (the rules of :meth:`GrayCode._load`)"""
    try:
        from PIL import Image
    except ImportError:
        raise ImportError("reading image files needs PIL (the pillow package), which is not installed: pass arrays") from None
    planes = []
    for fname in paths[:count]:
        with Image.open(fname) as im:
            if im.mode != "L":
                raise ValueError("%s is not an 8-bit single-channel image (mode %r): convert it yourself and pass arrays"
                                 % (fname, im.mode))
            img = np.array(im, dtype=np.uint8)
        if (img.shape[1], img.shape[0]) != size:
            raise ValueError("Image size of %s is mismatch!" % (fname,))
        planes.append(img)
    return planes


class GrayCode:
    """
    Gray-code structured light with a calibrated camera-projector rig (the reference's ``GrayCode``, ``active.py:1130-1263``),
    with no cv2 call: decode, compaction and triangulation are three HIP kernels.

    Parameters
    ----------
    rig : StereoRig
        Camera in position 1 (world origin), projector in position 2.  ``rig.distCoeffs2 = None`` ignores the projector's
        distortion.
    black_thr : int, optional
        Stored; ``getProjPixel`` does not read it (it belongs to ``computeShadowMasks``).  Default 40.
    white_thr : int, optional
        Minimum difference between a pattern image and its inverse for a valid pixel, 0 .. 256.  Default 5.

    The attributes are the reference's: ``rig``, ``num_patterns``, ``Rectify1``, ``Rectify2``, ``R_inv`` (4 x 4).  There is no
    ``graycode`` attribute: no cv2 object exists.  The undistortion maps of the camera go to a device once per instance.
    """

    def __init__(self, rig, black_thr=40, white_thr=5):
        self.rig = rig
        self.black_thr = black_thr
        self.white_thr = _white_thr(white_thr)
        self._proj = _proj_res(rig.res2)
        self.num_patterns = 2 * (self._proj[2] + self._proj[3])
        self.Rectify1, self.Rectify2, commonR = _low_level_rectify(rig)
        self.R_inv = _r_inv4(commonR)
        self._cache = {}                 # _cached_maps' entries

    def _maps(self, device=None):
        return _cached_maps(self._cache, self.rig, device)

    def _geometry(self):
        """The ``SSAMD_FTP_CLOUD_NGEOM`` doubles of ``ssamd_graycode_cloud``: only what the triangulation reads -- K2,
        ``distCoeffs2``, the rectifying transforms, the inverse common orientation, the baseline.  Neither the epipole nor a
        phase period is in it, so ``T[2] == 0`` is fine."""
        return _triangulation_geometry(self.rig, self.Rectify1, self.Rectify2, self.R_inv[:3, :3])

    def _load(self, paths, size):
        """The first ``num_patterns`` files as uint8 planes.  cv2's colour -> gray conversion is not restated: only 8-bit
        single-channel files are read."""
        return _gray_load(paths, self.num_patterns, size)

    def getCloud(self, images, roi=None, dense=False):
        """
        The 3-D points of a set of Gray-code images (``active.py:1174-1263``).

        The reference's steps: ``cv2.undistort`` of every image (here fused into the decode: the maps of
        ``initUndistortRectifyMap(K1, D1, I, K1, res1)``, :func:`grayCodeDecode`), ``getProjPixel`` for every pixel of the roi,
        and for the valid ones, from ``pc = (x + 0.5, y + 0.5)`` and ``pp = (xDec + 0.5, yDec + 0.5)``:
        ``cv2.undistortPoints(pp, K2, distCoeffs2, P=K2)``, the two rectifying homographies, ``baseline / |disparity|`` and the
        common rotation undone -- the operations that end :func:`ftpCloud`, by the same device function, fp64.

        Parameters
        ----------
        images : what :func:`grayCodeDecode` takes, or a sequence of paths
            Of the rig's ``res1``, in the order of the patterns; any following extra image is ignored (e.g. full white).
            Paths are opened with PIL and must be 8-bit single-channel files.
        roi : (x, y, x_end, y_end), optional
            As the reference's loops read it, ``range(roi_y, roi_h)`` and ``range(roi_x, roi_w)``: the third and fourth entry are
            exclusive end coordinates, not a width and a height.  Default None: the whole image.
        dense : bool, optional
            ``True`` (the reference's todo): the cloud in the shape of the roi with NaN at the invalid pixels; with a tensor
            nothing is read back and the whole chain is asynchronous on the current stream.  Default False.

        Returns
        -------
        ndarray or tensor
            float64 ``(n, 1, 3)``, the points of the valid pixels in raster order -- or ``[h, w, 3]`` with ``dense``.  An
            ndarray for host images, a tensor on the images' device for a tensor.
        """
        size = (int(self.rig.res1[0]), int(self.rig.res1[1]))
        if isinstance(images, (list, tuple)) and len(images) and all(isinstance(p, (str, os.PathLike)) for p in images):
            images = self._load(images, size)
        stack, dev = _gray_stack(images, size)
        box = _gray_roi(roi, size)
        geom = self._geometry()
        mx, my = self._maps(stack.device if dev else None)
        args = _gray_decode_args(stack, self._proj, self.white_thr, mx, my, box)
        x0, y0, w, h = box
        lib = _native.lib()
        if not dev:
            buf = np.empty((h * w, 3), np.float64)
            n = ctypes.c_int(0)
            if h * w:
                _native.check(lib.ssamd_graycode_cloud(*args, geom.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1 if dense else 0,
                                                       buf.ctypes.data, ctypes.byref(n), -1), _INVALID)
            if dense:
                return buf.reshape(h, w, 3)
            pts = buf[:n.value]
            return (pts if n.value == h * w else pts.copy()).reshape(-1, 1, 3)
        import torch
        decoded, counts = _gray_decode_device(stack, args, h, w)
        gp = geom.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        if dense:
            out = torch.empty((h, w, 3), dtype=torch.float64, device=stack.device)
            if h * w:
                _native.call_on_stream(stack, lib.ssamd_graycode_cloud_device, decoded.data_ptr(), h, w, x0, y0, gp, None, out.data_ptr(),
                                       invalid=_INVALID)
            return out
        if not h * w:
            return torch.empty((0, 1, 3), dtype=torch.float64, device=stack.device)
        offsets = torch.empty((counts.shape[0] + 1,), dtype=torch.int32, device=stack.device)
        _native.call_on_stream(stack, lib.ssamd_graycode_offsets_device, counts.data_ptr(), int(counts.shape[0]), offsets.data_ptr(),
                               invalid=_INVALID)
        n = int(offsets[-1].item())                                # the one read-back: the number of points sizes the result
        out = torch.empty((n, 1, 3), dtype=torch.float64, device=stack.device)
        if n:
            _native.call_on_stream(stack, lib.ssamd_graycode_cloud_device, decoded.data_ptr(), h, w, x0, y0, gp, offsets.data_ptr(),
                                   out.data_ptr(), invalid=_INVALID)
        return out


GrayCodeSingle = GrayCode


# ------------------------------------------------------------------------------------------------ Gray code, two cameras
_REDUCE = {"last": _native.STEREO_LAST, "mean": _native.STEREO_MEAN}


def _reduce_mode(reduce):
    if not isinstance(reduce, str) or reduce not in _REDUCE:
        raise ValueError('reduce must be "last" or "mean"')
    return _REDUCE[reduce]


def _stereo_proj(projRes):
    """-> (width, height, ncol, nrow) of a projector whose table the two-camera match can index: fewer than 2^31 pixels"""
    proj = _proj_res(projRes)
    if proj[0] * proj[1] >= 1 << 31:
        raise ValueError("a projector of %d x %d pixels is not supported: 2^31 or more" % (proj[0], proj[1]))
    return proj


def _origin(origin, name):
    try:
        vals = tuple(origin)
    except TypeError:
        vals = ()
    if len(vals) != 2 or not all(_integer(v) for v in vals) or min(int(v) for v in vals) < 0:
        raise ValueError("%s must be (x, y), two integers that are not negative" % name)
    return int(vals[0]), int(vals[1])


def _decoded_map(d, name):
    """-> (contiguous, 16-byte aligned int32 [h, w, 2] where it is, is it on a device)"""
    dev = _is_device_tensor(d)
    if not (dev or isinstance(d, np.ndarray)):
        raise TypeError("%s must be an int32 ndarray or CUDA/HIP tensor" % name)
    if dev:
        import torch
        if d.dtype != torch.int32:
            raise TypeError("%s must be int32" % name)
    elif d.dtype != np.int32:
        raise TypeError("%s must be int32" % name)
    if d.ndim != 3 or int(d.shape[2]) != 2:
        raise ValueError("%s must be [h, w, 2]: the result of grayCodeDecode" % name)
    if dev:
        d = d.contiguous()
        return (d.clone() if d.data_ptr() & 15 else d), True
    return np.ascontiguousarray(d), False


def _match_box(d, origin):
    """(x0, y0, w, h) of a decoded map at ``origin``, checked against the limits of the match"""
    h, w = int(d.shape[0]), int(d.shape[1])
    if h * w >= 1 << 31 or (origin[1] + h) * (origin[0] + w) >= 1 << 31:
        raise ValueError("decoded maps of 2^31 pixels or more, or reaching that far from the image origin, are not supported")
    return origin[0], origin[1], w, h


def _match_args(d1, box1, d2, box2, proj, mode):
    return (_ptr(d1), box1[3], box1[2], box1[0], box1[1], _ptr(d2), box2[3], box2[2], box2[0], box2[1], proj[0], proj[1], mode)


def _gray_match(d1, box1, d2, box2, proj, mode, dev):
    """-> (matches float64 [Hp, Wp, 4], matched cells per block int32 [nblocks]) where the decoded maps are"""
    pw, ph = proj[0], proj[1]
    args = _match_args(d1, box1, d2, box2, proj, mode)
    nblocks = _gray_blocks(ph, pw)
    if not dev:
        matches, counts = np.empty((ph, pw, 4), np.float64), np.empty((nblocks,), np.int32)
        _native.check(_native.lib().ssamd_graycode_stereo_match(*args, matches.ctypes.data, counts.ctypes.data, -1), _INVALID)
        return matches, counts
    import torch
    matches = torch.empty((ph, pw, 4), dtype=torch.float64, device=d1.device)
    counts = torch.empty((nblocks,), dtype=torch.int32, device=d1.device)
    per_cell = 20 if mode == _native.STEREO_MEAN else 4
    scratch = torch.empty((2 * ((per_cell * ph * pw + 7) // 8),), dtype=torch.int64, device=d1.device)    # SSAMD_GRAYCODE_STEREO_SCRATCH
    lib = _native.lib()
    with torch.cuda.device(d1.device):
        rc = lib.ssamd_graycode_stereo_match_device(*args, matches.data_ptr(), counts.data_ptr(), scratch.data_ptr(),
                                                    ctypes.c_void_p(torch.cuda.current_stream(d1.device).cuda_stream))
        if rc:
            _native.check(rc, _INVALID)
    return matches, counts


def grayCodeMatch(decoded1, decoded2, projRes, reduce="last", origin1=(0, 0), origin2=(0, 0)):
    """
    Two cameras' decoded Gray-code maps -> camera-camera correspondences, one per projector pixel: the inversion of both
    camera -> projector maps, by HIP kernels (``graycode_scatter_kernel`` once per camera, ``graycode_match_kernel``).

    Of the pixels of one camera that decode to one projector pixel, ``reduce="last"`` keeps the one that comes last in raster
    order (the reference's loops, where a later pixel overwrites an earlier one) and ``reduce="mean"`` their centroid (exact
    integer sums, one division): sub-pixel where the cameras out-resolve the projector.  Integer atomics only: the same bytes on
    every run.

    Parameters
    ----------
    decoded1, decoded2 : ndarray or CUDA/HIP tensor int32 ``[h, w, 2]``
        What :func:`grayCodeDecode` returns for camera 1 and camera 2 (sizes may differ); both on the host or both on one
        device.  ``(-1, -1)``, or a value outside the projector, contributes nothing.
    projRes : (width, height)
        Of the projector, each 1 .. 65536, fewer than 2^31 pixels together.
    reduce : "last" or "mean", optional
    origin1, origin2 : (x, y), optional
        Where each map's first pixel lies in its camera image (the ``roi`` origin it was decoded with): the coordinates of
        the result are absolute image coordinates.  Default (0, 0).

    Returns
    -------
    ndarray or tensor
        float64 ``[Hp, Wp, 4]``: ``(x1 + 0.5, y1 + 0.5, x2 + 0.5, y2 + 0.5)``, pixel centres, where both cameras see the projector
        pixel, four NaN elsewhere.  Where the inputs are.
    """
    proj = _stereo_proj(projRes)
    mode = _reduce_mode(reduce)
    d1, dev1 = _decoded_map(decoded1, "decoded1")
    d2, dev2 = _decoded_map(decoded2, "decoded2")
    if dev1 != dev2 or (dev1 and d1.device != d2.device):
        raise TypeError("decoded1 and decoded2 must both be on the host or both on one device")
    box1, box2 = _match_box(d1, _origin(origin1, "origin1")), _match_box(d2, _origin(origin2, "origin2"))
    return _gray_match(d1, box1, d2, box2, proj, mode, dev1)[0]


def _stereo_geometry(rect1, rect2, common_inv, baseline):
    """The ``SSAMD_FTP_CLOUD_NGEOM`` doubles of the two-camera triangulation: only ``[40:68]`` (the rectifying transforms, the
    inverse common orientation, the baseline) are read; no intrinsics, no distortion -- both images were undistorted."""
    g = np.zeros(NGEOM)
    g[40:49] = np.asarray(rect1, dtype=np.float64).ravel()
    g[49:58] = np.asarray(rect2, dtype=np.float64).ravel()
    g[58:67] = np.asarray(common_inv, dtype=np.float64).ravel()
    g[67] = baseline
    if not np.isfinite(g).all():
        raise ValueError("the rig gives a geometry that is not finite")
    return g


def _triangulate_pairs(geom, points1, points2):
    pts = StructuredLightRig._points
    p1, p2 = pts(points1, "points1"), pts(points2, "points2")
    if _is_device_tensor(p1) != _is_device_tensor(p2) or (_is_device_tensor(p1) and p1.device != p2.device):
        raise TypeError("points1 and points2 must both be on the host or both on one device")
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("%d points of image 1 but %d of image 2" % (p1.shape[0], p2.shape[0]))
    n = int(p1.shape[0])
    gp = geom.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    return _native.run("ssamd_stereo_triangulate", (p1, p2), (n, 1, 3), lambda a, b, out: (a, b, n, gp, out), _INVALID)


def stereoTriangulate(rig, points1, points2):
    """
    Triangulate camera-camera correspondences of a calibrated two-camera rig, by one HIP kernel
    (``graycode_stereo_cloud_kernel`` on point pairs): the two-camera counterpart of ``StructuredLightRig.triangulate`` and the
    last step of :meth:`GrayCodeStereo.getCloud` (reference ``active.py:1594-1606``), by the same device function
    (``rectified_triangulate``), fp64: ``Rectify1`` on ``points1``, ``Rectify2`` on ``points2`` (only x is used),
    ``getBaseline() * (p1 / |disparity|)`` and the common rotation undone.  No ``undistortPoints``: the points of BOTH images
    must already be undistorted.  A disparity of exactly 0 gives inf / NaN coordinates, as the reference's arithmetic does.

    Parameters
    ----------
    rig : StereoRig
        Two calibrated cameras; anything else is ``ValueError("Invalid argument!")``.
    points1, points2 : numpy.ndarray or CUDA/HIP tensor
        Ordered corresponding (x, y) couples, of any real dtype; the last dimension must be 2.  Both on the host or both on
        one device.  They are converted to float64.

    Returns
    -------
    numpy.ndarray or tensor
        float64 ``(n, 1, 3)``; three NaN where a couple holds a NaN.  Where the inputs are.
    """
    if isinstance(rig, StructuredLightRig):              # its R already is the common orientation
        geom = _stereo_geometry(rig.R1, rig.R2, rig.R_inv[:3, :3], rig.getBaseline())
    elif isinstance(rig, StereoRig):
        rect1, rect2, common = _low_level_rectify(rig)
        geom = _stereo_geometry(rect1, rect2, np.linalg.inv(common), rig.getBaseline())
    else:
        raise ValueError("Invalid argument!")
    return _triangulate_pairs(geom, points1, points2)


class GrayCodeStereo:
    """
    Gray-code active stereo with two calibrated cameras and one uncalibrated projector: what the reference's ``GrayCodeDouble``
    (``active.py:1463-1608``) sets out to do, with no cv2 call.  It is not a drop-in for that class, which cannot run as published;
    the semantics are those of its loops, repaired: both stacks are decoded (:func:`grayCodeDecode`, ``cv2.undistort`` of each
    camera fused in), both camera -> projector maps are inverted into one projector-shaped table (:func:`grayCodeMatch`), and the
    projector pixels both cameras see are triangulated camera against camera (:func:`stereoTriangulate`).  The projector is
    only a source of codes: its calibration plays no part.

    Parameters
    ----------
    rig : StereoRig
        Two calibrated cameras.
    projRes : (width, height)
        Of the projector, each 1 .. 65536, fewer than 2^31 pixels together.
    black_thr : int, optional
        Stored; ``getProjPixel`` does not read it.  Default 40.
    white_thr : int, optional
        Minimum difference between a pattern image and its inverse for a valid pixel, 0 .. 256.  Default 5.
    reduce : "last" or "mean", optional
        Which camera pixel stands for a projector pixel that several decode to (:func:`grayCodeMatch`).  ``"last"``, the
        default, is the reference's loop; ``"mean"`` is sub-pixel when the cameras out-resolve the projector.

    The attributes are the reference's: ``rig``, ``projRes``, ``num_patterns``, ``Rectify1``, ``Rectify2`` -- and ``R_inv``
    (4 x 4), which the reference reads but never assigns.  There is no ``graycode`` attribute.
    """

    def __init__(self, rig, projRes, black_thr=40, white_thr=5, reduce="last"):
        if not isinstance(rig, StereoRig):
            raise ValueError("Invalid argument!")
        self.rig = rig
        self._proj = _stereo_proj(projRes)
        self.projRes = (self._proj[0], self._proj[1])
        self.black_thr = black_thr
        self.white_thr = _white_thr(white_thr)
        self.reduce = reduce
        self._mode = _reduce_mode(reduce)
        self.num_patterns = 2 * (self._proj[2] + self._proj[3])
        self.Rectify1, self.Rectify2, commonR = _low_level_rectify(rig)
        self.R_inv = _r_inv4(commonR)
        self._cache = {}                 # _cached_maps' entries, both cameras'

    def _geometry(self):
        return _stereo_geometry(self.Rectify1, self.Rectify2, self.R_inv[:3, :3], self.rig.getBaseline())

    def _stacks(self, images):
        """-> ((stack1, stack2), on a device) of ``(stack1, stack2)`` or of the reference's list of (pathL, pathR) couples"""
        sizes = [(int(r[0]), int(r[1])) for r in (self.rig.res1, self.rig.res2)]
        if not isinstance(images, (list, tuple)) or not len(images):
            raise TypeError("images must be (stack1, stack2) or a sequence of (path1, path2) couples")
        if all(isinstance(p, (list, tuple)) and len(p) == 2 and all(isinstance(q, (str, os.PathLike)) for q in p) for p in images):
            images = [_gray_load([p[i] for p in images], self.num_patterns, sizes[i]) for i in range(2)]
        elif len(images) != 2:
            raise TypeError("images must be (stack1, stack2) or a sequence of (path1, path2) couples")
        (s1, dev1), (s2, dev2) = (_gray_stack(images[i], sizes[i]) for i in range(2))
        if dev1 != dev2 or (dev1 and s1.device != s2.device):
            raise TypeError("the two stacks must both be on the host or both on one device")
        return (s1, s2), dev1

    def getCloud(self, images, roi1=None, roi2=None, dense=False):
        """
        The 3-D points of two cameras' sets of Gray-code images (what ``active.py:1508-1608`` sets out to compute).

        Each stack is decoded over its roi through the maps of ``cv2.undistort(img, K_i, distCoeffs_i)``; each camera fills a
        projector-shaped table (``reduce``); a projector pixel both cameras see gives the couple of pixel centres
        ``(x1 + 0.5, y1 + 0.5)``, ``(x2 + 0.5, y2 + 0.5)`` in absolute image coordinates; the couples are triangulated in
        projector raster order (:func:`stereoTriangulate`).  A couple whose rectified x coordinates coincide (zero disparity)
        gives inf / NaN coordinates, as the reference's arithmetic does; nothing is raised.

        Parameters
        ----------
        images : (stack1, stack2), or a sequence of (path1, path2) couples
            Each stack as :func:`grayCodeDecode` takes it, of the rig's ``res1`` / ``res2``, both on the host or both on one
            device; or the reference's list of couples of image paths (8-bit single-channel files, read with PIL), in the
            order of the patterns.  Any following extra image is ignored.
        roi1, roi2 : (x, y, x_end, y_end), optional
            Per camera, read as :meth:`GrayCode.getCloud` reads its roi.  Default None: the whole image.
        dense : bool, optional
            ``True``: the cloud in the shape of the projector, NaN where a projector pixel is not seen by both cameras; with
            tensors nothing is read back.  Default False: with tensors one integer, the number of points, is read back.

        Returns
        -------
        ndarray or tensor
            float64 ``(n, 1, 3)``, the points in projector raster order -- or ``[Hp, Wp, 3]`` with ``dense``.  Where the images are.
        """
        (s1, s2), dev = self._stacks(images)
        stacks = (s1, s2)
        boxes = [_gray_roi(roi, (int(r[0]), int(r[1]))) for roi, r in ((roi1, self.rig.res1), (roi2, self.rig.res2))]
        geom = self._geometry()
        pw, ph = self.projRes
        maps = [_cached_maps(self._cache, self.rig, stacks[i].device if dev else None, which=i + 1) for i in range(2)]
        args = [_gray_decode_args(stacks[i], self._proj, self.white_thr, maps[i][0], maps[i][1], boxes[i]) for i in range(2)]
        if not all(b[2] * b[3] for b in boxes):                    # a camera without pixels: no projector pixel is seen by both
            if dev:
                import torch
                return (torch.full((ph, pw, 3), float("nan"), dtype=torch.float64, device=s1.device) if dense
                        else torch.empty((0, 1, 3), dtype=torch.float64, device=s1.device))
            return np.full((ph, pw, 3), np.nan) if dense else np.empty((0, 1, 3), np.float64)
        lib = _native.lib()
        gp = geom.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        if not dev:
            buf = np.empty((ph * pw, 3), np.float64)
            n = ctypes.c_int(0)
            side = [a[0:1] + a[2:10] for a in args]                # planes, hc, wc, mapx, mapy, x0, y0, h, w
            _native.check(lib.ssamd_graycode_stereo_points(*side[0], *side[1], *args[0][1:2], *args[0][10:], self._mode, gp,
                                                           1 if dense else 0, buf.ctypes.data, ctypes.byref(n), -1), _INVALID)
            if dense:
                return buf.reshape(ph, pw, 3)
            return buf[:n.value].copy().reshape(-1, 1, 3)
        import torch
        decoded = [_gray_decode_device(stacks[i], args[i], boxes[i][3], boxes[i][2])[0] for i in range(2)]
        matches, counts = _gray_match(decoded[0], boxes[0], decoded[1], boxes[1], self._proj, self._mode, True)
        if dense:
            out = torch.empty((ph, pw, 3), dtype=torch.float64, device=s1.device)
            _native.call_on_stream(s1, lib.ssamd_graycode_stereo_cloud_device, matches.data_ptr(), pw, ph, gp, None, out.data_ptr(), invalid=_INVALID)
            return out
        offsets = torch.empty((counts.shape[0] + 1,), dtype=torch.int32, device=s1.device)
        _native.call_on_stream(s1, lib.ssamd_graycode_offsets_device, counts.data_ptr(), int(counts.shape[0]), offsets.data_ptr(), invalid=_INVALID)
        n = int(offsets[-1].item())                                # the one read-back: the number of points sizes the result
        out = torch.empty((n, 1, 3), dtype=torch.float64, device=s1.device)
        if n:
            _native.call_on_stream(s1, lib.ssamd_graycode_stereo_cloud_device, matches.data_ptr(), pw, ph, gp, offsets.data_ptr(), out.data_ptr(),
                                   invalid=_INVALID)
        return out


# ------------------------------------------------------------------------------------------------ phase shifting
MAX_PERIODS = 8           # SSAMD_SL_MAX_PERIODS: periods per projector axis
_MOD_THR2_ALL = 2 * 255 * 255 + 1      # above every a^2 + b^2 of 8-bit images: masks all


def _periods(periods):
    """-> (float64 [nx], float64 [ny]) of ``periods = (list_x, list_y)``"""
    try:
        lists = tuple(periods)
    except TypeError:
        lists = ()
    if len(lists) != 2:
        raise ValueError("periods must be (list_x, list_y)")
    out = []
    for axis, name in zip(lists, "xy"):
        try:
            vals = [_finite(v, "a period") for v in axis]
        except TypeError:
            raise ValueError("periods must be (list_x, list_y)") from None
        if not 1 <= len(vals) <= MAX_PERIODS:
            raise ValueError("%d %s-periods: must be 1 .. %d" % (len(vals), name, MAX_PERIODS))
        if min(vals) <= 0:
            raise ValueError("periods must be positive")
        out.append(np.array(vals, dtype=np.float64))
    return out[0], out[1]


def _mod_thr2(min_modulation):
    """The threshold of the mask: a set masks its pixel iff ``a^2 + b^2 < 4 m^2`` in exact arithmetic on the double ``m``, which on
    integers ``a``, ``b`` is ``a^2 + b^2 < min(ceil(4 m^2), 130051)``; ``inf`` -> 130051 (masks all), ``None`` -> 0 (masks none).
    Integers throughout: ``m = p / q`` exactly (``float.as_integer_ratio``), so nothing is rounded -- ``ceil(4.0 * m * m)`` in
    double is one off at about 6 % of the ``m`` next to a ``sqrt(s) / 2`` and 0 for every ``0 < m < 1e-162``."""
    if min_modulation is None:
        return 0
    m = _number(min_modulation, "min_modulation")
    if not m >= 0:
        raise ValueError("min_modulation must be a number >= 0 or None")
    if m >= 181.0:                          # 4 * 181^2 > 130051 (and inf has no ratio)
        return _MOD_THR2_ALL
    p, q = m.as_integer_ratio()
    return min(-((-4 * p * p) // (q * q)), _MOD_THR2_ALL)


def phaseShiftPattern(periods, projRes):
    """
    The four-step phase-shift images of a projector, in the order :func:`phaseShiftDecode` reads them (the image-set order of
    the reference's ``calibration.phaseShift``): for each x-period ``T`` the four gray fringes
    ``buildFringe(T, shift=i * T / 4, dims=projRes)``, ``i = 0 .. 3`` -- ``cos(theta + i pi / 2)`` --, then for each y-period
    the same with ``vertical=True``.

    Parameters
    ----------
    periods : (list_x, list_y)
        Fringe periods in projector pixels along x and along y, each 1 .. 8 finite positive numbers, the longest first.
    projRes : (width, height)
        Of the projector, each 1 .. 65536.

    Returns
    -------
    numpy.ndarray
        uint8 ``[4 * (nx + ny), height, width]``.
    """
    tx, ty = _periods(periods)
    w, h = _proj_res(projRes)[:2]
    out = np.empty((4 * (len(tx) + len(ty)), h, w), np.uint8)
    at = 0
    for axis, vertical in ((tx, False), (ty, True)):
        for T in axis:
            for i in range(4):
                out[at] = buildFringe(float(T), shift=i * float(T) / 4, dims=(w, h), vertical=vertical)
                at += 1
    return out


def _phase_decode_args(stack, tx, ty, proj, thr2, mx, my, box):
    n = 4 * (len(tx) + len(ty))
    if int(stack.shape[0]) < n:
        raise ValueError("%d x-periods and %d y-periods need %d images, got %d" % (len(tx), len(ty), n, int(stack.shape[0])))
    dp = ctypes.POINTER(ctypes.c_double)
    return _stack_args(stack, n, mx, my, box) + (len(tx), len(ty), tx.ctypes.data_as(dp), ty.ctypes.data_as(dp), proj[0], proj[1], thr2)


def _phase_decode(stack, args, h, w):
    """-> float64 [h, w, 2] where the stack is; on its device's current stream for a tensor.  ``args`` already hold the stack's
    pointer (and the maps', which are of its kind)."""
    return _native.run("ssamd_phaseshift_decode", (stack,), (h, w, 2), lambda _, out: args + (out,), _INVALID)


def phaseShiftDecode(images, periods, projRes, maps=None, roi=None, min_modulation=None):
    """
    Decode a stack of four-step phase-shift images into a dense camera-to-projector map: the three closures of the
    reference's ``calibration.phaseShift`` (``getPhase``, ``unwrap``, ``getProjCoord``, ``calibration.py:656-687`` and
    ``:726-738``), which the reference samples at chessboard corners only, for every pixel of the region, by one HIP kernel
    (``phaseshift_decode_kernel``).

    Per set of four images ``I0 .. I3`` (``cos(theta + i pi / 2)`` expected): ``theta = mod(arctan2(I3 - I1, I0 - I2), 2 pi)``.
    The first period of an axis gives the absolute phase; every later period ``T`` refines it against the first ``T0``
    (heterodyne principle): ``k = rint((phi * T0 / T - theta) / (2 pi))``, ``phi = (theta + 2 pi k) * T / T0``.  Finally
    ``px = width * phi_x / (2 pi)`` and ``py = height * phi_y / (2 pi)``: as ``getProjCoord`` scales by the projector's
    resolution, not by the first period, the coordinates are pixels only when ``periods[v][0]`` equals the projector's extent
    along that axis (the reference's behaviour; nothing is raised otherwise).  fp64, the reference's operations in its order;
    ``arctan2`` is the device library's, so the result is close to numpy's, not bit-equal.  At an exact tie of a heterodyne
    step, ``phi * T0 / T - theta`` an odd multiple of ``pi`` -- clean fringes never meet one, unstructured input (noise) does at
    about one pixel in 10 000 --, ``k`` depends on the last bit of ``arctan2``, and the result may differ from numpy's by one
    period ``T`` of that step, as numpy's does from the same chain in long double.

    Parameters
    ----------
    images : ndarray or CUDA/HIP tensor uint8 ``[M, Hc, Wc]``, or a sequence of ``[Hc, Wc]`` uint8 arrays (stacked on the host)
        In the order of :func:`phaseShiftPattern`.  ``M >= N = 4 * (nx + ny)``; only the first N are read, so the reference's
        trailing image in normal light may stay in the stack.
    periods : (list_x, list_y)
        As the reference's: the periods of the fringes along x and along y, each 1 .. 8 finite positive numbers.
    projRes : (width, height)
        Of the projector, each 1 .. 65536.
    maps : (mapx, mapy), optional
        float32 ``[Hc, Wc]``: every image is sampled as :func:`grayCodeDecode` samples it.  Default: the images as they are.
    roi : (x, y, width, height), optional
        The region ``[y, y + height) x [x, x + width)``.  Default: the whole image.
    min_modulation : number >= 0, optional
        A pixel for which any set has ``sqrt((I3 - I1)^2 + (I0 - I2)^2) / 2 < min_modulation`` becomes (NaN, NaN).  The
        rule is exact: with ``a = I3 - I1``, ``b = I0 - I2`` and ``m`` the double passed, taken as the real number it is, a
        set masks its pixel iff ``a^2 + b^2 < 4 m^2`` -- nothing is rounded, neither a square root nor ``4 m^2``.  The kernel
        compares integers, ``a^2 + b^2 < min(ceil(4 m^2), 130051)`` with the ceiling taken on rationals (``inf`` masks every
        pixel, any ``m > 0`` masks ``a = b = 0``).  Default None: no pixel is masked, as in the reference.

    Returns
    -------
    ndarray or tensor
        float64 ``[h, w, 2]``: ``(px, py)``.  A tensor on the images' device, computed on its current stream, for a tensor.
    """
    tx, ty = _periods(periods)
    proj = _proj_res(projRes)
    thr2 = _mod_thr2(min_modulation)
    stack, dev = _gray_stack(images)
    mx, my = _gray_maps(maps, stack, dev)
    box = _roi(roi, (int(stack.shape[2]), int(stack.shape[1])))
    args = _phase_decode_args(stack, tx, ty, proj, thr2, mx, my, box)
    return _phase_decode(stack, args, box[3], box[2])


class PhaseShift:
    """
    A phase-shift scanner with a calibrated camera-projector rig: image stack in, dense cloud out, by two HIP kernels --
    :func:`phaseShiftDecode` with the camera's undistortion maps fused in, then ``StructuredLightRig.triangulate`` on the
    pixel grid.

    Camera pixel ``(x, y)`` and projector point ``(px, py)`` carry no half-pixel offsets.  That is the convention of the
    calibration routine whose formulae these are (``calibration.phaseShift`` pairs ``cornerSubPix`` coordinates, pixel centres
    at integers, with ``width * phi / (2 pi)``).  A user of another convention decodes with :func:`phaseShiftDecode` and calls
    ``StructuredLightRig.triangulate`` with points of their own.

    Parameters
    ----------
    rig : StereoRig
        Camera in position 1 (world origin), projector in position 2.  Held as a ``StructuredLightRig`` (``self.rig``).
    periods : (list_x, list_y)
        As :func:`phaseShiftDecode` takes them.
    min_modulation : number >= 0, optional
        As :func:`phaseShiftDecode` takes it: a set masks its pixel iff ``a^2 + b^2 < 4 m^2`` exactly, ``m`` the double as
        the real number it is.  Default None.

    At an exact tie of a heterodyne step, which only unstructured input produces, the decoded coordinate (and so the point)
    may lie one period of that step from numpy's: see :func:`phaseShiftDecode`.
    """

    def __init__(self, rig, periods, min_modulation=None):
        self.rig = rig if isinstance(rig, StructuredLightRig) else StructuredLightRig(rig)
        self.periods = _periods(periods)
        self.min_modulation = min_modulation
        self._thr2 = _mod_thr2(min_modulation)
        self._proj = _proj_res(self.rig.res2)
        self._cache = self.rig._cache    # _cached_maps' entries, shared with the rig's undistortCameraImage

    def getCloud(self, images, roi=None):
        """
        The dense cloud of a stack of phase-shift images.

        Parameters
        ----------
        images : what :func:`phaseShiftDecode` takes
            Of the rig's ``res1``, in the order of :func:`phaseShiftPattern`; any following extra image is ignored.
        roi : (x, y, width, height), optional
            Default None: the whole image.

        Returns
        -------
        ndarray or tensor
            float64 ``[h, w, 3]``, NaN at the masked pixels.  For a tensor a tensor on its device: the two kernels are queued
            on the current stream and nothing is read back.
        """
        size = (int(self.rig.res1[0]), int(self.rig.res1[1]))
        stack, dev = _gray_stack(images, size)
        box = _roi(roi, size)
        geom = self.rig._geometry()
        mx, my = _cached_maps(self._cache, self.rig, stack.device if dev else None)
        args = _phase_decode_args(stack, self.periods[0], self.periods[1], self._proj, self._thr2, mx, my, box)
        x0, y0, w, h = box
        proj = _phase_decode(stack, args, h, w)
        gp = geom.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        return _native.run("ssamd_sl_triangulate", (proj,), (h, w, 3), lambda p, out: (None, p, h * w, w, x0, y0, gp, out), _INVALID)
