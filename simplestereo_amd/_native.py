"""ctypes binding of libssamd.so (C ABI in include/ssamd.h, include/ssamd_active.h, include/ssamd_graycode.h,
include/ssamd_ftp_mapping.h, include/ssamd_structured_light.h and include/ssamd_graycode_stereo.h).

This is the only place Python touches the native library.  There is no Python or
CPU fallback for the operators: if the library is missing, or no HIP device is
visible, the calls fail loudly.
"""
import ctypes
import os

import numpy as np

from .build import LIB_PATH as _DEFAULT_LIB_PATH

# experiments only (a library built from another source tree, tools/ab_tree.py): another build of the same library is loaded
# only when the caller says twice that this is an experiment -- such a build need not compute the product's maps
LIB_PATH = _DEFAULT_LIB_PATH
if os.environ.get("SSAMD_LIB"):
    if os.environ.get("SSAMD_EXPERIMENT") != "1":
        raise ImportError("SSAMD_LIB is an experiment hook: set SSAMD_EXPERIMENT=1 as well to load %s instead of the product "
                          "library" % os.environ["SSAMD_LIB"])
    LIB_PATH = os.environ["SSAMD_LIB"]
ABI_VERSION = 8
ACTIVE_VERSION = 1         # SSAMD_ACTIVE_VERSION of include/ssamd_active.h, the second public header of the same library
GRAYCODE_VERSION = 1       # SSAMD_GRAYCODE_VERSION of include/ssamd_graycode.h, the third
FTP_MAPPING_VERSION = 1    # SSAMD_FTP_MAPPING_VERSION of include/ssamd_ftp_mapping.h, the fourth
SL_VERSION = 1             # SSAMD_SL_VERSION of include/ssamd_structured_light.h, the fifth
GRAYCODE_STEREO_VERSION = 1    # SSAMD_GRAYCODE_STEREO_VERSION of include/ssamd_graycode_stereo.h, the sixth
STEREO_LAST, STEREO_MEAN = 0, 1     # SSAMD_STEREO_LAST, SSAMD_STEREO_MEAN: its reduce modes
GRAYCODE_BLOCK = 1024      # SSAMD_GRAYCODE_BLOCK: pixels per block of the decode counts and the offsets

(K_LAB, K_ASW_AGG, K_ASW_FIN, K_GSW_AGG, K_GSW_FIN, K_REMAP, K_REPROJECT, K_ASW_ALT, K_ASW_EXACT, K_UNWRAP, K_FTP,
 K_NPUNWRAP, K_COUNT) = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
OK, EINVAL, ENODEVICE, EHIP, ENOMEM, ELIMIT = 0, -1, -2, -3, -4, -5

_lib = None

# Every function of include/ssamd.h once: argument types -> the entry points that take them.  i int, l long long, d double,
# f float, p a buffer (host or device) or a stream, s const char *, I / L / D pointers to int (int32_t) / long long / double;
# all return int but the two of _RETURN_STRING.  tests/test_native_signatures_cpu.py holds the table to the header.
_ASW, _GSW = "iiiddi", "iiiifii"      # winSize, maxDisparity, minDisparity + gammaC, gammaP, consistent / gamma, fMax, iterations, bins
_SIGNATURES = (
    ("", "ssamd_abi_version ssamd_last_error ssamd_device_count ssamd_profile_reset"),
    ("ppii" + _ASW + "pi", "ssamd_asw ssamd_asw_exact ssamd_asw_alternate"),
    ("ppii" + _ASW + "pIi", "ssamd_asw_multi ssamd_asw_exact_multi ssamd_asw_alternate_multi"),
    ("ppiiii" + _ASW + "pp", "ssamd_asw_device ssamd_asw_exact_device"),
    ("ppiiiiii" + _ASW + "pp", "ssamd_asw_device_rows2 ssamd_asw_exact_device_rows2"),
    ("ppiippppiii" + _ASW + "pp", "ssamd_asw_rectified_device ssamd_asw_exact_rectified_device"),
    ("ppii" + _ASW + "pp", "ssamd_asw_alternate_device"),
    ("ppiiiii" + _ASW + "pp", "ssamd_asw_alternate_rows_device"),
    ("ppii" + _GSW + "pi", "ssamd_gsw"),
    ("ppii" + _GSW + "pIi", "ssamd_gsw_multi"),
    ("ppiiii" + _GSW + "pp", "ssamd_gsw_device"),
    ("ppiiiiii" + _GSW + "pp", "ssamd_gsw_device_rows2"),
    ("ppiippppiii" + _GSW + "pp", "ssamd_gsw_rectified_device"),
    ("ppiiiiiddpi", "ssamd_asw_costs"),
    ("ppiiiiiddppi", "ssamd_asw_argmins"),
    ("ppii" + _GSW + "ppi", "ssamd_gsw_argmins"),
    ("piipi", "ssamd_bgr2lab"),
    ("piippiiipp", "ssamd_remap_bgr_device"),
    ("piiDpp", "ssamd_reproject_device"),
    ("iipppp", "ssamd_ftp_band"),
    ("lllI", "ssamd_np_unwrap_plan"),
    ("ilppp", "ssamd_debug_exact_queue"),
    ("iipp", "ssamd_debug_libm"),
    ("ppiiiddipppp", "ssamd_debug_exact_costs"),
    ("ip", "ssamd_debug_gsw_sqrt"),
    ("i", "ssamd_profile_enable ssamd_kernel_name ssamd_autotune"),
    ("DL", "ssamd_profile_read"),
    ("iiiiiI", "ssamd_asw_geometry ssamd_asw_kernel_form ssamd_gsw_geometry"),
    ("ss", "ssamd_set_option"),
    ("isL", "ssamd_counter"),
    # include/ssamd_graycode.h (SSAMD_GRAYCODE_VERSION); tests/test_graycode_cpu.py holds these rows to that header
    ("piiipp" + 9 * "i" + "DipIi", "ssamd_graycode_cloud"),
    ("piiiiDppp", "ssamd_graycode_cloud_device"),
    # include/ssamd_graycode_stereo.h (SSAMD_GRAYCODE_STEREO_VERSION); tests/test_graycode_stereo_cpu.py holds these rows to that header
    (2 * "piiii" + "iiippi", "ssamd_graycode_stereo_match"),
    (2 * "piiii" + "iiipppp", "ssamd_graycode_stereo_match_device"),
    (2 * "piippiiii" + 7 * "i" + "DipIi", "ssamd_graycode_stereo_points"),
) + tuple((args + last, name + suffix) for args, name in (       # NAME(..., int device) and NAME_device(..., void *stream)
    ("piiidp", "ssamd_iir_unwrap"),
    ("plllddp", "ssamd_np_unwrap"),
    ("piiip", "ssamd_np_unwrap_xy"),
    ("pipiiippidp", "ssamd_ftp_phase"),
    ("piiiipdp", "ssamd_ftp_cloud"),
    # include/ssamd_active.h (SSAMD_ACTIVE_VERSION); tests/test_stereo_ftp_cpu.py holds these rows to that header
    ("piiiiiipp", "ssamd_ftp_reference"),
    ("piiiip", "ssamd_stripe_centroids"),
    ("piiipp" + 9 * "i" + "pp", "ssamd_graycode_decode"),
    ("pip", "ssamd_graycode_offsets"),
    # include/ssamd_ftp_mapping.h (SSAMD_FTP_MAPPING_VERSION); tests/test_ftp_mapping_cpu.py holds these rows to that header
    ("piiippidp", "ssamd_ftp_carrier_phase"),
    ("piiiiDDddp", "ssamd_ftp_mapping_cloud"),
    # include/ssamd_structured_light.h (SSAMD_SL_VERSION); tests/test_phaseshift_cpu.py holds these rows to that header
    ("piiipp" + 6 * "i" + "DDiiip", "ssamd_phaseshift_decode"),
    ("ppliiiDp", "ssamd_sl_triangulate"),
    ("piiDpp", "ssamd_graycode_stereo_cloud"),
    ("pplDp", "ssamd_stereo_triangulate"),
) for last, suffix in (("i", ""), ("p", "_device")))
_RETURN_STRING = ("ssamd_last_error", "ssamd_kernel_name")
_CTYPES = {"i": ctypes.c_int, "l": ctypes.c_longlong, "d": ctypes.c_double, "f": ctypes.c_float, "p": ctypes.c_void_p,
           "s": ctypes.c_char_p, "I": ctypes.POINTER(ctypes.c_int), "L": ctypes.POINTER(ctypes.c_longlong),
           "D": ctypes.POINTER(ctypes.c_double)}


class NativeError(RuntimeError):
    """A libssamd call returned an error code."""

    def __init__(self, code, msg):
        super().__init__("libssamd error %d: %s" % (code, msg))
        self.code = code
        self.message = msg


def lib():
    """Load libssamd.so (once).  Raises ImportError with build instructions if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "simplestereo_amd: native library %s is missing. Build it with "
            "`python -m simplestereo_amd.build` (needs hipcc, targets gfx950). "
            "There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.  When torch is importable it goes
    # first, so libssamd's DT_NEEDED libamdhip64 resolves to the copy torch already loaded (same SONAME) and device
    # tensors, streams and this library share a runtime; loaded the other way round, whichever runtime initialises
    # second sees no device.
    try:
        import torch  # noqa: F401
    except Exception:      # noqa: BLE001 -- absent or broken torch: host-array calls do not need it
        pass
    L = ctypes.CDLL(LIB_PATH)
    L.ssamd_abi_version.restype = ctypes.c_int
    if L.ssamd_abi_version() != ABI_VERSION:
        raise ImportError("%s has ABI version %d, this package needs %d: rebuild it with `python -m simplestereo_amd.build`"
                          % (LIB_PATH, L.ssamd_abi_version(), ABI_VERSION))
    for args, names in _SIGNATURES:
        for name in names.split():
            fn = getattr(L, name)
            fn.restype = ctypes.c_char_p if name in _RETURN_STRING else ctypes.c_int
            fn.argtypes = [_CTYPES[a] for a in args]
    _lib = L
    return L


def check(rc, invalid=()):
    """Raise for a negative return code: ``ValueError`` with the library's message for the codes in ``invalid`` (a bad argument
    of the caller's, e.g. ``(EINVAL, ELIMIT)``), ``NativeError`` for every other."""
    if rc != 0:
        msg = lib().ssamd_last_error().decode("utf-8", "replace")
        if rc in invalid:
            raise ValueError(msg) from None
        raise NativeError(rc, msg)


def is_device_tensor(x):
    return type(x).__module__.startswith("torch") and hasattr(x, "is_cuda") and bool(x.is_cuda)


def c_double(v, strict=True):
    """PyArg_ParseTuple 'd' / 'f': a float, an int (bool included) or anything with __float__ / __index__.  ``strict`` also
    refuses strings and numbers beyond a double; without it anything float() accepts passes."""
    if strict and isinstance(v, (str, bytes, bytearray)):
        raise ValueError("Invalid input format!")
    try:
        return float(v)
    except ((TypeError, ValueError, OverflowError) if strict else (TypeError, ValueError)):
        raise ValueError("Invalid input format!") from None


def call_on_stream(t, fn, *args, invalid=()):
    """``fn(*args, stream)`` of a ``*_device`` entry point with the device of the tensor ``t`` current and ``stream`` that
    device's current stream; return codes as in :func:`check`."""
    import torch
    with torch.cuda.device(t.device):
        rc = fn(*args, ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream))
        if rc:
            check(rc, invalid)


def run(name, sources, shape, args, invalid=(), dtype=np.float64):
    """The operator ``name`` on host arrays, or ``name + "_device"`` on device tensors (``sources``: all of one kind; made
    contiguous): the result of ``shape`` and ``dtype`` (a numpy dtype; float64 by default) is allocated like them and returned
    as it is, without a native call, when an extent is 0.  ``args(pointers of the sources ..., pointer of the result)`` gives every argument but the last, which is
    the current device (-1) or the current stream."""
    if is_device_tensor(sources[0]):
        import torch
        srcs = [s.contiguous() for s in sources]
        out = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=srcs[0].device)
        if 0 not in shape:
            call_on_stream(out, getattr(lib(), name + "_device"), *args(*[s.data_ptr() for s in srcs], out.data_ptr()), invalid=invalid)
        return out
    srcs = [np.ascontiguousarray(s) for s in sources]
    out = np.empty(shape, dtype=dtype)
    if 0 not in shape:
        check(getattr(lib(), name)(*args(*[s.ctypes.data for s in srcs], out.ctypes.data), -1), invalid)
    return out


def set_option(name, value):
    """Experiment / test hook: set one of the SSAMD_* tuning options of the loaded library; ``None`` puts it back to what
    the environment had set when the library was loaded (unset if it had not).  The environment variables of the same
    names are only read at load time."""
    check(lib().ssamd_set_option(name.encode(), None if value is None else str(value).encode()))


def counter(name, device=-1):
    """Diagnostic counter of a device context (``evol_fallbacks``, ``evol_bytes``: include/ssamd.h)."""
    v = ctypes.c_longlong(0)
    check(lib().ssamd_counter(device, name.encode(), ctypes.byref(v)))
    return int(v.value)


class options:
    """``with _native.options(SSAMD_ASW_GEOM="3,5,8"): ...`` -- set tuning options for a block; afterwards every one of
    them is back at its load-time value.  If setting one fails, the ones already set are rolled back."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        done = []
        try:
            for k, v in self.kw.items():
                set_option(k, v)
                done.append(k)
        except Exception:
            for k in done:
                set_option(k, None)
            raise
        return self

    def __exit__(self, *exc):
        for k in self.kw:
            set_option(k, None)
        return False


def profile_read():
    ms = (ctypes.c_double * K_COUNT)()
    n = (ctypes.c_longlong * K_COUNT)()
    check(lib().ssamd_profile_read(ms, n))
    return list(ms), list(n)


def asw_geometry(width, rows, winSize, maxDisparity, minDisparity):
    out = (ctypes.c_int * 8)()
    check(lib().ssamd_asw_geometry(width, rows, winSize, maxDisparity, minDisparity, out))
    keys = ("tile_x", "chunk_d", "n_chunks", "threads", "lds_bytes", "grid_x", "grid_y", "grid_z")
    return dict(zip(keys, list(out)))


def asw_kernel_form(width, rows, winSize, maxDisparity, minDisparity):
    out = (ctypes.c_int * 5)()
    check(lib().ssamd_asw_kernel_form(width, rows, winSize, maxDisparity, minDisparity, out))
    return dict(zip(("phase_shifted", "tile_columns", "chunk_columns", "build_first_waves", "wave_kernel"), list(out)))


def gsw_geometry(width, rows, winSize, maxDisparity, minDisparity):
    out = (ctypes.c_int * 9)()
    check(lib().ssamd_gsw_geometry(width, rows, winSize, maxDisparity, minDisparity, out))
    keys = ("tile_x", "chunk_d", "n_chunks", "threads", "lds_bytes", "grid_x", "grid_y", "grid_z", "strip_rows")
    return dict(zip(keys, list(out)))


def np_unwrap_plan(outer, length, inner):
    """Launch plan of ``unwrapping.unwrap`` for the geometry [outer][length][inner] (csrc/np_unwrap_plan.h; needs no device)."""
    out = (ctypes.c_int32 * 8)()
    check(lib().ssamd_np_unwrap_plan(outer, length, inner, out))
    keys = ("form", "chunk", "lanes", "threads", "blocks", "lds_bytes", "per_thread", "groups")
    d = dict(zip(keys, list(out)))
    d["form"] = "column" if d["form"] else "row"
    return d
