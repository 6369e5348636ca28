"""Record what the C ABI answers to bad arguments: the return code and the ``ssamd_last_error()`` text of every call of CASES.

    python tests/golden/make_golden_abi_errors.py [output directory, default: this one]

Most calls break two rules at once, so that what is recorded is the ORDER of the argument checks as well as their wording.  Every
call fails, or returns 0 for an empty job, before a kernel is launched; the matcher checks run behind the device context, so a GPU
is needed.  The library asked is the one ``simplestereo_amd._native`` loads -- the tree's own ``libssamd.so``, or another build of
the same ABI named by ``SSAMD_LIB`` (with ``SSAMD_EXPERIMENT=1``).  The committed fixture was taken from the commit BEFORE the host
side of the library was cut into sections.  The two rows of ``ssamd_gsw_argmins`` were added with that entry point; recording them changed no
other row.

Writes ``abi_errors.json``: one row {"family", "entry", "args", "rc", "error"} per call; "error" is null where rc is 0 (the
library keeps the previous call's message then).  ``tests/test_gpu_abi_errors.py`` repeats the calls and wants every row back.

An argument is a number, or
    "NULL"                  a null pointer (also: the default stream)
    "nan", "inf"            the double
    ["host", n]             n zero bytes on the host
    ["dev", n, offset]      n zero bytes on the device, the pointer moved `offset` bytes off its 256-byte alignment
    ["ints", [...]]         int32 array on the host
    ["doubles", v, n]       n doubles of value v on the host (v may be "nan")
    ["str", text]           const char *
    ["longlong"]            pointer to a long long on the host
"""
import ctypes
import json
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

H, W = 8, 16
NULL, HOST, DEV = "NULL", ["host", H * W * 3], ["dev", H * W * 3, 0]
ASW = [5, 4, 0, 5.0, 17.5, 0]               # winSize, maxDisparity, minDisparity, gammaC, gammaP, consistent
GSW = [5, 4, 0, 10, 120.0, 1, 20]           # winSize, maxDisparity, minDisparity, gamma, fMax, iterations, bins
PI = math.pi
GEOM = ["doubles", 1.0, 68]                 # SSAMD_FTP_CLOUD_NGEOM
BAND = ["doubles", 0.1, H]


def _with(tail, **kw):
    """ASW / GSW with some of its parameters replaced by name"""
    names = ("win", "maxD", "minD", "gammaC", "gammaP", "consistent") if len(tail) == 6 else \
        ("win", "maxD", "minD", "gamma", "fMax", "iterations", "bins")
    return [kw.get(n, v) for n, v in zip(names, tail)]


def _cases():
    c = []

    def add(family, entries, *args):
        for e in entries.split():
            c.append({"family": family, "entry": e, "args": list(args)})

    # ---- np.unwrap: the plan's verdict comes before the NULL check; an empty geometry returns 0 whatever the pointers
    for sfx, LAST in (("", -1), ("_device", NULL)):
        add("np_unwrap", "ssamd_np_unwrap" + sfx, NULL, -1, 4, 1, PI, 2 * PI, NULL, LAST)
        add("np_unwrap", "ssamd_np_unwrap" + sfx, NULL, 0, 4, 1, PI, 2 * PI, NULL, LAST)
        add("np_unwrap", "ssamd_np_unwrap" + sfx, NULL, 2, 4, 1, PI, 2 * PI, NULL, LAST)
        add("np_unwrap", "ssamd_np_unwrap" + sfx, HOST, -1, 4, 1, PI, "nan", HOST, LAST)
        add("np_unwrap", "ssamd_np_unwrap" + sfx, HOST, -1, 4, 1, PI, "inf", HOST, LAST)
        add("np_unwrap", "ssamd_np_unwrap" + sfx, NULL, 2, 4, 1, PI, -1.0, NULL, LAST)
        add("np_unwrap", "ssamd_np_unwrap" + sfx, NULL, 1 << 20, 1 << 20, 2, PI, 2 * PI, NULL, LAST)
        add("np_unwrap", "ssamd_np_unwrap_xy" + sfx, NULL, -1, 4, 4, NULL, LAST)
        add("np_unwrap", "ssamd_np_unwrap_xy" + sfx, NULL, 0, 4, 4, NULL, LAST)
        add("np_unwrap", "ssamd_np_unwrap_xy" + sfx, NULL, 1, 4, 4, NULL, LAST)
    add("np_unwrap", "ssamd_np_unwrap_plan", -1, 4, 1, NULL)
    # ---- FTP cloud
    for sfx, LAST in (("", -1), ("_device", NULL)):
        add("ftp_cloud", "ssamd_ftp_cloud" + sfx, NULL, 0, 4, 0, 0, GEOM, 0.0, NULL, LAST)
        add("ftp_cloud", "ssamd_ftp_cloud" + sfx, HOST, 4, 4, -1, 0, NULL, 0.0, HOST, LAST)
        add("ftp_cloud", "ssamd_ftp_cloud" + sfx, HOST, 4, 4, 0, 0, ["doubles", "nan", 68], "nan", HOST, LAST)
        add("ftp_cloud", "ssamd_ftp_cloud" + sfx, HOST, 4, 4, 0, 0, ["doubles", "nan", 68], 1.0, HOST, LAST)
        add("ftp_cloud", "ssamd_ftp_cloud" + sfx, NULL, 4, 4, 0, 0, GEOM, 0.0, NULL, LAST)
        add("ftp_cloud", "ssamd_ftp_cloud" + sfx, NULL, 65536, 32768, 0, 0, NULL, 0.0, NULL, LAST)
        add("ftp_cloud", "ssamd_ftp_cloud" + sfx, NULL, 0, 4, 0, 0, NULL, 0.0, NULL, LAST)
    add("ftp_cloud", "ssamd_ftp_cloud_device", ["dev", 128, 8], 4, 4, 0, 0, GEOM, 0.0, ["dev", 384, 0], NULL)
    add("ftp_cloud", "ssamd_ftp_cloud_device", ["dev", 128, 0], 4, 4, 0, 0, GEOM, 0.0, ["dev", 384, 8], NULL)
    # ---- FTP phase: (obj, ch_obj, ref, ch_ref, h, w, fmin, fmax, unwrap, tau, out)
    for sfx, LAST in (("", -1), ("_device", NULL)):
        add("ftp_phase", "ssamd_ftp_phase" + sfx, NULL, 2, NULL, 3, 4, 4, BAND, BAND, 0, 0.5, NULL, LAST)
        add("ftp_phase", "ssamd_ftp_phase" + sfx, HOST, 1, HOST, 1, 4, 9000, BAND, BAND, 3, 0.5, HOST, LAST)
        add("ftp_phase", "ssamd_ftp_phase" + sfx, HOST, 2, HOST, 1, 0, 4, BAND, BAND, 0, 0.5, HOST, LAST)
        add("ftp_phase", "ssamd_ftp_phase" + sfx, HOST, 2, HOST, 1, 4, 4, NULL, NULL, 0, 0.5, HOST, LAST)
        add("ftp_phase", "ssamd_ftp_phase" + sfx, HOST, 1, HOST, 3, 4, 4, NULL, BAND, 3, 0.5, HOST, LAST)
        add("ftp_phase", "ssamd_ftp_phase" + sfx, HOST, 1, HOST, 1, 4, 9000, BAND, BAND, 1, 2.0, HOST, LAST)
        add("ftp_phase", "ssamd_ftp_phase" + sfx, HOST, 1, HOST, 1, 4, 4, BAND, BAND, 1, 2.0, HOST, LAST)
    add("ftp_phase", "ssamd_ftp_band", 0, -1, NULL, NULL, NULL, NULL)
    add("ftp_phase", "ssamd_ftp_band", 4, 2, NULL, NULL, NULL, NULL)
    # ---- IIR unwrap: (phase, n, h, w, tau, out)
    for sfx, LAST in (("", -1), ("_device", NULL)):
        add("iir_unwrap", "ssamd_iir_unwrap" + sfx, NULL, 1, 4, 4, 2.0, NULL, LAST)
        add("iir_unwrap", "ssamd_iir_unwrap" + sfx, HOST, 0, 4, 4, 0.5, HOST, LAST)
        add("iir_unwrap", "ssamd_iir_unwrap" + sfx, HOST, -1, 4, 4, 2.0, HOST, LAST)
        add("iir_unwrap", "ssamd_iir_unwrap" + sfx, HOST, 1, 4, 100000, 2.0, HOST, LAST)
        add("iir_unwrap", "ssamd_iir_unwrap" + sfx, HOST, 1, 4, 100000, 0.5, HOST, LAST)
        add("iir_unwrap", "ssamd_iir_unwrap" + sfx, HOST, 0, 4, 100000, -0.5, HOST, LAST)
    # ---- ASW / GSW on device buffers: (img1, img2, H, W, out_row0, out_rows, [skip_row0, skip_rows,] parameters, disparity, stream)
    for tail, entries in ((ASW, "ssamd_asw_device_rows2 ssamd_asw_exact_device_rows2"), (GSW, "ssamd_gsw_device_rows2")):
        add("device_matchers", entries, DEV, DEV, H, W, 0, H, 6, 4, *_with(tail, win=4), DEV, NULL)
        add("device_matchers", entries, NULL, DEV, H, W, 0, H, 6, 4, *tail, DEV, NULL)
        add("device_matchers", entries, DEV, DEV, H, W, 0, H, 2, -1, *_with(tail, win=4), DEV, NULL)
        add("device_matchers", entries, DEV, DEV, H, W, 2, 4, 1, 2, *tail, NULL, NULL)
        add("device_matchers", entries, DEV, DEV, H, W, 2, 4, 1, 2, *tail, DEV, NULL)
        add("device_matchers", entries, DEV, DEV, H, W, 0, H, 2, 2, *_with(tail, win=4, minD=-1), DEV, NULL)
        add("device_matchers", entries, DEV, DEV, H, W, 4, H, 5, 2, *tail, DEV, NULL)
        add("device_matchers", entries, DEV, DEV, 0, W, 0, H, 0, 0, *_with(tail, win=4), DEV, NULL)
        add("device_matchers", entries, DEV, DEV, H, W, 3, 0, 0, 0, *tail, NULL, NULL)
    add("device_matchers", "ssamd_asw_device ssamd_asw_exact_device", DEV, DEV, H, W, 0, H, *_with(ASW, win=4, gammaC=0.0), DEV, NULL)
    add("device_matchers", "ssamd_asw_device ssamd_asw_exact_device", DEV, DEV, H, W, 0, H, *_with(ASW, gammaC=0.0, maxD=40000), DEV, NULL)
    add("device_matchers", "ssamd_asw_device ssamd_asw_exact_device", DEV, DEV, H, W, 0, H, *_with(ASW, gammaC=0.0), DEV, NULL)
    add("device_matchers", "ssamd_asw_device ssamd_asw_exact_device", DEV, DEV, H, W, 0, H, *_with(ASW, win=257), NULL, NULL)
    add("device_matchers", "ssamd_asw_device_rows2 ssamd_asw_exact_device_rows2", DEV, DEV, H, W, 0, H, 0, H, *_with(ASW, gammaC=0.0), DEV, NULL)
    add("device_matchers", "ssamd_asw_alternate_device", NULL, DEV, H, W, *_with(ASW, win=4), DEV, NULL)
    add("device_matchers", "ssamd_asw_alternate_device", DEV, DEV, H, W, *_with(ASW, win=4, gammaP=0.0), DEV, NULL)
    add("device_matchers", "ssamd_gsw_device", DEV, DEV, H, W, 0, H, *_with(GSW, gamma=0, win=4), DEV, NULL)
    add("device_matchers", "ssamd_gsw_device", DEV, DEV, H, W, 0, H, *_with(GSW, gamma=0), DEV, NULL)
    add("device_matchers", "ssamd_gsw_device", NULL, DEV, H, W, 0, H, *_with(GSW, gamma=0), DEV, NULL)
    add("device_matchers", "ssamd_gsw_device_rows2", DEV, DEV, H, W, 0, H, 0, 0, *_with(GSW, gamma=0, win=4), DEV, NULL)
    add("device_matchers", "ssamd_gsw_device_rows2", DEV, DEV, H, W, 0, H, 0, 0, *_with(GSW, gamma=0), DEV, NULL)
    add("device_matchers", "ssamd_gsw_device_rows2", DEV, DEV, H, W, 0, H, 2, 2, *_with(GSW, gamma=0), DEV, NULL)
    add("device_matchers", "ssamd_gsw_device_rows2", DEV, DEV, H, W, 0, H, 0, 0, *_with(GSW, gamma=0, maxD=40000), DEV, NULL)
    # (img1, img2, H, W, out_row0, out_rows, row_parity, ...)
    add("device_matchers", "ssamd_asw_alternate_rows_device", NULL, DEV, H, W, 0, H, 2, *ASW, DEV, NULL)
    add("device_matchers", "ssamd_asw_alternate_rows_device", DEV, DEV, H, W, 0, H, 2, *_with(ASW, win=4), DEV, NULL)
    add("device_matchers", "ssamd_asw_alternate_rows_device", DEV, DEV, H, W, 0, H, 1, *_with(ASW, win=4), DEV, NULL)
    add("device_matchers", "ssamd_asw_alternate_rows_device", DEV, DEV, H, W, 0, H, 1, *_with(ASW, gammaC=0.0), DEV, NULL)
    add("device_matchers", "ssamd_asw_alternate_rows_device", DEV, DEV, H, W, 0, H + 1, 1, *ASW, DEV, NULL)
    add("device_matchers", "ssamd_asw_alternate_rows_device", DEV, DEV, H, W, 2, 0, 1, *_with(ASW, gammaC=0.0), DEV, NULL)
    # ---- the rig: (raw1, raw2, src_h, src_w, mapx1, mapy1, mapx2, mapy2, H, W, interpolation, parameters, disparity, stream)
    MAP = ["dev", H * W * 4, 0]
    for tail, entries in ((ASW, "ssamd_asw_rectified_device ssamd_asw_exact_rectified_device"), (GSW, "ssamd_gsw_rectified_device")):
        add("rig", entries, DEV, DEV, H, W, MAP, NULL, MAP, MAP, H, W, 2, *tail, DEV, NULL)
        add("rig", entries, DEV, DEV, 0, W, MAP, MAP, MAP, MAP, H, W, 2, *tail, DEV, NULL)
        add("rig", entries, DEV, DEV, H, W, MAP, MAP, MAP, MAP, H, W, 2, *_with(tail, win=4), DEV, NULL)
        add("rig", entries, DEV, DEV, H, W, MAP, MAP, MAP, MAP, H, W, 1, *_with(tail, win=4, minD=-1), DEV, NULL)
        add("rig", entries, DEV, DEV, H, W, MAP, MAP, MAP, MAP, H, W, 1, *_with(tail, win=4), NULL, NULL)
        add("rig", entries, DEV, DEV, H, W, MAP, MAP, MAP, MAP, 0, W, 0, *_with(tail, win=4), DEV, NULL)
    add("rig", "ssamd_gsw_rectified_device", DEV, DEV, H, W, MAP, MAP, MAP, MAP, H, W, 1, *_with(GSW, gamma=0), DEV, NULL)
    # (src, src_h, src_w, mapx, mapy, dst_h, dst_w, interpolation, dst, stream)
    add("rig", "ssamd_remap_bgr_device", DEV, H, W, ["dev", H * W * 4, 4], MAP, H, W, 2, DEV, NULL)
    add("rig", "ssamd_remap_bgr_device", DEV, H, W, ["dev", H * W * 4, 4], MAP, H, W, 1, DEV, NULL)
    add("rig", "ssamd_remap_bgr_device", DEV, H, W, MAP, MAP, H, W, 0, ["dev", H * W * 3, 2], NULL)
    add("rig", "ssamd_remap_bgr_device", NULL, 0, W, MAP, MAP, H, W, 2, DEV, NULL)
    add("rig", "ssamd_remap_bgr_device", DEV, H, W, ["dev", H * W * 4, 4], MAP, 0, W, 2, DEV, NULL)
    # (disparity, h, w, Q, points, stream)
    Q = ["doubles", 1.0, 16]
    add("rig", "ssamd_reproject_device", NULL, 0, W, Q, DEV, NULL)
    add("rig", "ssamd_reproject_device", DEV, H, W, NULL, DEV, NULL)
    add("rig", "ssamd_reproject_device", DEV, 0, W, Q, DEV, NULL)
    add("rig", "ssamd_reproject_device", ["dev", 256, 2], 70000, W, Q, DEV, NULL)
    add("rig", "ssamd_reproject_device", ["dev", 256, 2], H, W, Q, DEV, NULL)
    add("rig", "ssamd_reproject_device", DEV, H, W, Q, ["dev", 1536, 8], NULL)
    # ---- the matchers on host arrays: (img1, img2, H, W, parameters, disparity, device)
    OUT = ["host", H * W * 2]
    for tail, entries in ((ASW, "ssamd_asw ssamd_asw_exact ssamd_asw_alternate"), (GSW, "ssamd_gsw")):
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=4, minD=-1), OUT, -1)
        add("host_matchers", entries, NULL, HOST, H, W, *_with(tail, win=4), OUT, -1)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=4), NULL, -1)
        add("host_matchers", entries, HOST, HOST, 0, W, *_with(tail, minD=-1), OUT, -1)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, minD=-1, maxD=40000), OUT, -1)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=257), OUT, -1)
    add("host_matchers", "ssamd_gsw", HOST, HOST, H, W, *_with(GSW, gamma=0), OUT, -1)
    add("host_matchers", "ssamd_gsw", HOST, HOST, H, W, *_with(GSW, gamma=0, win=4), OUT, -1)
    add("host_matchers", "ssamd_asw ssamd_asw_exact ssamd_asw_alternate", HOST, HOST, H, W, *_with(ASW, gammaC=0.0, gammaP=0.0), OUT, -1)
    COSTS = ["host", H * W * 4 * 5]
    add("host_matchers", "ssamd_asw_costs", HOST, HOST, H, W, 5, 3, 4, 5.0, 17.5, COSTS, -1)
    add("host_matchers", "ssamd_asw_costs", HOST, HOST, H, W, 4, 3, 4, 5.0, 17.5, NULL, -1)
    add("host_matchers", "ssamd_asw_costs", HOST, HOST, H, W, 4, 3, 4, 5.0, 17.5, COSTS, -1)
    add("host_matchers", "ssamd_asw_costs", HOST, HOST, H, W, 4, 4, 0, 5.0, 17.5, COSTS, -1)
    add("host_matchers", "ssamd_asw_argmins", HOST, HOST, H, W, 5, 3, 4, 5.0, 17.5, OUT, OUT, -1)
    add("host_matchers", "ssamd_asw_argmins", HOST, HOST, H, W, 4, 3, 4, 5.0, 17.5, OUT, NULL, -1)
    add("host_matchers", "ssamd_asw_argmins", HOST, HOST, H, W, 4, 3, 4, 5.0, 17.5, OUT, OUT, -1)
    add("host_matchers", "ssamd_asw_argmins", HOST, HOST, H, W, 5, 4, 0, 0.0, 17.5, OUT, OUT, -1)
    add("host_matchers", "ssamd_gsw_argmins", HOST, HOST, H, W, *_with(GSW, win=4), OUT, NULL, -1)
    add("host_matchers", "ssamd_gsw_argmins", HOST, HOST, H, W, *_with(GSW, win=4), OUT, OUT, -1)
    # (..., disparity, devices, n_devices)
    for tail, entries in ((ASW, "ssamd_asw_multi ssamd_asw_exact_multi ssamd_asw_alternate_multi"), (GSW, "ssamd_gsw_multi")):
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=4), OUT, ["ints", [0]], 0)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=4), OUT, NULL, 1)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=4), OUT, ["ints", [-1] * 17], 17)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=4), OUT, ["ints", [0, -1]], 2)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=4), OUT, ["ints", [0, 0]], 2)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=4), OUT, ["ints", [0]], 1)
        add("host_matchers", entries, HOST, HOST, H, W, *tail, NULL, NULL, 0)
        add("host_matchers", entries, HOST, HOST, H, W, *_with(tail, win=257), OUT, ["ints", [99]], 1)
    # ---- library-wide and verification entry points
    add("library", "ssamd_counter", -1, ["str", "no_such_counter"], ["longlong"])
    add("library", "ssamd_counter", -1, NULL, ["longlong"])
    add("library", "ssamd_counter", 99, ["str", "no_such_counter"], NULL)
    add("library", "ssamd_set_option", ["str", "SSAMD_NO_SUCH_OPTION"], ["str", "1"])
    add("library", "ssamd_set_option", ["str", "SSAMD_NO_SUCH_OPTION"], NULL)
    add("library", "ssamd_set_option", NULL, ["str", "1"])
    add("library", "ssamd_debug_libm", 4, 4, HOST, HOST)
    add("library", "ssamd_debug_libm", 4, -1, NULL, HOST)
    add("library", "ssamd_debug_libm", 0, 0, HOST, HOST)
    add("library", "ssamd_debug_gsw_sqrt", 0, HOST)
    add("library", "ssamd_debug_gsw_sqrt", 4, NULL)
    add("library", "ssamd_debug_exact_queue", 0, -1, NULL, NULL, NULL)
    add("library", "ssamd_debug_exact_queue", 0, 4, NULL, NULL, ["longlong"])
    add("library", "ssamd_debug_exact_costs", HOST, HOST, H, W, 4, 5.0, 17.5, -1, NULL, NULL, NULL, NULL)
    add("library", "ssamd_debug_exact_costs", HOST, HOST, H, W, 4, 5.0, 17.5, 0, ["ints", [0, 0, 0]], ["host", 64], NULL, NULL)
    add("library", "ssamd_bgr2lab", NULL, 0, W, NULL, 99)
    add("library", "ssamd_bgr2lab", HOST, H, 0, NULL, 99)
    for entry in ("ssamd_asw_geometry", "ssamd_asw_kernel_form", "ssamd_gsw_geometry"):
        add("library", entry, W, H, 4, 4, 0, NULL)
        add("library", entry, W, H, 4, 3, 4, ["ints", [0] * 16])
        add("library", entry, W, H, 5, 3, 4, ["ints", [0] * 16])
        add("library", entry, 0, H, 5, 4, -1, ["ints", [0] * 16])
    return c


CASES = _cases()


def _double(v):
    return float(v) if isinstance(v, str) else v


def call(case, _native, dry=False):
    """(return code, message or None) of one case on the library ``_native`` has loaded; dry: only convert the arguments (no GPU)"""
    L = _native.lib()
    fn = getattr(L, case["entry"])
    assert len(fn.argtypes) == len(case["args"]), case
    keep, argv = [], []
    for a, ctype in zip(case["args"], fn.argtypes):
        arr = None
        if a == "NULL":
            v = None
        elif isinstance(a, str):
            v = float(a)
        elif not isinstance(a, list):
            v = a
        elif a[0] == "dev" and dry:
            v = 4096 + a[2]
        elif a[0] == "dev":
            import torch
            t = torch.zeros(a[1] + 256, dtype=torch.uint8, device="cuda")
            keep.append(t)
            v = t.data_ptr() + a[2]
            assert t.data_ptr() % 256 == 0
        elif a[0] == "str":
            v = a[1].encode()
        elif a[0] == "host":
            arr = np.zeros(a[1], np.uint8)
        elif a[0] == "ints":
            arr = np.array(a[1], np.int32)
        elif a[0] == "doubles":
            arr = np.full(a[2], _double(a[1]), np.float64)
        else:
            assert a == ["longlong"], a
            arr = np.zeros(1, np.int64)
        if arr is not None:
            keep.append(arr)
            v = arr.ctypes.data if ctype is ctypes.c_void_p else arr.ctypes.data_as(ctype)
        argv.append(v)
    if dry:
        return [t.from_param(v) for t, v in zip(fn.argtypes, argv)]
    rc = fn(*argv)
    return rc, (L.ssamd_last_error().decode("utf-8", "replace") if rc else None)


def replay(cases, _native):
    rows = []
    for case in cases:
        rc, err = call(case, _native)
        rows.append(dict(case, rc=rc, error=err))
    return rows


def main(out_dir):
    from simplestereo_amd import _native
    rows = replay(CASES, _native)
    with open(os.path.join(out_dir, "abi_errors.json"), "w") as f:
        json.dump(rows, f, indent=0)
    print("library", _native.LIB_PATH)
    print(len(rows), "calls,", sum(1 for r in rows if r["rc"] == 0), "return 0;", len({r["error"] for r in rows}), "distinct messages")
    for r in rows:
        print("%-36s %3d  %s" % (r["entry"], r["rc"], r["error"]))


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else HERE)
