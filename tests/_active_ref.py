"""What tests/golden/make_golden_active_ref.py and the tests of its fixtures share: the container of
tests/golden/active_ref_cases.{npz,json} -- values recorded from the reference's own simplestereo/active.py, run with a cv2
stand-in (oracle/ref_active.py) --, the recipes that regenerate every input from the seeded helpers of the numpy
restatements, and the reference's in-place roi shift of StereoFTP_Mapping emulated on the restatement.

Nothing here imports simplestereo_amd, the reference or cv2."""
import io
import json
import os
import zipfile

import numpy as np

import _ftp_mapping_ref as M
import _graycode_ref as G
import _stereo_ftp_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NPZ, JSON = os.path.join(GOLDEN, "active_ref_cases.npz"), os.path.join(GOLDEN, "active_ref_cases.json")
PACK_FROM = 256             # float64 arrays of at least this many values are stored packed (pack / unpack below)


# ------------------------------------------------------------------------------------------------ the container
def pack(a):
    """float64 array -> uint8 [8, n], the same bits in a form deflate can shrink by two fifths: the x, y and z of a cloud apart
    (a last axis of 3 goes first), the int64 patterns differenced twice along the flattened array (wrapping: exact), and
    byte k of every value together"""
    v = np.moveaxis(a, -1, 0) if a.ndim >= 2 and a.shape[-1] == 3 else a
    i = np.ascontiguousarray(v).reshape(-1).view(np.int64)
    for _ in range(2):
        i = np.diff(i, prepend=np.int64(0))
    return np.ascontiguousarray(i.view(np.uint8).reshape(-1, 8).T)


def unpack(b, shape):
    i = np.ascontiguousarray(b.T).reshape(-1).view(np.int64)
    for _ in range(2):
        i = np.cumsum(i, dtype=np.int64)
    shape = tuple(shape)
    if len(shape) >= 2 and shape[-1] == 3:
        return np.ascontiguousarray(np.moveaxis(i.view(np.float64).reshape((3,) + shape[:-1]), 0, -1))
    return i.view(np.float64).reshape(shape)


def save(arrays, meta):
    """An npz whose bytes depend on the arrays alone (fixed member dates, sorted names); large float64 arrays packed"""
    with zipfile.ZipFile(NPZ, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key in sorted(arrays):
            a = np.ascontiguousarray(arrays[key])
            name = key
            if a.dtype == np.float64 and a.size >= PACK_FROM:
                meta["packed"][key] = list(a.shape)
                assert np.array_equal(unpack(pack(a), a.shape).view(np.uint64), a.view(np.uint64)), key
                a = pack(a)
            buf = io.BytesIO()
            np.lib.format.write_array(buf, a, allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    with open(JSON, "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")


_LOADED = []


def load():
    """(meta, arrays), loaded once and shared, read-only"""
    if not _LOADED:
        with open(JSON) as f:
            meta = json.load(f)
        z = np.load(NPZ)
        arrays = {}
        for key in z.files:
            a = z[key]
            if key in meta["packed"]:
                a = unpack(a, meta["packed"][key])
            a.setflags(write=False)
            arrays[key] = a
        _LOADED.extend([meta, arrays])
    return _LOADED[0], _LOADED[1]


def fields(arrays, name):
    """{field: array} of the keys `name__field`"""
    return {k[len(name) + 2:]: v for k, v in arrays.items() if k.startswith(name + "__")}


# ------------------------------------------------------------------------------------------------ inputs, by recipe
_INPUTS = {}


def fringe(period):
    key = ("fringe", period)
    if key not in _INPUTS:
        _INPUTS[key] = S.build_fringe(period, stripeColor="r")
        _INPUTS[key].setflags(write=False)
    return _INPUTS[key]


def frame(rig, period):
    """S.render of the rig: computed once per rig and shared, read-only"""
    key = ("frame", json.dumps(rig, sort_keys=True), period)
    if key not in _INPUTS:
        _INPUTS[key] = S.render(rig, period)
        _INPUTS[key].setflags(write=False)
    return _INPUTS[key]


def box(rig, roi):
    return (0, 0) + tuple(rig["res1"]) if roi is None else tuple(roi)


def unwrap_columns_first(phase):
    """The callable of the `unwrappingMethod=` cases: np.unwrap down the columns first, then along the rows -- the other order
    than the default's, so that a class that ignored the callable would be noticed"""
    return np.unwrap(np.unwrap(phase, axis=0), axis=1)


UNWRAPPERS = {"columns_first": unwrap_columns_first}


def stripe_image(recipe, rig, period):
    """The BGR image of a findCentralStripe case: the rendered frame with its channels permuted (the stripe lives in channel
    `recipe["channel"]`), the listed rows blanked; "blank": "all" is an image without stripe"""
    img = np.array(frame(rig, period))
    if recipe["blank"] == "all":
        return np.zeros_like(img)
    perm = {2: [0, 1, 2], 1: [0, 2, 1], 0: [2, 1, 0]}[recipe["channel"]]
    img = np.ascontiguousarray(img[:, :, perm])
    for r in recipe["blank"]:
        img[r] = 0
    return img


def graycode_stack(c):
    """uint8 [N, H, W] of a Gray-code case: G.scene from its seed"""
    r = c["rig"]
    return G.scene(c["seed"], tuple(r["res1"]), tuple(r["res2"]), noise=c["noise"], holes=c["holes"])


# ------------------------------------------------------------------------------------------------ the reference's roi shift
def mapping_with_inplace_shift(rig, fr, period, img, roi, radius_factor=0.5):
    """M.pipeline_mapping with the reference's fault emulated: its _triangulate adds the roi origin to the stripe in place
    (active.py:569-570), so map_coordinates (:1431) then samples the cut phase map at the shifted stripe"""
    pm = M.pipeline_mapping(rig, fr, period, img, roi, radius_factor)
    x0, y0 = box(rig, roi)[:2]
    theta = M.stripe_phase(pm["phase"], pm["stripe"] + np.array([x0, y0], dtype=np.float64))
    return dict(pm, theta_shift=theta, cloud=M.mapping_cloud(pm["geom"], pm["F"], pm["phase"], theta, pm["peak"], x0, y0))
