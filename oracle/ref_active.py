"""Loads the reference's own Python modules (simplestereo/utils.py, rectification.py, _rigs.py, active.py) from where they lie,
with a stand-in for cv2, so that tests/golden/make_golden_active_ref.py can record what the reference's code computes.

What this pins and what it does not
-----------------------------------
Pinned, bit for bit: the reference's own numpy, scipy and control flow -- the dtypes it builds its matrices in, the order
of its steps, the in-place edits, the exceptions -- everything between two cv2 calls.

Not pinned: the cv2 calls themselves.  cv2 is not installed where this project is built, so every cv2 function the exercised
paths touch is answered by the numpy restatement of OpenCV's published arithmetic that the tests already use
(tests/_stereo_ftp_ref.py, tests/_graycode_ref.py).  Those stay "unpinned against cv2" exactly as the README says;
tests/test_cv2_pins_*.py pin them wherever cv2 exists.  A golden recorded through this loader therefore proves that the
restatements and the kernels follow the reference's code GIVEN those cv2 restatements, and nothing about cv2.

Process rule
------------
load() puts the stand-in into sys.modules["cv2"].  It is for the golden-maker process only: no test imports this file, since a
fake cv2 inside a pytest process would turn the importorskip("cv2") pins into tests of the stand-in against itself.

No program text of the reference is copied: load() imports the files where they lie and returns None when they are absent."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.join(os.path.dirname(HERE), "tests")
REFERENCE = os.environ.get("SSAMD_REFERENCE", "/root/reference")
SUBMODULES = ("utils", "rectification", "_rigs", "active")


def _restatements():
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import _graycode_ref as G
    import _stereo_ftp_ref as S
    return S, G


def _coeffs(d):
    return [] if d is None else [float(v) for v in np.asarray(d, dtype=np.float64).ravel()]


def make_cv2():
    """The cv2 stand-in: a types.ModuleType holding only what the exercised paths of the four modules touch."""
    S, G = _restatements()
    cv2 = types.ModuleType("cv2")
    cv2.__doc__ = "stand-in for cv2: numpy restatements of the calls simplestereo's active half makes (oracle/ref_active.py)"
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.INTER_CUBIC = 0, 1, 2
    cv2.CV_32FC1 = 5
    cv2.IMREAD_GRAYSCALE = 0
    cv2.Mat = np.ndarray
    cv2.files = {}                                   # name -> uint8 array: what imread "reads"

    def undistort(img, K, d, dst=None, newCameraMatrix=None):
        if dst is not None or newCameraMatrix is not None:
            raise NotImplementedError("cv2 stand-in: undistort with a new camera matrix")
        img = np.asarray(img)
        if img.dtype != np.uint8:
            raise NotImplementedError("cv2 stand-in: undistort of uint8 images only")
        K = np.asarray(K, dtype=np.float64)
        mx, my = S.undistort_maps(K, _coeffs(d), (img.shape[1], img.shape[0]))
        if img.ndim == 2:
            return G.remap_stack(img[None], mx, my)[0]
        if img.ndim == 3 and img.shape[2] == 3:
            return S.remap_linear(img, mx, my)
        raise NotImplementedError("cv2 stand-in: undistort of [H, W] or [H, W, 3] images only")

    def projectPoints(objectPoints, rvec, tvec, cameraMatrix, distCoeffs):
        pts = np.asarray(objectPoints)
        R = np.asarray(rvec, dtype=np.float64)
        if R.shape != (3, 3):
            raise NotImplementedError("cv2 stand-in: projectPoints takes the 3x3 matrix only (no Rodrigues vector)")
        out = S.project(pts.reshape(-1, 3).astype(np.float64), R, np.asarray(tvec, dtype=np.float64).reshape(3),
                        np.asarray(cameraMatrix, dtype=np.float64), _coeffs(distCoeffs))
        return out.reshape(-1, 1, 2).astype(pts.dtype), None

    def undistortPoints(src, cameraMatrix, distCoeffs, dst=None, R=None, P=None):
        pts = np.asarray(src)
        Rm = None
        if R is not None or P is not None:
            Rm = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
            if P is not None:
                Rm = np.asarray(P, dtype=np.float64)[:3, :3].dot(Rm) if R is not None else np.asarray(P, dtype=np.float64)[:3, :3]
        out = S.undistort_points(pts.reshape(-1, 2).astype(np.float64), np.asarray(cameraMatrix, dtype=np.float64), _coeffs(distCoeffs), Rm)
        return out.reshape(-1, 1, 2).astype(pts.dtype)

    def perspectiveTransform(src, m):
        pts = np.asarray(src)
        m = np.asarray(m, dtype=np.float64)
        n = pts.shape[-1]
        if m.shape != (n + 1, n + 1) or n not in (2, 3):
            raise NotImplementedError("cv2 stand-in: perspectiveTransform of 2-D points with 3x3 or 3-D points with 4x4")
        flat = pts.reshape(-1, n).astype(np.float64)
        if n == 2:
            out = S.perspective(flat, m)
        elif np.array_equal(m[3], [0, 0, 0, 1]) and not m[:3, 3].any():
            out = flat.dot(m[:3, :3].T)               # w = 1 exactly: the rotation alone
        else:
            q = np.hstack((flat, np.ones((flat.shape[0], 1)))).dot(m.T)
            out = q[:, :3] / q[:, 3:]
        return out.reshape(pts.shape).astype(pts.dtype)

    def remap(src, map1, map2, interpolation, *a, **kw):
        if a or kw:
            raise NotImplementedError("cv2 stand-in: remap with the default constant border 0 only")
        src = np.asarray(src)
        if src.dtype != np.uint8:
            raise NotImplementedError("cv2 stand-in: remap of uint8 images only")
        if interpolation == cv2.INTER_CUBIC and src.ndim == 2:
            return S.remap_cubic(src, map1, map2)
        if interpolation == cv2.INTER_LINEAR:
            return G.remap_stack(src[None], map1, map2)[0] if src.ndim == 2 else S.remap_linear(src, map1, map2)
        raise NotImplementedError("cv2 stand-in: remap with INTER_CUBIC (gray) or INTER_LINEAR")

    def imread(filename, flags=None):
        img = cv2.files.get(filename)
        return None if img is None else np.array(img)

    def imwrite(filename, img):
        from PIL import Image
        Image.fromarray(np.asarray(img)).save(filename)
        return True

    class structured_light_GrayCodePattern:
        def __init__(self, width, height):
            self.width, self.height = int(width), int(height)
            self.black_thr, self.white_thr = 40, 5

        @staticmethod
        def create(width, height):
            return structured_light_GrayCodePattern(width, height)

        def setBlackThreshold(self, v):
            self.black_thr = v

        def setWhiteThreshold(self, v):
            self.white_thr = v

        def getNumberOfPatternImages(self):
            return G.num_patterns(self.width, self.height)

        def generate(self):
            return True, [np.array(p) for p in G.pattern(self.width, self.height)]

        def getProjPixel(self, patternImages, x, y):
            return G.get_proj_pixel(patternImages, x, y, self.width, self.height, self.white_thr)

    for f in (undistort, projectPoints, undistortPoints, perspectiveTransform, remap, imread, imwrite):
        setattr(cv2, f.__name__, f)
    cv2.structured_light_GrayCodePattern = structured_light_GrayCodePattern
    return cv2


def load(reference=None):
    """-> the reference's package (a stub module whose submodules utils, rectification, _rigs and active are the reference's
    files, executed from where they lie; StereoRig and RectifiedStereoRig as its __init__ would export them), or None when the
    reference is absent.  The package's __init__.py is not executed (it asks pkg_resources for an installed distribution), and
    the `matplotlib.use('TkAgg')` of active.py selects Agg while the import runs."""
    root = os.path.join(reference or REFERENCE, "simplestereo")
    if not os.path.isfile(os.path.join(root, "active.py")):
        return None
    if "simplestereo" in sys.modules:
        return sys.modules["simplestereo"]
    sys.modules["cv2"] = make_cv2()
    pkg = types.ModuleType("simplestereo")
    pkg.__path__ = [root]
    pkg.__package__ = "simplestereo"
    sys.modules["simplestereo"] = pkg
    import matplotlib
    use = matplotlib.use
    matplotlib.use = lambda backend, **kw: use("Agg", **kw)
    dont_write = sys.dont_write_bytecode
    sys.dont_write_bytecode = True                   # leave the reference tree as it is
    try:
        for name in SUBMODULES:
            setattr(pkg, name, importlib.import_module("simplestereo." + name))
    finally:
        matplotlib.use = use
        sys.dont_write_bytecode = dont_write
    pkg.StereoRig, pkg.RectifiedStereoRig = pkg._rigs.StereoRig, pkg._rigs.RectifiedStereoRig
    pkg.cv2 = sys.modules["cv2"]
    return pkg
