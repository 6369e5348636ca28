"""Pins of the OpenCV-backed plumbing that can only be checked where cv2 exists.

The reference computes its rectification maps, the remap and the 3-D reprojection with OpenCV
(reference simplestereo/_rigs.py:540-541, 564-565, 628).  cv2 is not installed in the build container nor on the GPU
boxes, so there these tests SKIP and f1 / f2 stay "parity unpinned" (DESIGN.md section 7); on any machine with cv2
they compare `simplestereo_amd._rigs` -- the numpy restatement the GPU kernels are tested against -- with cv2 itself,
and with tests/golden/cv2_pins.npz when tests/golden/make_golden_cv2.py has been run there."""
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)


def _pins():
    path = os.path.join(GOLDEN, "cv2_pins.npz")
    if os.path.exists(path):
        return dict(np.load(path))
    pytest.importorskip("cv2", reason="cv2 absent and tests/golden/cv2_pins.npz not generated: f1/f2 stay unpinned here")
    import make_golden_cv2
    return make_golden_cv2.with_cv2()


def test_rectification_maps_match_initUndistortRectifyMap():
    pins = _pins()
    import make_golden_cv2
    rig, _, _, _ = make_golden_cv2.inputs()
    for k, (mx, my) in {"1": (rig.mapx1, rig.mapy1), "2": (rig.mapx2, rig.mapy2)}.items():
        # float32 maps of a double pipeline: agreement to a few ulps of a pixel coordinate ~1e3
        assert np.abs(mx - pins["mapx" + k]).max() < 2e-3 and np.abs(my - pins["mapy" + k]).max() < 2e-3


def test_remap_matches_cv2_remap_on_cv2s_own_maps():
    pins = _pins()
    import make_golden_cv2
    from simplestereo_amd import _rigs
    _, img, img16, _ = make_golden_cv2.inputs()
    for k in ("1", "2"):
        mx, my = pins["mapx" + k], pins["mapy" + k]
        assert np.array_equal(_rigs._remap(img, mx, my, _rigs.INTER_LINEAR), pins["remap_linear" + k])       # fixed point: exact
        assert np.array_equal(_rigs._remap(img, mx, my, _rigs.INTER_NEAREST), pins["remap_nearest" + k])
        d16 = np.abs(_rigs._remap(img16, mx, my, _rigs.INTER_LINEAR).astype(np.int64) - pins["remap_linear_u16_" + k].astype(np.int64))
        assert d16.max() <= 1                                                                                  # float path: last-bit


def test_get3DPoints_matches_reprojectImageTo3D():
    pins = _pins()
    import make_golden_cv2
    rig, _, _, disp = make_golden_cv2.inputs()
    got = rig.get3DPoints(disp)
    want = pins["points"]
    ok = np.isfinite(want).all(-1)
    assert np.allclose(got[ok], want[ok], rtol=2e-6, atol=1e-6)


def test_remap_coordinates_outside_every_range_match_cv2():
    """NaN, +-inf, +-1e30, +-2^31, +-2^26 in mapx, mapy or both: the border value 0 (cvRound gives INT_MIN), and coordinates
    on the 1/64-pixel grid, where cvRound's half-to-even decides the 1/32 cell -- the cases of
    tests/test_gpu_rigs_limits.py and tests/test_rigs_cpu.py, against cv2.remap itself"""
    cv2 = pytest.importorskip("cv2", reason="cv2 absent: the out-of-range semantics stay pinned to the published arithmetic only")
    from simplestereo_amd import _rigs
    rng = np.random.default_rng(4)
    img = rng.integers(1, 256, (7, 8, 3)).astype(np.uint8)
    out = [np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 2.0 ** 26, -2.0 ** 26]
    mx = np.array([out + [2.25] * len(out) + out + [0.0] * len(out) + out], np.float32)
    my = np.array([[3.5] * len(out) + out + out + out + [0.0] * len(out)], np.float32)
    k = np.arange(-3 * 64, 10 * 64 + 1, dtype=np.float32) / np.float32(64)
    gx, gy = np.meshgrid(k[::3], k[::5])
    for ax, ay in ((mx, my), (np.ascontiguousarray(gx, np.float32), np.ascontiguousarray(gy, np.float32))):
        for ours, theirs in ((_rigs.INTER_LINEAR, cv2.INTER_LINEAR), (_rigs.INTER_NEAREST, cv2.INTER_NEAREST)):
            want = cv2.remap(img, ax, ay, theirs, borderMode=cv2.BORDER_CONSTANT, borderValue=0)
            with np.errstate(invalid="ignore"):
                assert np.array_equal(_rigs._remap(img, ax, ay, ours), want)
