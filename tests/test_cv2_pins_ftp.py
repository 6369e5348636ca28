"""Pins of the cv2 calls of the reference's StereoFTP front end (active.py:478-490, :517, :535, :638) that can only be checked
where cv2 exists.  cv2 is not installed where this project is built and tested, so there these tests SKIP and the parts stay
"parity unpinned" (README, compatibility table); on any machine with cv2 they compare the numpy restatements the kernels are
tested against with cv2 itself."""
import numpy as np
import pytest

import _ftp_cloud_ref as C
import _stereo_ftp_ref as S

cv2 = pytest.importorskip("cv2", reason="cv2 absent: the bicubic table, cv2.undistort and the float32 places stay unpinned here")


def test_remap_cubic_matches_cv2_remap():
    """8-bit INTER_CUBIC is integer arithmetic on a fixed table: every byte equal -- this pins the table, and with it which
    entry takes the correction (recalled, not verified, where cv2 is absent)"""
    from simplestereo_amd import _rigs
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (37, 53), dtype=np.uint8)
    # every pair of fractions, cells inside and across the borders
    fy, fx = np.mgrid[0:32, 0:32]
    mx = (20 + fx / 32.0).astype(np.float32)
    my = (15 + fy / 32.0).astype(np.float32)
    assert np.array_equal(_rigs._remap(img, mx, my, _rigs.INTER_CUBIC), cv2.remap(img, mx, my, cv2.INTER_CUBIC))
    mx = rng.uniform(-6, 59, (64, 80)).astype(np.float32)
    my = rng.uniform(-6, 43, (64, 80)).astype(np.float32)
    want = cv2.remap(img, mx, my, cv2.INTER_CUBIC, borderMode=cv2.BORDER_CONSTANT, borderValue=0)
    assert np.array_equal(_rigs._remap(img, mx, my, _rigs.INTER_CUBIC), want)
    assert np.array_equal(S.remap_cubic(img, mx, my), want)


def test_undistort_matches_cv2_undistort():
    """cv2.undistort builds its maps strip by strip in fixed point: the bilinear remap on the float32 maps of
    initUndistortRectifyMap(K, D, I, K) is the same image to within one grey level"""
    import simplestereo_amd as ss
    rig = C.rig_params(res1=(160, 48))
    rig["distCoeffs1"] = [-0.08, 0.03, 0.0005, -0.0004, 0.0]
    frame = S.render(rig, 12.0)
    sf = ss.active.StereoFTP(C.make_rig(ss, rig), S.build_fringe(12.0, stripeColor="r"), 12.0)
    want = cv2.undistort(frame, np.array(rig["intrinsic1"]), np.array(rig["distCoeffs1"]))
    got = sf._undistort(frame)
    assert np.abs(got.astype(int) - want.astype(int)).max() <= 1


def test_float32_places_of_calculateCameraFrequency():
    """cv2.projectPoints and cv2.undistortPoints return float32 for float32 input (active.py:513-535): the two places where
    _calculateCameraFrequency rounds to float32"""
    rig = C.rig_params(res1=(160, 48))
    rg = S.Rig(rig, 12.0, 1280)
    obj = np.array([[3.0, -2.0, 1000.0], [-8.0, 5.0, 1012.5]]).reshape(-1, 1, 3).astype(np.float32)
    pCenter, _ = cv2.projectPoints(obj, rg.R, rg.T, rg.K2, np.array(rg.d2))
    assert pCenter.dtype == np.float32
    mine = S.project(obj.reshape(-1, 3).astype(np.float64), rg.R, rg.T, rg.K2, rg.d2).astype(np.float32)
    assert np.abs(pCenter.reshape(-1, 2) - mine).max() <= 2 * np.spacing(np.float32(1280))
    und = cv2.undistortPoints(pCenter.reshape(-1, 1, 2), rg.K2, np.array(rg.d2), P=rg.K2)
    assert und.dtype == np.float32
    mine = S.undistort_points(pCenter.reshape(-1, 2).astype(np.float64), rg.K2, rg.d2, rg.K2).astype(np.float32)
    assert np.abs(und.reshape(-1, 2) - mine).max() <= 2 * np.spacing(np.float32(1280))
