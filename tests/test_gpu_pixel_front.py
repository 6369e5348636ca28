"""GPU tier: the pixel front of the matchers (csrc/lab_kernels.hip.h: load_bgr, lab_record, lab_records_pair) at the sizes
where its two reads differ.  Pixel p of a uint8 [n][3] image is one unaligned 4-byte read, except the image's LAST pixel,
which is three byte reads: a 1 x 1 image is nothing but that branch, 5 x 7 and 3 x 64 end on it after 34 and 191 pixels
of the other.  Every kernel that reads image bytes goes through it: the Lab records of StereoASW (one launch with the TAD volume,
or a launch of their own: SSAMD_ASW_PREPASS_FUSE 1 / 0), the TAD volume's pixels, the packed pixels of StereoGSW, ssamd_bgr2lab."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 2), (5, 7, 4), (3, 64, 9)]              # H, W, maxDisparity


def _pair(H, W):
    rng = np.random.default_rng(100 * H + W)
    L = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    R = np.ascontiguousarray(np.roll(L, -1, axis=1))
    R[..., 1] ^= rng.integers(0, 4, (H, W), dtype=np.uint8)
    return L, R


@pytest.mark.parametrize("H,W,maxd", SHAPES)
def test_the_pixel_front_on_images_that_end_on_the_byte_reads(H, W, maxd):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import simplestereo_amd as ss
    from oracle import oracle
    from simplestereo_amd import _native
    L, R = _pair(H, W)
    for img in (L, R):
        lab = np.empty((H, W, 3), np.float32)
        _native.check(_native.lib().ssamd_bgr2lab(img.ctypes.data, H, W, lab.ctypes.data, -1))
        want = oracle.bgr2lab(img).astype(np.float32)
        assert np.array_equal(lab.view(np.uint32), want.view(np.uint32)), (H, W, int(np.count_nonzero(lab != want)))
    for cons in (False, True):
        p = dict(winSize=5, maxDisparity=maxd, minDisparity=0, gammaC=5.0, gammaP=17.5, consistent=cons)
        ref = oracle.asw(L, R, **p)
        maps = {}
        for fuse in ("1", "0"):
            # (no autotuning: a call with trial launches writes its records first and never fuses)
            with _native.options(SSAMD_ASW_PREPASS_FUSE=fuse, SSAMD_AUTOTUNE="0"):
                maps[fuse] = ss.passive.StereoASW(**p).compute(L, R)
                assert _native.counter("exact_overflow") == 0
        assert np.array_equal(maps["1"], maps["0"]), (H, W, cons)
        assert np.array_equal(maps["1"], ref), (H, W, cons, int(np.count_nonzero(maps["1"] != ref)))
    g = dict(winSize=5, maxDisparity=maxd, minDisparity=0, gamma=10, fMax=120, iterations=3)
    assert np.array_equal(ss.passive.StereoGSW(**g).compute(L, R), oracle.gsw(L, R, **g)), (H, W)
