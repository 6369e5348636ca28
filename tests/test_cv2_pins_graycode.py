"""Pins of cv2.structured_light_GrayCodePattern (the reference's generateGrayCodeImgs and GrayCode, active.py:46-51, :1163-1166,
:1223) that can only be checked where OpenCV's contrib module exists.  cv2 is not installed where this project is built and
tested, so there these tests SKIP and Gray code stays "parity unpinned" (README, compatibility table); on any machine with
cv2.structured_light they compare the numpy restatement the kernels are tested against with cv2 itself."""
import numpy as np
import pytest

import _graycode_ref as G

cv2 = pytest.importorskip("cv2", reason="cv2 absent: GrayCodePattern stays unpinned here")
if not hasattr(cv2, "structured_light_GrayCodePattern"):
    pytest.skip("cv2 without the structured_light module: GrayCodePattern stays unpinned here", allow_module_level=True)


@pytest.mark.parametrize("res", [(2, 1), (5, 3), (13, 6), (320, 200), (1024, 768), (1280, 720), (1920, 1080)])
def test_number_of_pattern_images(res):
    gc = cv2.structured_light_GrayCodePattern.create(*res)
    assert gc.getNumberOfPatternImages() == G.num_patterns(*res)


@pytest.mark.parametrize("res", [(5, 3), (13, 6), (320, 200)])
def test_generate(res):
    import simplestereo_amd as ss
    ok, imgs = cv2.structured_light_GrayCodePattern.create(*res).generate()
    assert ok
    want = np.stack(imgs)
    assert np.array_equal(G.pattern(*res), want) and np.array_equal(ss.active.grayCodePattern(res), want)


@pytest.mark.parametrize("thr", [0, 1, 5, 40])
def test_get_proj_pixel(thr):
    res = (13, 6)
    gc = cv2.structured_light_GrayCodePattern.create(*res)
    gc.setWhiteThreshold(thr)
    stack = G.random_stack(41, 14, 7, 9)
    rng = np.random.default_rng(42)
    stack[:, :, 5:] = G.render(rng.integers(0, 16, (7, 4)), rng.integers(0, 8, (7, 4)), 13, 6, rng.integers(0, 8, (7, 7, 4)))
    want = G.decode(stack, 13, 6, thr)
    imgs = [np.ascontiguousarray(p) for p in stack]
    for y in range(7):
        for x in range(9):
            err, pix = gc.getProjPixel(imgs, x, y)
            assert tuple(want[y, x]) == ((-1, -1) if err else tuple(pix)), (x, y)
