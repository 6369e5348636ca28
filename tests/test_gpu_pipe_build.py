"""Tier T2 (GPU): the support-weight build of asw_aggregate_pipe_kernel (whole waves of left or of right window centres,
proximity weights by scalar loads from the window's table, batches of four plus a straight-line remainder) against the
round-1 workgroup kernel on the same tile and the same tap-column chunks.

Both kernels evaluate every weight with the same expression and add the same taps in the same order, so the fp32 argmin
map and the raw cost volume must be equal BIT FOR BIT: there is no tolerance in this file.  The shapes are the smallest
that take every path of the build: two full tiles and a partial one, a left-border tile whose threads are dealt over fewer
disparity groups, windows clipped at the first and last rows, chunk lengths with remainders 0, 1 and 3, tiles with fewer
and with more centre-waves than waves.  Inputs: colours drawn uniformly from 0..255 (textured), two constant images (every
colour distance is 0: a weight is its proximity term alone), and a constant left image against a textured right one (the
left weights are proximity terms alone while the matching costs still vary)."""
import numpy as np
import pytest
from simplestereo_amd import _native

import _asw_forms as F

pytestmark = pytest.mark.gpu

# name -> tile (_asw_forms.PIPE_TILES: 8 XG columns x 4 DG disparities, tap-column chunks), H, W, win, minD, maxD, consistent
CASES = {
    "120x196": ("120x196", 40, 250, 35, 0, 192, False),           # chunks 16 + 19
    "120x196-win33": ("120x196", 40, 250, 33, 0, 192, False),     # chunks 16 + 17: remainder 1
    "120x196-minD3": ("120x196", 40, 250, 35, 3, 195, False),
    "216x68": ("216x68", 24, 450, 35, 0, 64, False),              # 9 centre-waves on 8 waves
    "88x260": ("88x260", 24, 180, 35, 0, 256, False),
    "generic-8-8-8-11": ("48x36", 24, 100, 35, 0, 35, True),      # 3 centre-waves on one wave, chunks 8, 8, 8, 11
}
# static = 1: the library's default, which picks the instantiation with compile-time strides whenever the planned strides equal
# one of its tiles' (120 / 316 / 208, 88 / 348 / 272, 216 / 284 / 80: the first five cases; the test asserts the tile, the host
# then has no other choice); static = 0 forces the generic instantiation on the same tile.  No static tile has the strides of
# the last case, so it runs the generic instantiation either way and is listed once.
PARAMS = [(name, static) for name in CASES for static in (1, 0) if not (name.startswith("generic") and static == 0)]


def _forms(name, static):
    """the two sides of a case as (form, W, H, params): the phase-shifted kernel, and the round-1 kernel on the same tile and chunks"""
    tile, H, W, win, mind, maxd, cons = CASES[name]
    XG, DG, JC = F.PIPE_TILES[tile]
    p = dict(winSize=win, maxDisparity=maxd, minDisparity=mind, gammaC=5.0, gammaP=17.5)
    return ((F.also(F.pipe_tile(XG, DG, JC, static=static), n_chunks=1), W, H, p),
            (F.workgroup_tile("%d,%d,%d,8" % (XG, DG, JC), win=win, SSAMD_ASW_STATIC=str(static)), W, H, p))


def forced_rows():
    return [row for name, static in PARAMS for row in _forms(name, static)]


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import simplestereo_amd
    assert _native.lib().ssamd_device_count() >= 1
    return simplestereo_amd


def _images(H, W, seed):
    rng = np.random.default_rng(seed)
    tex = lambda: rng.integers(0, 256, (H, W, 3), dtype=np.uint8)                                   # noqa: E731
    const = lambda: np.ascontiguousarray(np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (H, W, 3)))   # noqa: E731
    return [("textured", tex(), tex()), ("constant", const(), const()), ("constant-left", const(), tex())]


@pytest.mark.parametrize("name,static", PARAMS)
def test_pipe_build_equals_the_round1_kernel(name, static, ss):
    pipe, round1 = _forms(name, static)
    _, W, H, p = pipe
    m = ss.passive.StereoASW(consistent=CASES[name][-1], exact=False, **p)
    for label, L, R in _images(H, W, 11):
        with F.forced(*pipe):
            got, got_c = m.compute(L, R), F.cost_dump(L, R, p)
        with F.forced(*round1):
            want, want_c = m.compute(L, R), F.cost_dump(L, R, p)
        assert np.array_equal(got, want), (name, static, label, int((got != want).sum()))
        assert F.same_costs(got_c, want_c) == 0, (name, static, label, F.same_costs(got_c, want_c))
