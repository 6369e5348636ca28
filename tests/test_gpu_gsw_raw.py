"""GPU tier: the RAW winners of GSW.  ``StereoGSW`` always ends with the left-right check and the occlusion filling, and
every other GSW test compares only the filled map: a wrong winner that the check invalidates and the filling paints over is
invisible there.  ``ssamd_gsw_argmins`` dumps both winner images before that step; here they are held, pixel for pixel and
with no exclusion, to the oracle's literal restatement of the reference's loops (``oracle.gsw(closed=False, return_raw=True)``,
itself held to maps recorded from the reference at the same parameter edges by tests/test_oracle_golden_gsw_edges.py), and
the filled map of ``StereoGSW.compute`` to the oracle's.

Conventions of both dumps: ``left[y, x]`` = x - dBest of the left-referenced pass (x when the candidate loop is empty or
nothing won), ``right[y, x]`` = dBest of the right-referenced pass (0 when nothing won).

Where an edge is the point of a case, the test first shows on the CPU that its input reaches the edge and prints the count."""

import numpy as np
import pytest

import _gsw_edges as edges
from simplestereo_amd import _native

pytestmark = pytest.mark.gpu

_ORACLE = {}      # (input key, parameters) -> (map, left, right) of the literal oracle: computed once, never written to


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import simplestereo_amd
    return simplestereo_amd


def _key(p):
    return tuple(sorted((k, repr(v)) for k, v in p.items()))


def oracle_raw(name, a, b, p):
    from oracle import oracle
    k = (name, _key(p))
    if k not in _ORACLE:
        got = oracle.gsw(a, b, closed=False, return_raw=True, **p)
        for g in got:
            g.setflags(write=False)
        _ORACLE[k] = got
    return _ORACLE[k]


def gpu_raw(a, b, p):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    H, W = a.shape[:2]
    left, right = np.full((H, W), -7, np.int16), np.full((H, W), -7, np.int16)
    _native.check(_native.lib().ssamd_gsw_argmins(a.ctypes.data, b.ctypes.data, H, W, p["winSize"], p["maxDisparity"], p["minDisparity"],
                                                  p["gamma"], p["fMax"], p["iterations"], p.get("bins", 20), left.ctypes.data,
                                                  right.ctypes.data, -1))
    return left, right


def check(ss, name, a, b, p, tag=""):
    """raw left, raw right and the filled map against the literal oracle: every pixel, np.array_equal"""
    want, want_left, want_right = oracle_raw(name, a, b, p)
    left, right = gpu_raw(a, b, p)
    filled = ss.passive.StereoGSW(**p).compute(a, b)
    print("%s %s %s: raw left %d, raw right %d, filled %d of %d pixels differ" % (
        name, tag, {k: v for k, v in p.items() if k != "bins"}, int((left != want_left).sum()), int((right != want_right).sum()),
        int((filled != want).sum()), want.size))
    assert left.dtype == np.int16 and left.shape == want_left.shape
    assert np.array_equal(left, want_left)
    assert np.array_equal(right, want_right)
    assert filled.dtype == np.int16 and np.array_equal(filled, want)
    return left, right, filled


def P(**kw):
    p = dict(winSize=11, maxDisparity=16, minDisparity=0, gamma=10, fMax=120.0, iterations=3, bins=20)
    p.update(kw)
    return p


def noise_pair(h, w, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w, 3), dtype=np.uint8), rng.integers(0, 256, (h, w, 3), dtype=np.uint8)


def synth_pair(h, w, maxd, seed):
    from simplestereo_amd.synth import make_pair
    return make_pair(h, w, maxd, seed)[:2]


# ------------------------------------------------------------------------------------------------ borders and quirks
_BORDERS = [((1, 40), P(winSize=7, maxDisparity=12)), ((2, 40), P(winSize=7, maxDisparity=12)),
            ((12, 33), P(winSize=21, maxDisparity=12)), ((9, 7), P(winSize=21, maxDisparity=30)),
            ((9, 12), P(winSize=21, maxDisparity=30)), ((20, 64), P(winSize=9, maxDisparity=20, minDisparity=1))]


@pytest.mark.parametrize("gamma", [10, -7])
@pytest.mark.parametrize("shape,p", _BORDERS, ids=["%dx%d" % s for s, _ in _BORDERS])
def test_borders_and_the_left_pass_break_quirk(shape, p, gamma, ss):
    """window and disparity range wider than the image, one- and two-row images (image row 0 keeps the centre row of its
    weights where the window sticks out on the right: the whole image is the call, so y == 0 is the absolute row), and the
    columns W - pad .. W - 1 where the left pass's `break` leaves only the centre"""
    H, W = shape
    p = dict(p, gamma=gamma)
    pad = p["winSize"] // 2
    a, b = synth_pair(H, W, max(p["maxDisparity"], 4), 11 + H + W)
    first = max(0, W - pad)
    print("%dx%d win %d: %d clipped left-pass windows (columns %d..%d), %d of them on image row 0" % (
        H, W, p["winSize"], H * (W - first), first, W - 1, W - first))
    assert W - first >= 1
    left, _, _ = check(ss, "border_%dx%d" % shape, a, b, p)
    want_left = oracle_raw("border_%dx%d" % shape, a, b, p)[1]
    assert left[:, first:].size == H * (W - first) and np.array_equal(left[:, first:], want_left[:, first:])
    assert np.array_equal(left[0], want_left[0])


# ------------------------------------------------------------------------------------------------ tile forms
_GEOMS = ["8,4,1", "16,2,1", "3,7,2", "5,3,2,2", "5,3,2,4", "6,7,2,8", "2,1,1", "2,1,2"]
_TILE_PARAMS = [P(winSize=11, maxDisparity=70), P(winSize=11, maxDisparity=41, minDisparity=5)]


@pytest.mark.parametrize("geom", _GEOMS)
def test_tile_forms_raw_winners(geom, ss):
    """every tile shape and strip height of the tiled kernel: W = 90 is a multiple of no tile width used, 37 rows leave a
    part-filled last strip for every Ty * Hy > 1; the two one-slot forms run one slot of disparities per chunk, so the winners
    merge across many chunks by the global atomicMin; widths 1, 2, 3, 5 are narrower than one thread's four columns"""
    a, b = synth_pair(37, 90, 70, 1)
    with _native.options(SSAMD_GSW_GEOM=geom):
        for p in _TILE_PARAMS:
            g = _native.gsw_geometry(90, 37, p["winSize"], p["maxDisparity"], p["minDisparity"])
            print(geom, g)
            assert 90 % g["tile_x"] != 0 and (g["strip_rows"] == 1 or 37 % g["strip_rows"] != 0)
            if geom in ("2,1,1", "2,1,2"):
                assert g["n_chunks"] >= 3 and g["chunk_d"] in (4, 8)
            check(ss, "tile_37x90", a, b, p, geom)
        for w in (1, 2, 3, 5):
            na, nb = synth_pair(6, w, 4, 30 + w)
            check(ss, "narrow_6x%d" % w, na, nb, P(winSize=5, maxDisparity=3), geom)


# ------------------------------------------------------------------------------------------------ subnormal support weights
def _weight_table(gamma):
    s = np.arange(3 * 255 * 255 + 1, dtype=np.float64)
    dist = np.sqrt(s).astype(np.float32)
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(-dist.astype(np.float64) / gamma).astype(np.float32)


def _window_pair_distances(img, win):
    """s = |BGR(cell) - BGR(centre)|^2 of every (centre, in-image window cell) pair"""
    pad = win // 2
    H, W = img.shape[:2]
    v = img.astype(np.int64)
    out = []
    for dy in range(-pad, pad + 1):
        for dx in range(-pad, pad + 1):
            y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
            d = v[y0:y1, x0:x1] - v[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
            out.append((d * d).sum(-1).ravel())
    return np.concatenate(out)


@pytest.mark.parametrize("gamma", [1, 4])
def test_subnormal_support_weights(gamma, ss):
    """the table entries between 2^-149 and 2^-126 (s = 7628 .. 10810 for gamma = 1, 122043 .. 172963 for gamma = 4):
    products and sums of subnormal floats must not be flushed to zero.  (Seed: uniform noise rarely reaches colour distances
    beyond 349, which gamma = 4 needs; of the seeds 1 .. 300 only 90 and 248 give 100 such pairs at this size.)"""
    a, b = noise_pair(16, 40, 248)
    tab = _weight_table(gamma)
    tiny = np.float32(2.0 ** -126)
    n = sum(int(((tab[s] > 0) & (tab[s] < tiny)).sum()) for s in (_window_pair_distances(a, 7), _window_pair_distances(b, 7)))
    print("gamma %d: %d window pairs with a positive subnormal support weight" % (gamma, n))
    assert n >= 100
    check(ss, "noise_16x40_s248", a, b, P(winSize=7, maxDisparity=9, gamma=gamma, fMax=1000.0))


# ------------------------------------------------------------------------------------------------ parameter edges
@pytest.fixture(scope="module")
def recorded():
    return edges.recorded_maps()


@pytest.mark.parametrize("cid", edges.CASE_IDS)
def test_parameter_edges_raw_and_filled(cid, ss, recorded):
    """every recorded parameter set on both of its inputs: raw winners and filled map against the oracle, and the filled map
    against what the reference itself returned"""
    a, b = edges.pair(cid)
    _, _, filled = check(ss, edges.META[cid]["input"], a, b, edges.params(cid), cid)
    assert np.array_equal(filled, recorded[cid])


# ------------------------------------------------------------------------------------------------ negative gamma beyond G9f
_G9F = P(winSize=5, maxDisparity=9, minDisparity=2, gamma=-7)


def _negative_gamma_inputs(golden_inputs):
    return {"crop": golden_inputs("crop"), "synth_40x64": synth_pair(40, 64, 12, 3), "noise_24x48": noise_pair(24, 48, 24)}


@pytest.mark.parametrize("name", ["crop", "synth_40x64", "noise_24x48"])
def test_negative_gamma_unreached_cells_disqualify_candidates(name, ss, golden_inputs):
    """gamma < 0: a window cell the relaxation never reaches ends at exp(+inf) = inf, and one tapped inf weight makes the
    candidate's cost inf or NaN.  In the left pass at x >= W - pad every non-centre cell is such a cell, so nothing wins there:
    with minDisparity = 2 a winner would give a disparity in 2 .. 9, `x` can only be the "nothing won" value."""
    a, b = _negative_gamma_inputs(golden_inputs)[name]
    W, pad = a.shape[1], _G9F["winSize"] // 2
    want_left = oracle_raw(name, a, b, _G9F)[1]
    border = want_left[:, W - pad:]
    nothing = int((border == np.arange(W - pad, W)[None, :]).sum())
    print("%s: the oracle's left pass wins nothing at %d of %d pixels of columns %d..%d" % (name, nothing, border.size, W - pad, W - 1))
    assert W - pad > _G9F["maxDisparity"] and nothing >= 1
    check(ss, name, a, b, _G9F)


# ------------------------------------------------------------------------------------------------ the plain kernel
def _plain_calls():
    return _native.counter("gsw_plain_calls")


@pytest.mark.parametrize("shape,p", [((96, 128), P(winSize=11, maxDisparity=40)), ((64, 96), P(winSize=7, maxDisparity=24, minDisparity=3))],
                         ids=["96x128", "64x96"])
def test_tiled_and_plain_kernels_agree_on_raw_winners(shape, p, ss):
    """SSAMD_GSW_PLAIN: the reference's loops one thread per pixel, a second standard on the device that needs no CPU oracle"""
    a, b = synth_pair(shape[0], shape[1], p["maxDisparity"], 9)
    n0 = _plain_calls()
    left, right = gpu_raw(a, b, p)
    assert _plain_calls() == n0
    with _native.options(SSAMD_GSW_PLAIN=1):
        pleft, pright = gpu_raw(a, b, p)
        pfilled = ss.passive.StereoGSW(**p).compute(a, b)
    assert _plain_calls() == n0 + 2
    print("%dx%d: tiled and plain raw winners differ at %d (left) and %d (right) pixels" % (
        shape[0], shape[1], int((left != pleft).sum()), int((right != pright).sum())))
    assert np.array_equal(left, pleft) and np.array_equal(right, pright)
    assert np.array_equal(ss.passive.StereoGSW(**p).compute(a, b), pfilled)
    assert left.max() <= max(p["maxDisparity"], shape[1] - 1) and (right <= shape[1] - 1).all()


def test_which_parameters_take_the_plain_kernel(ss):
    """a default-parameter call launches the tiled kernel (one timed launch in the aggregation's profile slot) and never the
    plain one; gamma < 0, fMax < 0 and a NaN fMax take the plain kernel, which is not timed in that slot"""
    lib = _native.lib()
    a, b = synth_pair(24, 64, 16, 2)

    def launches(**kw):
        lib.ssamd_profile_reset()
        n0 = _plain_calls()
        ss.passive.StereoGSW(**kw).compute(a, b)
        return _native.profile_read()[1][_native.K_GSW_AGG], _plain_calls() - n0

    lib.ssamd_profile_enable(1)
    try:
        assert launches() == (1, 0)
        assert launches(gamma=1, fMax=0.0) == (1, 0)
        assert launches(fMax=float("inf")) == (1, 0)
        assert launches(fMax=-0.0) == (1, 0)
        assert launches(gamma=-7) == (0, 1)
        assert launches(fMax=-5.0) == (0, 1)
        assert launches(fMax=float("nan")) == (0, 1)
        with _native.options(SSAMD_GSW_PLAIN=1):
            assert launches() == (0, 1)
        assert launches() == (1, 0)
    finally:
        lib.ssamd_profile_enable(0)
        lib.ssamd_profile_reset()
    assert "gsw_aggregate_kernel" in lib.ssamd_kernel_name(_native.K_GSW_AGG).decode()
