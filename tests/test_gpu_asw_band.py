"""GPU tier: the fp32 cost images of every ASW aggregation kernel form, measured against the near-tie band they are trusted to
stay inside (asw_exact_prepare's `tol`, mirrored by _tie_inputs.tol).

The default StereoASW path returns the fp64 reference's map because every candidate whose fp32 cost image lies within `tol` of
the fp32 winner's is decided again in fp64.  That holds exactly as long as the kernels' error, taken as a DIFFERENCE between the
reference's winner and any other candidate of the pixel, stays within `tol` (tests/_asw_band_ref.py has the argument).  The map
tests cannot tell how near the kernels come to it; here the images themselves are read (test hook SSAMD_ASW_COST_KEYS: the cost
dump of ssamd_asw_costs holds the 32-bit images of asw_cost_key instead of the float costs) and compared with the image of the
oracle's fp64 costs, on the case matrix of tests/golden/asw_band_cases.json -- the corners of the band's scaling rule, every
kernel family.

The dump runs the cost-WRITING instantiations of the kernels (asw_pick_pipe_kernel(g, true, ...), asw_pick_wave_kernel(g, true,
...), asw_aggregate_kernel<true, ...>), not the ones a StereoASW call runs.  Their winners are held equal to the production
instantiations' by tests/test_gpu_pipe_build.py and the form-equality tests of tests/test_gpu_asw.py.

Printed per case and form (pytest -s): E max and its 99.9th percentile, the emulation's E max, D max, tol and D max / tol, the
share of the band in use; per canary band the pixels that leave the oracle's map.  profiles/exact_band_margin.txt is one run."""
import json
import os

import numpy as np
import pytest

import _asw_band_ref as B
import _asw_forms as F
import _tie_inputs as T

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(G, "asw_band_cases.json")) as _f:
    FIXTURE = json.load(_f)
OC = T.OracleCache()


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import simplestereo_amd
    return simplestereo_amd


@pytest.mark.parametrize("name", sorted(B.CASES))
def test_cost_images_against_the_band(name, ss):
    """Per candidate (cost <= 39, both images on one side of 20): E = |image32 - image64| <= 2 x max(the emulation's E max, 8).
    The emulation (tests/_asw_band_ref.py::emulate32) adds the same fp32 terms one by one in raster order; the factor 2 is for
    the kernels' other order and their fused multiply-adds.  The same bar holds over the candidates above rule (d)'s floor
    (fp64 image > zkey) against the emulation's E max over those.

    Differential, over the near pairs (d*, c): D = (image32(d*) - image32(c)) - (image64(d*) - image64(c)) <= tol for every
    pair of the band class (image32(d*) > zkey), in every case; cases with differential = true in the fixture have 200 of
    them.  The others (windows of 3 and 9 at large gammaC, the noisy low-contrast frames, the flush cases) have next to none.
    Last, the guarantee itself on these inputs: the reference's winner lies within tol of the fp32 winner, or at or below zkey.
    Forms that run the same case return the same images word for word.

    Measured on an MI355X (profiles/exact_band_margin.txt): the kernels' E max is the emulation's to within 2 ulps in every case;
    the largest share of the band in use is 0.34 (D max 43 of 128, window 21, gammaC 5, gammaP 100), 0.18 at the bench's
    parameters.  The three flush cases (gammaC 0.7, perturbed patches) hold candidates whose fp64 cost is below 1e-37, made of
    weights that v_exp_f32 returns as 0: there E reaches 1.3e7 ... 3.2e7 ulps and D 6 645 ... 9 683 (tol 914), in the kernels
    and -- once it flushes an exp2 below 2^-126 as the instruction does -- in the emulation alike, to the ulp.  Every one of
    those winners lies below zkey (the largest such cost is 8.5e-38, Z = 4.1e-34 at that window): rule (d) queues them, no band
    counted in ulps could, and so their pairs form the floor class, whose D is printed and not held to tol."""
    case, fx = B.CASES[name], FIXTURE[name]
    L, R, p = B.case_inputs(name)
    _, cost = OC.asw(L, R, return_costs=True, **p)
    tol, zk = B.case_tol(name), B.zkey(p["winSize"])
    assert tol == fx["tol"] and zk == fx["zkey"]
    bar, bar_above = 2 * max(fx["emu_E_max"], B.E_FLOOR), 2 * max(fx["emu_E_max_above_zkey"], B.E_FLOOR)
    i64 = B.image64(cost)
    ds = B.first_minimum(cost)[..., None]
    H, W = L.shape[:2]
    first = None
    for form in case["forms"]:
        with F.forced(form, W, H, p):
            i32, c = B.image32(F.cost_dump(L, R, p, keys=True)), F.cost_dump(L, R, p) if first is None else None
        assert np.array_equal(i32 < 0, np.isnan(cost)), (name, form, "candidates that exist")
        if first is None:
            first = (form, i32)
            # the hook changes what is written, nothing else: the float dump is the image's cost
            ok = i32 >= 0
            with np.errstate(invalid="ignore"):
                low = np.where(ok, i32, 0).astype(np.uint32).view(np.float32)
                high = np.float32(40) - (0xC0000000 - np.where(i32 >= B.HIGH, i32, 0xC0000000)).astype(np.uint32).view(np.float32)
            assert np.array_equal(c[ok], np.where(i32 >= B.HIGH, high, low)[ok]), (name, form, "float dump")
            assert np.all(np.isnan(c[~ok]))
        else:
            assert np.array_equal(i32, first[1]), (name, form, first[0], int(np.count_nonzero(i32 != first[1])))
        e_max, e_p999, n = B.candidate_error(cost, i32)
        a_max, a_p999, a_n = B.candidate_error(cost, i32, above=zk)
        d_max, pairs, f_max, f_pairs = B.differential_error(cost, i32, tol, zk)
        print("BAND %-15s %-11s win %3d gC %4g gP %5g | measured %7d  E max %8d  p99.9 %10.1f  emulation %8d | above zkey %7d  "
              "E max %4d  p99.9 %6.1f  emulation %4d | band pairs %5d  D max %4d  tol %4d  share %.3f | floor pairs %4d  D max %5d" %
              (name, form, p["winSize"], p["gammaC"], p["gammaP"], n, e_max, e_p999, fx["emu_E_max"], a_n, a_max, a_p999,
               fx["emu_E_max_above_zkey"], pairs, d_max, tol, d_max / tol, f_pairs, f_max))
        assert n >= 0.999 * fx["measured"], (name, form, n)                            # (all but candidates on the seam at 20)
        # a candidate whose two images lie either side of 20 is not measured: it must be within the bar of the seam
        with np.errstate(invalid="ignore"):
            seam = (i32 >= 0) & (cost <= B.MEASURED_MAX) & ((i32 >= B.HIGH) != (i64 >= B.HIGH))
        assert np.all(np.abs(cost[seam] - 20.0) <= bar_above * 2.0 ** -19), (name, form, "seam")
        assert e_max <= bar, (name, form, e_max, bar)
        assert a_max <= bar_above, (name, form, a_max, bar_above)
        assert d_max <= tol, (name, form, d_max, tol)
        if case["differential"]:
            assert pairs >= B.MIN_PAIRS, (name, form, pairs)
        # the reference's winner is queued: within tol of the fp32 winner (rule (a)) or at most zkey (rule (d))
        w32, w64 = np.take_along_axis(i32, ds, 2)[..., 0], np.take_along_axis(i64, ds, 2)[..., 0]
        best = np.where(i32 >= 0, i32, 1 << 40).min(axis=2)
        judged = (np.take_along_axis(cost, ds, 2)[..., 0] <= B.MEASURED_MAX) & ((w32 >= B.HIGH) == (w64 >= B.HIGH)) & \
            ((w32 >= B.HIGH) == (best >= B.HIGH))
        assert np.all((w32 - best <= tol) | (w32 <= zk) | ~judged), (name, form, "a winner outside the band")


# ---- band canaries ---------------------------------------------------------------------------------------------------------------
def _canary_inputs():
    """the tie-rich matrix of tests/test_gpu_exact_forms.py at its small shapes (planner's forms: wave, six per lane, phase-shifted,
    several chunks), and the band cases whose near-ties are not exact: (tag, generator or case, H, W, params)"""
    out = []
    for win, maxd, H, W in ((9, 15, 24, 128), (9, 17, 24, 128), (21, 18, 16, 128), (35, 34, 16, 128), (21, 71, 16, 128)):
        for kind, gC in (("quantised", 0.7), ("black_margins", 5.0), ("patches", 0.7)):
            out.append(("%s %dx%d w%d D%d" % (kind, W, H, win, maxd), kind, H, W,
                        dict(winSize=win, maxDisparity=maxd, minDisparity=0, gammaC=gC, gammaP=17.5)))
    for kind, gC in (("quantised", 0.7), ("black_margins", 5.0)):
        out.append(("%s 600x8 w5 D530" % kind, kind, 8, 600, dict(winSize=5, maxDisparity=530, minDisparity=0, gammaC=gC, gammaP=17.5)))
    for name in ("w35_g5_wave4", "w35_g5_pipe", "w35_g0.7_wave8", "w9_g0.7_wave6", "w21_g5_pipe", "w61_g50",
                 "w9_g0.7_flush", "w21_g0.7_flush", "w35_g0.7_flush"):
        out.append((name, None, 0, 0, None))
    return out


CANARY_BANDS = (("8", 1024), ("1/2", 64), ("1/4", 32), ("1/8", 16), ("1/32", 4), ("1/128", 1))
CANARY_LEFT = {b: 0 for b, _ in CANARY_BANDS}          # running totals over the inputs run so far


@pytest.mark.parametrize("tag,kind,H,W,p", _canary_inputs(), ids=[c[0].replace(" ", "_") for c in _canary_inputs()])
def test_band_canaries(tag, kind, H, W, p, ss):
    """SSAMD_EXACT_TOL at 8 x the default: every map equals the default band's and the oracle's -- a wider band finds nothing
    the default one misses.  At 1/2 ... 1/128 of the default nothing is asserted: the number of pixels that leave the oracle's
    map is printed (with the running total over the inputs so far), and the smallest band that still reproduces every map is
    the measured margin."""
    from simplestereo_amd import _native
    if kind is None:
        L, R, p = B.case_inputs(tag)
    else:
        L, R = T.pair(kind, H, W, p["maxDisparity"], seed=3)
    for cons in (False, True):
        q = dict(p, consistent=cons)
        ref = OC.asw(L, R, **q)
        d = ss.passive.StereoASW(**q).compute(L, R)
        assert _native.counter("exact_overflow") == 0
        assert np.array_equal(d, ref), (tag, cons, int(np.count_nonzero(d != ref)))
        n32 = int(np.count_nonzero(ss.passive.StereoASW(exact=False, **q).compute(L, R) != ref))
        row = []
        for band, t in CANARY_BANDS:
            with _native.options(SSAMD_EXACT_TOL=str(t)):
                dt = ss.passive.StereoASW(**q).compute(L, R)
                assert _native.counter("exact_overflow") == 0
            n = int(np.count_nonzero(dt != ref))
            if band == "8":
                assert np.array_equal(dt, d) and n == 0, (tag, cons, n)
            CANARY_LEFT[band] += n
            row.append("%s: %d" % (band, n))
        print("CANARY %-32s cons=%d  fp32 map alone %5d | pixels off the oracle's map at band x %s" % (tag, cons, n32, "  ".join(row)))
    print("CANARY running total off the oracle's map: " + "  ".join("x %s: %d" % (b, CANARY_LEFT[b]) for b, _ in CANARY_BANDS))
