"""GPU tier: the support-weight build of asw_aggregate_kernel (the "workgroup" form) has ONE batch body, run for whole batches of
ASW_WB tap columns and, with clamped indices, for the last partial batch of a segment.  A sweep over the windows 3 .. 17 on both
register tiles (8 and 4 columns per thread), with whole window rows and with chunks of tap columns, runs it at segment lengths
of every remainder modulo ASW_WB; the standard is the wave kernel, whose device code does not go through that body:
  * the cost images of the cost-writing instantiations (test hook SSAMD_ASW_COST_KEYS, as tests/test_gpu_asw_band.py reads
    them) equal the wave kernel's word for word, on its 4- and its 8-column tile;
  * the maps of the instantiations a StereoASW call runs equal the fp64 oracle's.
The segment rule of asw_layout_e (csrc/asw_plan.h) is restated here from ssamd_asw_geometry's tile, and the sweep is held to
cover the remainders 0, 1, 2 and 3 on each register tile -- that part needs no device."""
import numpy as np
import pytest

import _asw_band_ref as B
import _asw_forms as F
import _tie_inputs as T

H, W, MAXD, SEED = 6, 96, 19, 3
ASW_WB = 4                                     # csrc/asw_shared.hip.h
WINDOWS = tuple(range(3, 18, 2))
# SSAMD_ASW_GEOM = "XG,DG,JC,RX": 40- and 28-column tiles (the last one of a row partial), 12 disparities per chunk (two chunks,
# the second reaching past maxDisparity); JC 0 = whole window rows
GEOMS = {8: ("5,3,0,8", "5,3,8,8"), 4: ("7,3,0,4", "7,3,4,4")}
OC = T.OracleCache()


def _params(win):
    return dict(winSize=win, maxDisparity=MAXD, minDisparity=0, gammaC=5.0, gammaP=17.5)


def _tile(win, geom):
    """the workgroup form on a forced tile, several tiles to a row"""
    return F.also(F.workgroup_tile(geom, win=win), grid_x=lambda n: n > 1)


def _plan(win, geom):
    with F.forced(_tile(win, geom), W, H, _params(win)) as f:
        return f


def forced_rows():
    """every form the sweep forces, as (form, W, H, params): tests/test_asw_forms_cpu.py asks the planner for each"""
    for win in WINDOWS:
        for form in [F.wave(4), F.wave(8)] + [_tile(win, geom) for geoms in GEOMS.values() for geom in geoms]:
            yield form, W, H, _params(win)


def segment_lengths(win, geom, rx):
    """the tap-column segments one weight-build task covers, per chunk of a window row: asw_layout_e's balance rule
    (the cheapest of 1 .. 8 segments per chunk, a round of tasks costing the segment length rounded up to ASW_WB, plus 2)"""
    f = _plan(win, geom)
    assert f["tile_columns"] == rx, f
    wcols = f["chunk_columns"] or win
    ncen = 2 * f["tile_x"] + f["chunk_d"] - 1               # left centres Tx, right centres Tx + Dc - 1
    best = None
    for ns in range(1, min(wcols, 8) + 1):
        length = (wcols + ns - 1) // ns
        rounds = (ncen * ns + f["threads"] - 1) // f["threads"]
        cost = rounds * ((length + ASW_WB - 1) // ASW_WB * ASW_WB + 2)
        if best is None or cost < best[0]:
            best = (cost, ns, length)
    _, wseg, wlen = best
    out = []
    for jc in range(0, win, wcols):
        jend = min(win, jc + wcols)
        for sgm in range(wseg):
            j0, j1 = jc + sgm * wlen, min(jend, jc + (sgm + 1) * wlen)
            if j1 > j0:
                out.append(j1 - j0)
    assert sum(out) == win
    return out


def test_the_sweep_covers_every_remainder_of_a_segment_on_both_register_tiles():
    for rx, geoms in GEOMS.items():
        seen = {(n % ASW_WB, n >= ASW_WB) for geom in geoms for win in WINDOWS for n in segment_lengths(win, geom, rx)}
        assert {r for r, _ in seen} == {0, 1, 2, 3}, (rx, sorted(seen))
        # a remainder after whole batches and a segment that is nothing but a remainder
        assert {r for r, whole in seen if whole and r} and {r for r, whole in seen if not whole}, (rx, sorted(seen))
        assert any(int(g.split(",")[2]) and _plan(win, g)["chunk_columns"] for g in geoms for win in WINDOWS)


@pytest.mark.gpu
@pytest.mark.parametrize("win", WINDOWS)
def test_workgroup_build_against_the_wave_kernel_and_the_oracle(win):
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    L, R = T.pair("perturbed:stripes", H, W, MAXD, seed=SEED)
    p = _params(win)
    ref = OC.asw(L, R, **p)
    wave = {}
    for rx in (4, 8):
        with F.forced(F.wave(rx), W, H, p):
            wave[rx] = B.image32(F.cost_dump(L, R, p, keys=True))
    assert np.array_equal(wave[4], wave[8])
    assert np.any(wave[4] >= 0) and np.any(wave[4] < 0)              # candidates that exist, and the left border's that do not
    for rx, geoms in GEOMS.items():
        for geom in geoms:
            with F.forced(_tile(win, geom), W, H, p) as f:
                assert f["tile_columns"] == rx, f
                img = B.image32(F.cost_dump(L, R, p, keys=True))
                d = ss.passive.StereoASW(**p).compute(L, R)
                assert _native.counter("exact_overflow") == 0
            for wrx in (4, 8):
                assert np.array_equal(img, wave[wrx]), (win, geom, "wave", wrx, int(np.count_nonzero(img != wave[wrx])))
            assert np.array_equal(d, ref), (win, geom, int(np.count_nonzero(d != ref)))
