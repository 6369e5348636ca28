"""Tier T2 (GPU): HIP ASW path vs golden vectors of the reference and vs the CPU oracle.

Tolerance (BASELINE.json north_star): disparity within <= 1 level of the reference on
>= 99.5 % of ALL pixels (every reference output pixel is defined).  The reference
aggregates in fp64, the kernels in fp32, so int16 maps are not required to be
bit-identical; raw costs must agree to |c_gpu - c_ref| <= 1e-4 * max(1, |c_ref|)."""
import json
import os

import numpy as np
import pytest
from simplestereo_amd import _native

import _asw_forms as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "cases.json")) as _f:
    _META = json.load(_f)
_ASW = sorted(k for k, m in _META.items() if m["params"]["algo"] == "asw")

WITHIN1 = 0.995       # the stated bar
EXACT = 0.990         # tighter informational bar: fp32-vs-fp64 argmin flips should be rare


def _within1(a, b):
    return float(np.mean(np.abs(a.astype(np.int32) - b.astype(np.int32)) <= 1))


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import simplestereo_amd
    from simplestereo_amd import _native
    assert _native.lib().ssamd_device_count() >= 1
    return simplestereo_amd


@pytest.mark.parametrize("cid", _ASW)
def test_asw_vs_reference_golden(cid, ss, golden_cases, golden_inputs):
    maps, meta = golden_cases
    a, b = golden_inputs(meta[cid]["input"])
    p = dict(meta[cid]["params"])
    p.pop("algo")
    d = ss.passive.StereoASW(**p).compute(a, b)
    assert d.dtype == np.int16 and d.shape == maps[cid].shape and d.flags["C_CONTIGUOUS"]
    w1, ex = _within1(d, maps[cid]), float(np.mean(d == maps[cid]))
    print("%s within1=%.5f exact=%.5f" % (cid, w1, ex))
    assert w1 >= WITHIN1
    assert ex >= EXACT


@pytest.mark.parametrize("shape,params", [
    ((18, 40), dict(winSize=7, maxDisparity=6, minDisparity=1, gammaC=5, gammaP=17.5)),
    ((33, 70), dict(winSize=35, maxDisparity=20, minDisparity=0, gammaC=5, gammaP=17.5)),
    ((40, 97), dict(winSize=11, maxDisparity=40, minDisparity=3, gammaC=9, gammaP=12.5)),
    ((24, 300), dict(winSize=5, maxDisparity=260, minDisparity=0, gammaC=5, gammaP=17.5)),
])
def test_asw_raw_costs_vs_oracle(shape, params, ss, tsukuba):
    """raw aggregated costs (fp32 kernels vs fp64 oracle), including which entries exist"""
    from oracle import oracle
    from simplestereo_amd.synth import make_pair
    H, W = shape
    a, b, _ = make_pair(H, W, params["maxDisparity"], seed=H + W)
    _, cref = oracle.asw(a, b, return_costs=True, **params)
    c = F.cost_dump(a, b, params)
    assert np.array_equal(np.isnan(c), np.isnan(cref))
    ok = ~np.isnan(cref)
    err = np.abs(c[ok] - cref[ok]) / np.maximum(1.0, np.abs(cref[ok]))
    print("max rel cost err %.3e" % err.max())
    assert err.max() <= 1e-4


def test_lab_conversion_vs_oracle(ss, tsukuba):
    from oracle import oracle
    from simplestereo_amd import _native
    img = tsukuba["left"]
    H, W = img.shape[:2]
    lab = np.empty((H, W, 3), np.float32)
    _native.check(_native.lib().ssamd_bgr2lab(img.ctypes.data, H, W, lab.ctypes.data, -1))
    ref = oracle.bgr2lab(img)
    assert np.abs(lab - ref).max() <= 2e-3        # float32 storage of values up to ~100 + device powf
    ramp = np.arange(256, dtype=np.uint8)
    cube = np.stack(np.meshgrid(ramp[::5], ramp[::5], ramp[::5], indexing="ij"), -1).reshape(1, -1, 3).copy()
    lab2 = np.empty(cube.shape, np.float32)
    _native.check(_native.lib().ssamd_bgr2lab(cube.ctypes.data, 1, cube.shape[1], lab2.ctypes.data, -1))
    ref2 = oracle.bgr2lab(cube)
    assert np.abs(lab2 - ref2).max() <= 1e-4
    # the cube root is evaluated in fp64 (glibc_powf_pos_t): nearly every value is the reference's double rounded to float
    assert float(np.mean(lab2 == ref2.astype(np.float32))) >= 0.995


def test_asw_device_tensor_path_and_strips_bit_exact(ss, golden_inputs):
    """operands resident in HBM; a row strip carrying its halo reproduces the whole-image rows exactly"""
    import torch
    from simplestereo_amd import strips
    a, b = golden_inputs("synth_96x128")
    m = ss.passive.StereoASW(winSize=21, maxDisparity=32, minDisparity=0, consistent=True)
    full = m.compute(a, b)
    tL, tR = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    dev = m.compute(tL, tR)
    assert dev.is_cuda and dev.dtype == torch.int16
    assert np.array_equal(dev.cpu().numpy(), full)
    H, pad = a.shape[0], m.winSize // 2
    for world in (2, 3, 5):
        rows = []
        for rank in range(world):
            r0, r1 = strips.strip_bounds(H, world, rank)
            h0, h1 = strips.halo_bounds(H, r0, r1, pad)
            out = m._compute_device(tL[h0:h1], tR[h0:h1], out_row0=r0 - h0, out_rows=r1 - r0)
            rows.append(out.cpu().numpy())
        assert np.array_equal(np.concatenate(rows, 0), full), world


def test_asw_properties_full_size_config2(ss):
    """BASELINE config 2 (640x480, D 0..64, win 35) against the reference golden G6f is covered by
    test_asw_vs_reference_golden; here: determinism and quality vs the synthetic ground truth"""
    from simplestereo_amd.synth import make_pair
    a, b, gt = make_pair(480, 640, 64, 0)
    m = ss.passive.StereoASW(winSize=35, maxDisparity=64)
    d1, d2 = m.compute(a, b), m.compute(a, b)
    assert np.array_equal(d1, d2)
    vis = np.zeros_like(gt, bool)
    vis[:, 64:] = True
    good = np.abs(d1.astype(np.int32) - gt)[vis] <= 1
    print("config2 quality vs synthetic GT: %.4f" % good.mean())
    assert good.mean() > 0.90


def test_asw_degenerate_ranges(ss, golden_inputs):
    """empty candidate loops leave dBest = 0 -> output x (_passive.cpp:54,98)"""
    from oracle import oracle
    a, b = golden_inputs("crop")
    d = ss.passive.StereoASW(winSize=5, maxDisparity=3, minDisparity=7).compute(a, b)      # max < min
    assert np.array_equal(d, np.tile(np.arange(a.shape[1], dtype=np.int16), (a.shape[0], 1)))
    p = dict(winSize=5, maxDisparity=30, minDisparity=30, gammaC=5, gammaP=17.5, consistent=True)
    assert _within1(ss.passive.StereoASW(**p).compute(a, b), oracle.asw(a, b, **p)) >= WITHIN1
    flat = np.full((12, 50, 3), 77, np.uint8)      # all costs exactly 0: ties -> smallest disparity
    p = dict(winSize=7, maxDisparity=9, minDisparity=2)
    assert np.array_equal(ss.passive.StereoASW(**p).compute(flat, flat), oracle.asw(flat, flat, **p))


SYNTH = (128, 96)        # W, H of the golden input synth_96x128
GEOMS = ["6,5,8", "10,9,16", "3,9,8", "12,3,8", "12,5,0,4", "7,9,8,4", "20,3,4,4", "5,10,12,4"]


def _geometry_rows(geom):
    """the forced tile; the same tile without the second e tile (row-start barrier kept); and with the XOR-swizzled e rows only"""
    p = dict(winSize=21, maxDisparity=int(geom.split(",")[1]) * 4 - 1, minDisparity=0)      # geom = XG,DG[,JC[,RX]]: 4-column register tiles as well
    return [(F.workgroup_tile(geom, **extra),) + SYNTH + (p,)
            for extra in ({}, dict(SSAMD_ASW_NO_E2="1"), dict(SSAMD_ASW_NO_E2="1", SSAMD_ASW_XOR_ONLY="1"))]


@pytest.mark.parametrize("geom", GEOMS)
def test_asw_forced_geometries_and_chunked_staging_agree(geom, ss, golden_inputs):
    """every launch geometry (tile shape, tap-column chunking) computes the same sums in the same order:
    forced shapes via the SSAMD_ASW_GEOM tuning hook must reproduce the default result bit for bit"""
    a, b = golden_inputs("synth_96x128")
    rows = _geometry_rows(geom)
    m = ss.passive.StereoASW(consistent=True, **rows[0][3])
    want = m.compute(a, b)
    for row in rows:
        with F.forced(*row):
            assert np.array_equal(m.compute(a, b), want), row[0][0]


PHASE_SHIFTED = [("6,5,8", 21), ("10,9,16", 35), ("3,9,8", 17), ("12,3,8", 35), ("15,13,16", 35), ("9,17,8", 33),
                 ("4,30,16", 41), ("16,12,8", 17), ("2,3,8", 39)]


def _phase_shifted_rows(geom, win):
    """the tile with whole window rows on the plain kernel, then phase-shifted with chunks of JC and the wave order off and on"""
    XG, DG, JC = (int(v) for v in geom.split(","))
    p = dict(winSize=win, maxDisparity=DG * 4 - 2, minDisparity=1, gammaC=7.0)
    return [(form,) + SYNTH + (p,) for form in [F.workgroup_tile("%d,%d,0,8" % (XG, DG))] +
            [F.pipe_tile(XG, DG, JC, dephase=dephase) for dephase in ("0", "1")]]


@pytest.mark.parametrize("geom,win", PHASE_SHIFTED)
def test_asw_phase_shifted_kernel_equals_the_plain_one(geom, win, ss, golden_inputs):
    """asw_aggregate_pipe_kernel (lanes along the disparity groups, plain LDS rows, waves 0-3 building before they
    aggregate, tail-merged tap-column chunks of 8 or 16) accumulates the same taps in the same order as
    asw_aggregate_kernel: for forced tiles, windows whose last chunk is 8..15 columns long, both chunk lengths and
    the wave order switched on and off, the maps are those of the plain kernel bit for bit (consistent mode: both
    argmins and the raw cost dump as well)"""
    a, b = golden_inputs("synth_96x128")
    plain, *shifted = _phase_shifted_rows(geom, win)
    p = plain[3]
    m = ss.passive.StereoASW(consistent=True, **p)
    with F.forced(*plain):
        want, want_c = m.compute(a, b), F.cost_dump(a, b, p)
    for row in shifted:
        with F.forced(*row):
            got, got_c = m.compute(a, b), F.cost_dump(a, b, p)
        assert np.array_equal(got, want), (geom, win, row[0][0])
        assert F.same_costs(got_c, want_c) == 0, (geom, win, row[0][0])


TAD_VOLUME = [((48, 200), 35, 70), ((36, 1000), 27, 150), ((30, 2000), 35, 192)]


def _tad_volume_rows(shape, win, maxd):
    """the planner's phase-shifted kernel on the TAD volume, and building its e tiles itself"""
    p = dict(winSize=win, maxDisparity=maxd)
    return [((opts, dict(phase_shifted=1)), shape[1], shape[0], p) for opts in ({}, dict(SSAMD_ASW_EVOL="0"))]


@pytest.mark.parametrize("shape,win,maxd", TAD_VOLUME)
def test_asw_tad_volume_equals_the_in_kernel_e_tiles(shape, win, maxd, ss):
    """the phase-shifted kernel fed by LDS-DMA from the pre-computed TAD volume (asw_tad_volume_kernel: 16-byte stores,
    rows of whole 16-byte blocks) computes the map of the same kernel building its e tiles itself (SSAMD_ASW_EVOL=0)"""
    import torch
    from simplestereo_amd.synth import make_pair
    H, W = shape
    L, R, _ = make_pair(H, W, maxd, 21)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    volume, in_kernel = _tad_volume_rows(shape, win, maxd)
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, consistent=True)
    with F.forced(*volume):
        want = m.compute(tL, tR)
    with F.forced(*in_kernel):
        assert torch.equal(m.compute(tL, tR), want)


WAVE = [(35, 16, 0, False), (35, 16, 0, True), (21, 7, 0, True), (9, 3, 0, False),
        (15, 1, 1, True), (1, 12, 0, True), (5, 47, 0, True), (17, 36, 5, True),
        (11, 23, 9, True), (63, 20, 2, False),
        (35, 55, 0, True), (21, 66, 3, False), (15, 48, 0, True)]     # round 3: 49..64 disparities


def _wave_rows(win, maxd, mind):
    """the workgroup kernels, then both register tiles of the wave kernel: the strip's left and right centres as one list of build
    rounds (round 3, merged) and in separate rounds (round-2 form).  A tile that does not fit LDS for the window / range is left out
    by the test (the planner then reports another wave_kernel)."""
    p = dict(winSize=win, maxDisparity=maxd, minDisparity=mind, gammaC=6.0)
    return [(form,) + SYNTH + (p,) for form in [F.NO_WAVE] +
            [F.wave(rx, SSAMD_ASW_WAVE_MERGE=merge) for rx, merge in (("8", None), ("4", None), ("8", "0"), ("4", "0"))]]


def _fits(row):
    """does the wave kernel's tile of this row fit LDS?  Any other mismatch of the form is the test's failure."""
    try:
        with F.forced(*row):
            return True
    except F.FormMismatch as e:
        if e.key != "wave_kernel":
            raise
        return False


@pytest.mark.parametrize("win,maxd,mind,consistent", WAVE)
def test_asw_wave_kernel_equals_the_workgroup_kernels(win, maxd, mind, consistent, ss, golden_inputs):
    """asw_aggregate_wave_kernel (small disparity ranges: a wave builds the support weights of its own strip, no
    workgroup barriers) accumulates the same taps in the same order as the workgroup kernels: with both register tiles
    forced, for ranges of 1..48 disparities, windows 1..63, minDisparity 0 and above, image widths that end
    inside a strip and images narrower than one strip, the maps -- consistent mode: both argmins, and the raw cost
    dump -- are those of the workgroup kernel bit for bit.  The class default (maxDisparity 16) runs this kernel."""
    a, b = golden_inputs("synth_96x128")
    pairs = [(a, b), (np.ascontiguousarray(a[:50, :77]), np.ascontiguousarray(b[:50, :77])),
             (np.ascontiguousarray(a[:40, :23]), np.ascontiguousarray(b[:40, :23]))]
    full_hd = lambda win, maxd, mind=0: F.planned(1920, 1080, dict(winSize=win, maxDisparity=maxd, minDisparity=mind))["wave_kernel"]   # noqa: E731
    assert full_hd(win, maxd, mind) in (4, 8)
    assert full_hd(35, 16) == 4          # class default range (round 3: merged build rounds)
    assert full_hd(35, 20) == 8 and full_hd(35, 64) == 0
    workgroup, *tiles = _wave_rows(win, maxd, mind)
    p = workgroup[3]
    m = ss.passive.StereoASW(consistent=consistent, **p)

    def run(L, R):
        return m.compute(L, R), F.cost_dump(L, R, p)
    with F.forced(*workgroup):
        want = [run(L, R) for L, R in pairs]
    ran = 0
    for row in tiles:
        if not _fits(row):
            continue                                      # this tile does not fit LDS for the window / range
        ran += 1
        with F.forced(*row):
            for (L, R), (wd, wc) in zip(pairs, want):
                gd, gc = run(L, R)
                assert np.array_equal(gd, wd), (row[0][0], L.shape)
                assert F.same_costs(gc, wc) == 0, (row[0][0], L.shape)
    assert ran >= 2


FULL_WIDTH = [(7, 35), (16, 35), (39, 21), (60, 35)]


def _full_width_rows(maxd, win):
    """the workgroup kernels; both tiles of the wave kernel with 1, 2 and 4 waves per workgroup; the last of them not unrolled"""
    p = dict(winSize=win, maxDisparity=maxd)
    return [(form, 1920, 44, p) for form in [F.NO_WAVE] +
            [F.wave(rx, SSAMD_ASW_WAVE_WG=wg) for rx, wg in (("8", "1"), ("4", "1"), ("8", "4"), ("4", "2"))] +
            [F.wave("4", SSAMD_ASW_WAVE_WG="2", SSAMD_ASW_WAVE_UNROLL="0")]]


@pytest.mark.parametrize("maxd,win", FULL_WIDTH)
def test_asw_wave_kernel_full_width_rows(maxd, win, ss):
    """1920-column rows (20 strips of 96 columns / 15 of 128 / 34 of 56 plus a ragged last one; waves per workgroup 1, 2
    and 4): both tiles of the wave kernel give the map of the workgroup kernels bit for bit"""
    import torch
    from simplestereo_amd.synth import make_pair
    L, R, _ = make_pair(44, 1920, maxd, 11)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, consistent=True)
    workgroup, *tiles = _full_width_rows(maxd, win)
    with F.forced(*workgroup):
        want = m.compute(tL, tR)
    for row in tiles:
        with F.forced(*row):
            assert torch.equal(m.compute(tL, tR), want), row[0][0]


STRIPS = dict(winSize=13, maxDisparity=16)


def test_asw_wave_kernel_strips_and_alternate_rows(ss, golden_inputs):
    """the wave kernel under the other entry points: a row strip with its halo equals the rows of the whole frame, the
    alternate-rows mode and the separate argmins equal those computed with the workgroup kernels"""
    import torch
    a, b = golden_inputs("synth_96x128")
    tL, tR = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m = ss.passive.StereoASW(consistent=True, **STRIPS)
    alt = ss.passive.StereoASW(alternate=True, **STRIPS)
    with F.forced(F.NO_WAVE, *SYNTH, STRIPS):
        want, want_alt = m.compute(tL, tR), alt.compute(tL, tR)
        want_strip = m._compute_device(tL[20:70].contiguous(), tR[20:70].contiguous(), out_row0=6, out_rows=38)
    for rx in ("8", "4"):
        with F.forced(F.wave(rx), *SYNTH, STRIPS):
            assert torch.equal(m.compute(tL, tR), want)
            assert torch.equal(alt.compute(tL, tR), want_alt)
            got_strip = m._compute_device(tL[20:70].contiguous(), tR[20:70].contiguous(), out_row0=6, out_rows=38)
            assert torch.equal(got_strip, want_strip)
            assert torch.equal(got_strip, want[26:64])


@pytest.mark.parametrize("H,W,maxd,shift", [(1080, 1920, 192, 150), (2160, 4096, 256, 233)])
def test_asw_full_size_configs_3_and_5_known_shift_and_strip_invariance(H, W, maxd, shift, ss):
    """BASELINE configs 3 and 5 at full size, through size-independent properties: (1) a right image that is the
    left image moved by a constant shift has aggregated cost exactly 0 at d = shift wherever the window and its
    shifted copy are inside the image -> the map must equal the shift there (ties -> smallest d cannot
    undercut it on a textured image); (2) rows matched as a strip carrying its halo equal the same rows of the
    whole frame bit for bit; (3) determinism."""
    import torch
    from simplestereo_amd.synth import make_pair
    L = make_pair(H, W, maxd, 5)[0]
    R = np.zeros_like(L)
    R[:, :W - shift] = L[:, shift:]
    R[:, W - shift:] = L[:, :shift]                      # wrapped columns: not inspected
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = ss.passive.StereoASW(winSize=35, maxDisparity=maxd)
    d = m.compute(tL, tR)
    torch.cuda.synchronize()
    dn = d.cpu().numpy()
    pad = 17
    inner = dn[:, shift + pad:W - pad]                    # right taps x - shift - pad .. stay inside [0, W - shift)
    frac = float((inner == shift).mean())
    print("%dx%d D0..%d: %.5f of the interior pixels at the known shift %d" % (W, H, maxd, frac, shift))
    assert frac >= 0.9999
    assert torch.equal(m.compute(tL, tR), d)
    r0, rows = H // 2 - 20, 45
    h0, h1 = r0 - pad, r0 + rows + pad
    strip = m._compute_device(tL[h0:h1].contiguous(), tR[h0:h1].contiguous(), out_row0=r0 - h0, out_rows=rows)
    assert torch.equal(strip, d[r0:r0 + rows])


AUTOTUNE = [dict(winSize=21, maxDisparity=39), dict(winSize=35, maxDisparity=16, consistent=True),
            dict(winSize=9, maxDisparity=70, minDisparity=3), dict(winSize=15, maxDisparity=24, alternate=True)]


def _unrelated_rows():
    """a forced geometry that has nothing to do with the tuner's, on the 120-column crop"""
    return [(F.tile("3,5,8"), 120, 96, p) for p in AUTOTUNE]


def test_autotune_changes_the_geometry_never_the_map(ss, golden_inputs):
    """with autotuning on, the first call of a shape times ~10 candidate geometries (8- and 4-column tiles, chunked
    and unchunked, key path and direct path) on the call's buffers; the map must be the one of the model's choice"""
    a, b = golden_inputs("synth_96x128")
    cases = AUTOTUNE
    want = [ss.passive.StereoASW(**p).compute(a, b) for p in cases]
    before = ss.passive.set_autotune(True)
    try:
        # other image sizes than `want` used, so these shapes have not been seen (tuned or cached) yet
        a2, b2 = np.ascontiguousarray(a[:, :120]), np.ascontiguousarray(b[:, :120])
        ref2 = [None] * len(cases)
        got_first = [ss.passive.StereoASW(**p).compute(a2, b2) for p in cases]        # tuning calls
        got_again = [ss.passive.StereoASW(**p).compute(a2, b2) for p in cases]        # tuned geometry from the cache
    finally:
        ss.passive.set_autotune(before)
    from oracle import oracle
    for p, g1, g2 in zip(cases, got_first, got_again):
        assert np.array_equal(g1, g2)
    forced = []                                             # an unrelated forced geometry computes the same maps
    for row in _unrelated_rows():
        with F.forced(*row):
            forced.append(ss.passive.StereoASW(**row[3]).compute(a2, b2))
    for g1, f in zip(got_first, forced):
        assert np.array_equal(g1, f)
    assert all(w.shape == (96, 128) for w in want)


@pytest.mark.parametrize("shape,win,maxd,consistent", [((48, 200), 35, 60, False), ((48, 200), 35, 70, True), ((40, 300), 21, 16, True),
                                                       ((30, 2000), 35, 192, False),
                                                       # tiles planned on the volume (their LDS only fits without the staged colour bytes): re-planned
                                                       ((30, 1920), 35, 64, False), ((24, 1920), 35, 128, True)])
def test_asw_without_room_for_the_tad_volume(shape, win, maxd, consistent, ss):
    """when the device has no room for the pre-computed TAD volume (here: the cap forced down to 1 MiB) the phase-shifted
    kernel builds its e tiles itself and a small range falls back from the wave kernel to the workgroup kernels: same maps"""
    import torch
    from simplestereo_amd.synth import make_pair
    H, W = shape
    L, R, _ = make_pair(H, W, maxd, 9)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, consistent=consistent)
    want = m.compute(tL, tR)
    with _native.options(SSAMD_ASW_EVOL_MAX_MB="1"):
        got = m.compute(tL, tR)
    assert torch.equal(got, want)
    assert torch.equal(m.compute(tL, tR), want)


def test_asw_when_the_tad_volume_allocation_really_fails(ss):
    """SSAMD_ASW_EVOL_FAIL makes the volume's allocation a hipMalloc no device can serve: the failure is HIP's sticky last
    error on ROCm 7, and the advertised fallback (phase-shifted kernel with in-kernel e tiles) must still run -- same map,
    the fallback counted, and the next ordinary call gets its volume again"""
    import torch
    from simplestereo_amd.synth import make_pair
    L, R, _ = make_pair(40, 300, 70, 9)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = ss.passive.StereoASW(winSize=35, maxDisparity=70)
    assert F.planned(300, 40, dict(winSize=35, maxDisparity=70))["phase_shifted"] == 1
    want = m.compute(tL, tR)
    with _native.options(SSAMD_ASW_EVOL_FAIL="1"):
        with F.counted("evol_fallbacks") as n:
            got = m.compute(tL, tR)
        assert torch.equal(got, want)
        assert n.delta == 1
        # the small-range wave kernel cannot run without its volume: the call falls back to the workgroup geometry stored
        # next to the wave geometry (round 5; a clean error until round 4) -- same map, the fallback counted, no stale HIP
        # error afterwards; a first call of a shape under the tuner simply ends up on a workgroup candidate
        small = ss.passive.StereoASW(winSize=35, maxDisparity=16)
        prev = _native.lib().ssamd_autotune(0)
        try:
            with F.counted("evol_fallbacks") as n:
                untuned = small.compute(tL, tR)
            assert n.delta > 0
        finally:
            _native.lib().ssamd_autotune(prev)
        tuned = small.compute(tL, tR)
        assert torch.equal(untuned, tuned)
    with F.counted("evol_fallbacks") as n:
        assert torch.equal(small.compute(tL, tR), tuned)      # same map from the wave kernel once the volume can be had again
        assert torch.equal(m.compute(tL, tR), want)
    assert n.delta == 0 and _native.counter("evol_bytes") > 0
    assert ss.passive.StereoASW(winSize=35, maxDisparity=16).compute(tL, tR).shape == (40, 300)


@pytest.mark.parametrize("shape,maxd,consistent,force", [((135, 1920), 192, False, None), ((135, 1920), 192, True, None),
                                                         ((90, 700), 70, False, "1"), ((90, 700), 70, True, "1")])
def test_asw_half_width_tiles_for_the_last_partial_round(shape, maxd, consistent, force, ss):
    """a launch whose last round of workgroups is at most half full (the 135-row strip of an 8-GPU run of config 3: 8.44
    rounds) runs the rows of that round with tiles of half the columns: same maps, same raw costs as one geometry for all rows.
    (90 x 700 / D 0..70: 4-wave tiles of 88 columns, two resident per CU -- 720 workgroups = 1.4 rounds of 512; round 5 counts the
    slots as CUs x resident workgroups, until round 4 a 37-row frame was split against 256 slots although all of it fits one round)"""
    import torch
    from simplestereo_amd.synth import make_pair
    H, W = shape
    L, R, _ = make_pair(H, W, maxd, 21)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    p = dict(winSize=35, maxDisparity=maxd)
    m = ss.passive.StereoASW(consistent=consistent, **p)
    with _native.options(SSAMD_ASW_TAIL="0", SSAMD_AUTOTUNE="0"), F.counted("tail_splits") as n:
        want = m.compute(tL, tR)
        cw = F.cost_dump(L, R, p) if not consistent else None
    assert n.delta == 0
    opts = dict(SSAMD_AUTOTUNE="0")
    if force:
        opts["SSAMD_ASW_TAIL"] = force
    with _native.options(**opts):
        with F.counted("tail_splits") as n:
            got = m.compute(tL, tR)
        assert n.delta == 1, "the split did not happen: the test does not test it"
        if cw is not None:
            assert F.same_costs(F.cost_dump(L, R, p), cw) == 0
    assert torch.equal(got, want)


def test_tad_volume_is_not_released_on_every_switch_of_shape(ss):
    """a workload alternating a large and a small shape keeps the larger volume (given back only after eight small calls
    in a row): no hipFree / hipMalloc per switch"""
    import torch
    from simplestereo_amd.synth import make_pair
    L, R, _ = make_pair(800, 1920, 192, 2)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    big = ss.passive.StereoASW(winSize=35, maxDisparity=192)
    small = ss.passive.StereoASW(winSize=35, maxDisparity=16)
    sL, sR = tL[:48].contiguous(), tR[:48].contiguous()
    big.compute(tL, tR)
    cap = _native.counter("evol_bytes")
    if cap <= (256 << 20):
        pytest.skip("the volume of this frame is below the release threshold")
    for _ in range(3):
        small.compute(sL, sR)
        assert _native.counter("evol_bytes") == cap
        big.compute(tL, tR)
    for _ in range(9):
        small.compute(sL, sR)
    assert _native.counter("evol_bytes") < cap


SIX = [(35, 16, 0, False), (35, 16, 0, True), (15, 17, 0, True), (7, 21, 5, False), (63, 18, 2, True), (11, 22, 5, True)]


def _six_rows(win, maxd, mind):
    """the workgroup kernels, three groups of six per lane, five groups of four: asked at the 700 x 37 frame.  The test skips a
    window whose 4-column tile does not fit LDS."""
    p = dict(winSize=win, maxDisparity=maxd, minDisparity=mind, gammaC=6.0)
    return [(form, 700, 37, p) for form in (F.NO_WAVE, "wave6", "wave4x5")]


@pytest.mark.parametrize("win,maxd,mind,consistent", SIX)
def test_asw_wave_kernel_six_disparities_per_lane(win, maxd, mind, consistent, ss, golden_inputs):
    """asw_aggregate_wave6_kernel (17 / 18 disparities -- the class default maxDisparity = 16 -- as three groups of SIX per
    lane: 8-byte e slots, nine right weights from an 8-byte-aligned address) computes the maps and the raw costs of the
    four-per-lane wave kernel and of the workgroup kernels bit for bit, on full and ragged images"""
    from simplestereo_amd.synth import make_pair
    nD = maxd - mind + 1
    assert nD in (17, 18)
    a, b = golden_inputs("synth_96x128")
    L2, R2, _ = make_pair(37, 700, maxd, 5)
    pairs = [(a, b), (np.ascontiguousarray(a[:50, :77]), np.ascontiguousarray(b[:50, :77])), (L2, R2),
             (np.ascontiguousarray(a[:9, :23]), np.ascontiguousarray(b[:9, :23]))]
    workgroup, six_row, four_row = _six_rows(win, maxd, mind)
    p = workgroup[3]
    m = ss.passive.StereoASW(consistent=consistent, **p)

    def run(L, R):
        return m.compute(L, R), F.cost_dump(L, R, p)
    with F.forced(*workgroup):
        want = [run(L, R) for L, R in pairs]
    if not _fits(six_row):
        pytest.skip("the 4-column tile does not fit LDS for this window")
    with F.forced(*six_row):                                # three groups of six
        six = [run(L, R) for L, R in pairs]
    with F.forced(*four_row):                               # five groups of four
        four = [run(L, R) for L, R in pairs]
    for (wd, wc), (sd, sc), (fd, fc) in zip(want, six, four):
        assert np.array_equal(sd, wd) and np.array_equal(fd, wd)
        assert F.same_costs(sc, wc) == 0 and F.same_costs(fc, wc) == 0


@pytest.mark.parametrize("shape,win,maxd,mind,consistent", [((48, 160), 65, 20, 0, False), ((60, 140), 99, 12, 2, True),
                                                             ((50, 180), 127, 40, 0, False), ((40, 120), 255, 9, 0, True),
                                                             ((30, 200), 191, 70, 0, False)])
def test_asw_windows_beyond_63(shape, win, maxd, mind, consistent, ss):
    """windows of 65 .. 255 columns (the geometry search accepts up to 255; the small-range wave kernel stops at 63, so these run
    the workgroup kernels with tap-column chunking): raw costs within the stated tolerance of the fp64 oracle, maps within the bars,
    GSW with the same windows bit-exact"""
    from oracle import oracle
    from simplestereo_amd.synth import make_pair
    H, W = shape
    L, R, _ = make_pair(H, W, maxd, 31 + win)
    p = dict(winSize=win, maxDisparity=maxd, minDisparity=mind, gammaC=7.0, gammaP=40.0)
    d = ss.passive.StereoASW(consistent=consistent, **p).compute(L, R)
    ref, cref = oracle.asw(L, R, consistent=False, return_costs=True, **p)
    if consistent:
        ref = oracle.asw(L, R, consistent=True, **p)
    c = F.cost_dump(L, R, p)
    assert np.array_equal(np.isnan(c), np.isnan(cref))
    ok = ~np.isnan(cref)
    assert (np.abs(c[ok] - cref[ok]) / np.maximum(1.0, np.abs(cref[ok]))).max() <= 1e-4
    diff = np.abs(d.astype(np.int32) - ref.astype(np.int32))
    print("win %d: exact %.4f within-1 %.4f" % (win, np.mean(diff == 0), np.mean(diff <= 1)))
    assert np.mean(diff <= 1) >= 0.995 and np.mean(diff == 0) >= 0.99
    if win <= 127:          # (the closed-form oracle needs seconds for these; the literal relaxation would need hours)
        g = dict(winSize=win, maxDisparity=maxd, minDisparity=mind, gamma=10, fMax=120, iterations=3)
        assert np.array_equal(ss.passive.StereoGSW(**g).compute(L, R), oracle.gsw(L, R, closed=True, **g))


def forced_rows():
    """every forced form of this file, as (form, W, H, params): tests/test_asw_forms_cpu.py asks the planner for each"""
    rows = [row for geom in GEOMS for row in _geometry_rows(geom)]
    rows += [row for r in PHASE_SHIFTED for row in _phase_shifted_rows(*r)] + [row for r in TAD_VOLUME for row in _tad_volume_rows(*r)]
    rows += [_wave_rows(*r[:3])[0] for r in WAVE] + [row for r in FULL_WIDTH for row in _full_width_rows(*r)]
    rows += [(form,) + SYNTH + (STRIPS,) for form in (F.NO_WAVE, F.wave("8"), F.wave("4"))]
    return rows + _unrelated_rows() + [_six_rows(*r[:3])[0] for r in SIX]


def rows_that_may_not_fit():
    """wave-kernel tiles that the tests leave out, or skip for, where they do not fit LDS; the tests that need them are listed
    with the least number of rows that must fit"""
    return [(_wave_rows(*r[:3])[1:], 2) for r in WAVE] + [(_six_rows(*r[:3])[1:], 0) for r in SIX]
