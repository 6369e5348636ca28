"""Tier T2 (GPU): HIP ASW path vs golden vectors of the reference and vs the CPU oracle.

Tolerance (BASELINE.json north_star): disparity within <= 1 level of the reference on
>= 99.5 % of ALL pixels (every reference output pixel is defined).  The reference
aggregates in fp64, the kernels in fp32, so int16 maps are not required to be
bit-identical; raw costs must agree to |c_gpu - c_ref| <= 1e-4 * max(1, |c_ref|)."""
import json
import os

import numpy as np
import pytest
from simplestereo_amd import _native      # noqa: E402  (tuning options: _native.set_option)

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
    import ctypes
    from oracle import oracle
    from simplestereo_amd import _native
    from simplestereo_amd.synth import make_pair
    H, W = shape
    a, b, _ = make_pair(H, W, params["maxDisparity"], seed=H + W)
    _, cref = oracle.asw(a, b, return_costs=True, **params)
    nD = params["maxDisparity"] - params["minDisparity"] + 1
    c = np.empty((H, W, nD), np.float32)
    _native.check(_native.lib().ssamd_asw_costs(a.ctypes.data, b.ctypes.data, H, W, params["winSize"],
                                                params["maxDisparity"], params["minDisparity"],
                                                float(params["gammaC"]), float(params["gammaP"]),
                                                c.ctypes.data, -1))
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


@pytest.mark.parametrize("geom", ["6,5,8", "10,9,16", "3,9,8", "12,3,8", "12,5,0,4", "7,9,8,4", "20,3,4,4", "5,10,12,4"])
def test_asw_forced_geometries_and_chunked_staging_agree(geom, ss, golden_inputs):
    """every launch geometry (tile shape, tap-column chunking) computes the same sums in the same order:
    forced shapes via the SSAMD_ASW_GEOM tuning hook must reproduce the default result bit for bit"""
    a, b = golden_inputs("synth_96x128")
    maxd = int(geom.split(",")[1]) * 4 - 1        # geom = XG,DG[,JC[,RX]]: 4-column register tiles as well
    m = ss.passive.StereoASW(winSize=21, maxDisparity=maxd, minDisparity=0, consistent=True)
    want = m.compute(a, b)
    _native.set_option("SSAMD_ASW_GEOM", geom)
    try:
        got = m.compute(a, b)
        # the same tile without the second e tile (row-start barrier kept) and with the XOR-swizzled e rows only
        _native.set_option("SSAMD_ASW_NO_E2", "1")
        got_one_e = m.compute(a, b)
        _native.set_option("SSAMD_ASW_XOR_ONLY", "1")
        got_xor = m.compute(a, b)
    finally:
        for k in ("SSAMD_ASW_GEOM", "SSAMD_ASW_NO_E2", "SSAMD_ASW_XOR_ONLY"):
            _native.set_option(k, None)
    assert np.array_equal(got, want)
    assert np.array_equal(got_one_e, want) and np.array_equal(got_xor, want)


@pytest.mark.parametrize("geom,win", [("6,5,8", 21), ("10,9,16", 35), ("3,9,8", 17), ("12,3,8", 35), ("15,13,16", 35), ("9,17,8", 33),
                                      ("4,30,16", 41), ("16,12,8", 17), ("2,3,8", 39)])
def test_asw_phase_shifted_kernel_equals_the_plain_one(geom, win, ss, golden_inputs):
    """asw_aggregate_pipe_kernel (lanes along the disparity groups, plain LDS rows, waves 0-3 building before they
    aggregate, tail-merged tap-column chunks of 8 or 16) accumulates the same taps in the same order as
    asw_aggregate_kernel: for forced tiles, windows whose last chunk is 8..15 columns long, both chunk lengths and
    the wave order switched on and off, the maps are those of the plain kernel bit for bit (consistent mode: both
    argmins and the raw cost dump as well)"""
    a, b = golden_inputs("synth_96x128")
    XG, DG, JC = (int(v) for v in geom.split(","))
    maxd = DG * 4 - 2
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, minDisparity=1, consistent=True, gammaC=7.0)
    from simplestereo_amd import _native
    H, W = a.shape[:2]

    def costs():
        c = np.empty((H, W, maxd), np.float32)
        _native.check(_native.lib().ssamd_asw_costs(a.ctypes.data, b.ctypes.data, H, W, win, maxd, 1, 7.0, 17.5, c.ctypes.data, -1))
        return c
    _native.set_option("SSAMD_ASW_GEOM", "%d,%d,0,8" % (XG, DG))          # the tile, whole window rows, plain kernel
    _native.set_option("SSAMD_ASW_PIPE", "0")
    try:
        want, want_c = m.compute(a, b), costs()
        for dephase in ("0", "1"):
            _native.set_option("SSAMD_ASW_PIPE", str(JC))
            _native.set_option("SSAMD_ASW_DEPHASE", dephase)
            got, got_c = m.compute(a, b), costs()
            assert np.array_equal(got, want), (geom, win, dephase)
            assert np.array_equal(got_c, want_c, equal_nan=True), (geom, win, dephase)
    finally:
        for k in ("SSAMD_ASW_GEOM", "SSAMD_ASW_PIPE", "SSAMD_ASW_DEPHASE"):
            _native.set_option(k, None)


@pytest.mark.parametrize("shape,win,maxd", [((48, 200), 35, 70), ((36, 1000), 27, 150), ((30, 2000), 35, 192)])
def test_asw_tad_volume_equals_the_in_kernel_e_tiles(shape, win, maxd, ss):
    """the phase-shifted kernel fed by LDS-DMA from the pre-computed TAD volume (asw_tad_volume_kernel: 16-byte stores,
    rows of whole 16-byte blocks) computes the map of the same kernel building its e tiles itself (SSAMD_ASW_EVOL=0)"""
    import torch
    from simplestereo_amd import _native
    from simplestereo_amd.synth import make_pair
    H, W = shape
    L, R, _ = make_pair(H, W, maxd, 21)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    assert _native.asw_kernel_form(W, H, win, maxd, 0)["phase_shifted"] == 1
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, consistent=True)
    want = m.compute(tL, tR)
    try:
        _native.set_option("SSAMD_ASW_EVOL", "0")
        assert torch.equal(m.compute(tL, tR), want)
    finally:
        _native.set_option("SSAMD_ASW_EVOL", None)


@pytest.mark.parametrize("win,maxd,mind,consistent", [(35, 16, 0, False), (35, 16, 0, True), (21, 7, 0, True), (9, 3, 0, False),
                                                       (15, 1, 1, True), (1, 12, 0, True), (5, 47, 0, True), (17, 36, 5, True),
                                                       (11, 23, 9, True), (63, 20, 2, False),
                                                       (35, 55, 0, True), (21, 66, 3, False), (15, 48, 0, True)])     # round 3: 49..64 disparities
def test_asw_wave_kernel_equals_the_workgroup_kernels(win, maxd, mind, consistent, ss, golden_inputs):
    """asw_aggregate_wave_kernel (small disparity ranges: a wave builds the support weights of its own strip, no
    workgroup barriers) accumulates the same taps in the same order as the workgroup kernels: with both register tiles
    forced, for ranges of 1..48 disparities, windows 1..63, minDisparity 0 and above, image widths that end
    inside a strip and images narrower than one strip, the maps -- consistent mode: both argmins, and the raw cost
    dump -- are those of the workgroup kernel bit for bit.  The class default (maxDisparity 16) runs this kernel."""
    from simplestereo_amd import _native
    a, b = golden_inputs("synth_96x128")
    pairs = [(a, b), (np.ascontiguousarray(a[:50, :77]), np.ascontiguousarray(b[:50, :77])),
             (np.ascontiguousarray(a[:40, :23]), np.ascontiguousarray(b[:40, :23]))]
    nD = maxd - mind + 1
    assert _native.asw_kernel_form(1920, 1080, win, maxd, mind)["wave_kernel"] in (4, 8)
    assert _native.asw_kernel_form(1920, 1080, 35, 16, 0)["wave_kernel"] == 4          # class default range (round 3: merged build rounds)
    assert _native.asw_kernel_form(1920, 1080, 35, 20, 0)["wave_kernel"] == 8
    assert _native.asw_kernel_form(1920, 1080, 35, 64, 0)["wave_kernel"] == 0
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, minDisparity=mind, consistent=consistent, gammaC=6.0)

    def run(L, R):
        H, W = L.shape[:2]
        c = np.empty((H, W, nD), np.float32)
        _native.check(_native.lib().ssamd_asw_costs(L.ctypes.data, R.ctypes.data, H, W, win, maxd, mind, 6.0, 17.5, c.ctypes.data, -1))
        return m.compute(L, R), c
    try:
        _native.set_option("SSAMD_ASW_WAVE", "0")
        want = [run(L, R) for L, R in pairs]
        _native.set_option("SSAMD_ASW_WAVE", "1")
        ran = 0
        # both register tiles; the strip's left and right centres as one list of build rounds (round 3, merged) and in
        # separate rounds (round-2 form)
        for rx, merge in (("8", None), ("4", None), ("8", "0"), ("4", "0")):
            _native.set_option("SSAMD_ASW_WAVE_RX", rx)
            _native.set_option("SSAMD_ASW_WAVE_MERGE", merge)
            if _native.asw_kernel_form(128, 96, win, maxd, mind)["wave_kernel"] != int(rx):
                continue                                      # this tile does not fit LDS for the window / range
            ran += 1
            for (L, R), (wd, wc) in zip(pairs, want):
                gd, gc = run(L, R)
                assert np.array_equal(gd, wd), (rx, merge, L.shape)
                assert np.array_equal(gc, wc, equal_nan=True), (rx, merge, L.shape)
        assert ran >= 2
    finally:
        for k in ("SSAMD_ASW_WAVE", "SSAMD_ASW_WAVE_RX", "SSAMD_ASW_WAVE_MERGE"):
            _native.set_option(k, None)


@pytest.mark.parametrize("maxd,win", [(7, 35), (16, 35), (39, 21), (60, 35)])
def test_asw_wave_kernel_full_width_rows(maxd, win, ss):
    """1920-column rows (20 strips of 96 columns / 15 of 128 / 34 of 56 plus a ragged last one; waves per workgroup 1, 2
    and 4): both tiles of the wave kernel give the map of the workgroup kernels bit for bit"""
    import torch
    from simplestereo_amd.synth import make_pair
    L, R, _ = make_pair(44, 1920, maxd, 11)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, consistent=True)
    try:
        _native.set_option("SSAMD_ASW_WAVE", "0")
        want = m.compute(tL, tR)
        _native.set_option("SSAMD_ASW_WAVE", "1")
        for rx, wg in (("8", "1"), ("4", "1"), ("8", "4"), ("4", "2")):
            _native.set_option("SSAMD_ASW_WAVE_RX", rx); _native.set_option("SSAMD_ASW_WAVE_WG", wg)
            assert torch.equal(m.compute(tL, tR), want), (rx, wg)
        _native.set_option("SSAMD_ASW_WAVE_UNROLL", "0")
        assert torch.equal(m.compute(tL, tR), want)
    finally:
        for k in ("SSAMD_ASW_WAVE", "SSAMD_ASW_WAVE_RX", "SSAMD_ASW_WAVE_WG", "SSAMD_ASW_WAVE_UNROLL"):
            _native.set_option(k, None)


def test_asw_wave_kernel_strips_and_alternate_rows(ss, golden_inputs):
    """the wave kernel under the other entry points: a row strip with its halo equals the rows of the whole frame, the
    alternate-rows mode and the separate argmins equal those computed with the workgroup kernels"""
    from simplestereo_amd import _native
    import torch
    a, b = golden_inputs("synth_96x128")
    tL, tR = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    m = ss.passive.StereoASW(winSize=13, maxDisparity=16, consistent=True)
    alt = ss.passive.StereoASW(winSize=13, maxDisparity=16, alternate=True)
    try:
        _native.set_option("SSAMD_ASW_WAVE", "0")
        want, want_alt = m.compute(tL, tR), alt.compute(tL, tR)
        want_strip = m._compute_device(tL[20:70].contiguous(), tR[20:70].contiguous(), out_row0=6, out_rows=38)
        _native.set_option("SSAMD_ASW_WAVE", "1")
        for rx in ("8", "4"):
            _native.set_option("SSAMD_ASW_WAVE_RX", rx)
            assert _native.asw_kernel_form(128, 96, 13, 16, 0)["wave_kernel"] == int(rx)
            assert torch.equal(m.compute(tL, tR), want)
            assert torch.equal(alt.compute(tL, tR), want_alt)
            got_strip = m._compute_device(tL[20:70].contiguous(), tR[20:70].contiguous(), out_row0=6, out_rows=38)
            assert torch.equal(got_strip, want_strip)
            assert torch.equal(got_strip, want[26:64])
    finally:
        for k in ("SSAMD_ASW_WAVE", "SSAMD_ASW_WAVE_RX"):
            _native.set_option(k, None)


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


def test_autotune_changes_the_geometry_never_the_map(ss, golden_inputs):
    """with autotuning on, the first call of a shape times ~10 candidate geometries (8- and 4-column tiles, chunked
    and unchunked, key path and direct path) on the call's buffers; the map must be the one of the model's choice"""
    a, b = golden_inputs("synth_96x128")
    cases = [dict(winSize=21, maxDisparity=39), dict(winSize=35, maxDisparity=16, consistent=True),
             dict(winSize=9, maxDisparity=70, minDisparity=3), dict(winSize=15, maxDisparity=24, alternate=True)]
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
    _native.set_option("SSAMD_ASW_GEOM", "3,5,8")           # an unrelated forced geometry computes the same maps
    try:
        forced = [ss.passive.StereoASW(**p).compute(a2, b2) for p in cases]
    finally:
        _native.set_option("SSAMD_ASW_GEOM", None)
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
    assert _native.asw_kernel_form(300, 40, 35, 70, 0)["phase_shifted"] == 1
    want = m.compute(tL, tR)
    n0 = _native.counter("evol_fallbacks")
    with _native.options(SSAMD_ASW_EVOL_FAIL="1"):
        got = m.compute(tL, tR)
        assert torch.equal(got, want)
        assert _native.counter("evol_fallbacks") == n0 + 1
        # the small-range wave kernel cannot run without its volume: the call falls back to the workgroup geometry stored
        # next to the wave geometry (round 5; a clean error until round 4) -- same map, the fallback counted, no stale HIP
        # error afterwards; a first call of a shape under the tuner simply ends up on a workgroup candidate
        small = ss.passive.StereoASW(winSize=35, maxDisparity=16)
        prev = _native.lib().ssamd_autotune(0)
        try:
            n1 = _native.counter("evol_fallbacks")
            untuned = small.compute(tL, tR)
            assert _native.counter("evol_fallbacks") > n1
        finally:
            _native.lib().ssamd_autotune(prev)
        tuned = small.compute(tL, tR)
        assert torch.equal(untuned, tuned)
    n2 = _native.counter("evol_fallbacks")
    assert torch.equal(small.compute(tL, tR), tuned)          # same map from the wave kernel once the volume can be had again
    assert torch.equal(m.compute(tL, tR), want)
    assert _native.counter("evol_fallbacks") == n2 and _native.counter("evol_bytes") > 0
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
    m = ss.passive.StereoASW(winSize=35, maxDisparity=maxd, consistent=consistent)

    def costs():
        c = np.empty((H, W, maxd + 1), np.float32)
        _native.check(_native.lib().ssamd_asw_costs(L.ctypes.data, R.ctypes.data, H, W, 35, maxd, 0, 5.0, 17.5, c.ctypes.data, -1))
        return c
    with _native.options(SSAMD_ASW_TAIL="0", SSAMD_AUTOTUNE="0"):
        n0 = _native.counter("tail_splits")
        want = m.compute(tL, tR)
        cw = costs() if not consistent else None
        assert _native.counter("tail_splits") == n0
    opts = dict(SSAMD_AUTOTUNE="0")
    if force:
        opts["SSAMD_ASW_TAIL"] = force
    with _native.options(**opts):
        n0 = _native.counter("tail_splits")
        got = m.compute(tL, tR)
        assert _native.counter("tail_splits") == n0 + 1, "the split did not happen: the test does not test it"
        if cw is not None:
            assert np.array_equal(costs(), cw, equal_nan=True)
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


@pytest.mark.parametrize("win,maxd,mind,consistent", [(35, 16, 0, False), (35, 16, 0, True), (15, 17, 0, True), (7, 21, 5, False), (63, 18, 2, True),
                                                       (11, 22, 5, True)])
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
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, minDisparity=mind, consistent=consistent, gammaC=6.0)

    def run(L, R):
        H, W = L.shape[:2]
        c = np.empty((H, W, nD), np.float32)
        _native.check(_native.lib().ssamd_asw_costs(L.ctypes.data, R.ctypes.data, H, W, win, maxd, mind, 6.0, 17.5, c.ctypes.data, -1))
        return m.compute(L, R), c
    try:
        _native.set_option("SSAMD_ASW_WAVE", "0")
        want = [run(L, R) for L, R in pairs]
        _native.set_option("SSAMD_ASW_WAVE", "1")
        _native.set_option("SSAMD_ASW_WAVE_RX", "4")
        if _native.asw_kernel_form(700, 37, win, maxd, mind)["wave_kernel"] != 4:
            pytest.skip("the 4-column tile does not fit LDS for this window")
        assert _native.asw_geometry(700, 37, win, maxd, mind)["chunk_d"] == 18          # three groups of six
        six = [run(L, R) for L, R in pairs]
        _native.set_option("SSAMD_ASW_WAVE_RD", "4")
        assert _native.asw_geometry(700, 37, win, maxd, mind)["chunk_d"] == 20          # five groups of four
        four = [run(L, R) for L, R in pairs]
        for (wd, wc), (sd, sc), (fd, fc) in zip(want, six, four):
            assert np.array_equal(sd, wd) and np.array_equal(fd, wd)
            assert np.array_equal(sc, wc, equal_nan=True) and np.array_equal(fc, wc, equal_nan=True)
    finally:
        for k in ("SSAMD_ASW_WAVE", "SSAMD_ASW_WAVE_RX", "SSAMD_ASW_WAVE_RD"):
            _native.set_option(k, None)


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
    nD = maxd - mind + 1
    c = np.empty((H, W, nD), np.float32)
    _native.check(_native.lib().ssamd_asw_costs(L.ctypes.data, R.ctypes.data, H, W, win, maxd, mind, 7.0, 40.0, c.ctypes.data, -1))
    assert np.array_equal(np.isnan(c), np.isnan(cref))
    ok = ~np.isnan(cref)
    assert (np.abs(c[ok] - cref[ok]) / np.maximum(1.0, np.abs(cref[ok]))).max() <= 1e-4
    diff = np.abs(d.astype(np.int32) - ref.astype(np.int32))
    print("win %d: exact %.4f within-1 %.4f" % (win, np.mean(diff == 0), np.mean(diff <= 1)))
    assert np.mean(diff <= 1) >= 0.995 and np.mean(diff == 0) >= 0.99
    if win <= 127:          # (the closed-form oracle needs seconds for these; the literal relaxation would need hours)
        g = dict(winSize=win, maxDisparity=maxd, minDisparity=mind, gamma=10, fMax=120, iterations=3)
        assert np.array_equal(ss.passive.StereoGSW(**g).compute(L, R), oracle.gsw(L, R, closed=True, **g))
