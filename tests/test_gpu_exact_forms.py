"""GPU tier: the fp64 tie-break pass (exact mode, the default) of EVERY kernel form and entry point, on tie-rich inputs.

The form tests of test_gpu_asw.py compare one form's map with another's on make_pair frames, where the fp32 argmin is the fp64
one almost everywhere: a form whose near-tie epilogue (asw_exact_select / asw_exact_merge) queues nothing, or queues the wrong
pixel, passes them.  Here every form runs on inputs of tests/_tie_inputs.py (hundreds of pixels whose best two fp64 costs lie
below fp32 resolution: test_tie_inputs_cpu.py) and, plain and consistent, must (1) really run -- its geometry or a counter says
so --, (2) return the fp64 oracle's map bit for bit without a queue overflow, and (3) have teeth: under the same options the
fp32 map alone (exact=False) differs from the oracle somewhere, and in consistent mode right-referenced pixels get flagged.
Inputs and oracle maps are shared by the forms (one oracle call per input and parameters).  Last: a lone zero-cost winner whose
fp64 cost exceeds a rival's tiny positive cost (rule (d) of exact_near)."""
import os

import numpy as np
import pytest

import _asw_forms as F
import _tie_inputs as T

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OC = T.OracleCache()


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import simplestereo_amd
    return simplestereo_amd


def _n(native):
    return {k: native.counter(k) for k in ("exact_overflow", "exact_entries", "exact_flagged_left", "exact_flagged_right")}


def _case(ss, tag, L, R, p, form):
    """one (input, params) under `form` (of _asw_forms; bare options force no kernel form): the default map is the oracle's;
    returns (n32, flagged right)"""
    from simplestereo_amd import _native
    H, W = L.shape[:2]
    with (_native.options(**form) if isinstance(form, dict) else F.forced(form, W, H, p)):
        d = ss.passive.StereoASW(**p).compute(L, R)
        c = _n(_native)
        d32 = ss.passive.StereoASW(exact=False, **p).compute(L, R)
    ref = OC.asw(L, R, **p)
    n64, n32 = int(np.count_nonzero(d != ref)), int(np.count_nonzero(d32 != ref))
    print("%-34s %-26s cons=%d  n32 %5d  n64 %d  entries %7d  flagged L %5d R %5d" %
          (tag, "%dx%d w%d D%d gC%g" % (W, H, p["winSize"], p["maxDisparity"], p["gammaC"]), p["consistent"], n32, n64,
           c["exact_entries"], c["exact_flagged_left"], c["exact_flagged_right"]))
    assert c["exact_overflow"] == 0, tag
    assert n64 == 0, (tag, p, n64, n32)
    return n32, c["exact_flagged_right"]


def _matrix(ss, tag, form, inputs):
    """every input, plain and consistent; the teeth of the form"""
    n32, fr = 0, 0
    for kind, H, W, p in inputs:
        L, R = T.pair(kind, H, W, p["maxDisparity"], seed=3)
        for cons in (False, True):
            a, b = _case(ss, tag, L, R, dict(p, consistent=cons, minDisparity=p.get("minDisparity", 0), gammaP=17.5), form)
            n32 += a
            fr = max(fr, b) if cons else fr
    assert n32 > 0, ("no case of this form has a pixel where the fp32 map differs from the oracle: the case has no teeth", tag)
    assert fr > 0, ("consistent mode flagged no right-referenced pixel", tag)


def _inputs(win, maxd, H=24, W=128):
    return [("quantised", H, W, dict(winSize=win, maxDisparity=maxd, gammaC=0.7)),
            ("black_margins", H, W, dict(winSize=win, maxDisparity=maxd, gammaC=5.0)),
            ("patches", H, W, dict(winSize=win, maxDisparity=maxd, gammaC=0.7))]


# ---- workgroup kernel (asw_aggregate_kernel): 8- / 4-column tiles, whole window rows and chunks of 4 / 8 / 16, one e tile, XOR rows
WORKGROUP = [("6,5,0,8", 8, 0, {}), ("6,5,8,8", 8, 8, {}), ("10,9,16,8", 8, 16, {}), ("12,5,0,4", 4, 0, {}), ("7,9,8,4", 4, 8, {}),
             ("20,3,4,4", 4, 4, {}), ("6,5,8,8", 8, 8, dict(SSAMD_ASW_NO_E2="1")),
             ("6,5,8,8", 8, 8, dict(SSAMD_ASW_NO_E2="1", SSAMD_ASW_XOR_ONLY="1"))]


def _workgroup(geom, rx, jc, extra):
    return F.also(F.workgroup_tile(geom, **extra), tile_columns=rx, chunk_columns=jc), _inputs(21, int(geom.split(",")[1]) * 4 - 1)


@pytest.mark.parametrize("geom,rx,jc,extra", WORKGROUP)
def test_workgroup_kernel(geom, rx, jc, extra, ss):
    _matrix(ss, "workgroup %s %s" % (geom, extra), *_workgroup(geom, rx, jc, extra))


# ---- phase-shifted kernel (asw_aggregate_pipe_kernel): chunks of 8 / 16, wave order, TAD volume or in-kernel e tiles
PIPE = [("6,5,0,8", 21, "8", "0", {}), ("6,5,0,8", 21, "8", "1", {}), ("10,9,0,8", 35, "16", "0", {}), ("10,9,0,8", 35, "16", "1", {}),
        ("6,5,0,8", 21, "8", "1", dict(SSAMD_ASW_EVOL="0")), ("10,9,0,8", 35, "16", "0", dict(SSAMD_ASW_EVOL="0")),
        ("6,5,0,8", 21, "8", "1", dict(SSAMD_ASW_EVOL_MAX_MB="1"))]


def _pipe(geom, win, jc, dephase, extra):
    XG, DG = (int(v) for v in geom.split(",")[:2])
    return F.pipe_tile(XG, DG, int(jc), dephase=dephase, **extra), _inputs(win, DG * 4 - 2, H=16)


@pytest.mark.parametrize("geom,win,jc,dephase,extra", PIPE)
def test_phase_shifted_kernel(geom, win, jc, dephase, extra, ss):
    _matrix(ss, "phase-shifted %s JC %s dephase %s %s" % (geom, jc, dephase, extra), *_pipe(geom, win, jc, dephase, extra))


TAIL = F.pipe_tile(4, 5, 8, SSAMD_ASW_TAIL="1", SSAMD_AUTOTUNE="0")
TAIL_PARAMS = dict(winSize=13, maxDisparity=19, minDisparity=0, gammaC=0.7, gammaP=17.5)
TAIL_ROWS = range(32, 689, 8)


def test_half_width_tail_tiles(ss):
    """SSAMD_ASW_TAIL=1: the smallest row count (8-row steps) whose launch has a last round at most half full on this device"""
    p, W, found = TAIL_PARAMS, 128, None
    for H in TAIL_ROWS:
        L, R = T.pair("quantised", H, W, p["maxDisparity"], seed=3)
        with F.forced(TAIL, W, H, p), F.counted("tail_splits") as n:
            ss.passive.StereoASW(**p).compute(L, R)
        if n.delta == 1:
            found = H
            break
    assert found is not None, "no launch of up to 688 rows split its last round: the tail tiles were not tested"
    L, R = T.pair("quantised", found, W, p["maxDisparity"], seed=3)
    n32 = 0
    for cons in (False, True):
        with F.forced(TAIL, W, found, p), F.counted("tail_splits") as n:
            a, _ = _case(ss, "tail tiles (%d rows)" % found, L, R, dict(p, consistent=cons), {})
            assert n.delta >= 1
        n32 += a
    assert n32 > 0


# ---- wave kernel (asw_aggregate_wave_kernel): register tiles, merged build rounds, waves per workgroup, unrolling
WAVE = [("8", {}, 128, None), ("4", {}, 128, None), ("8", dict(SSAMD_ASW_WAVE_MERGE="0"), 128, None),
        ("4", dict(SSAMD_ASW_WAVE_MERGE="0"), 128, None), ("8", dict(SSAMD_ASW_WAVE_WG="2"), 1000, 128),
        ("4", dict(SSAMD_ASW_WAVE_WG="4"), 1000, 256), ("8", dict(SSAMD_ASW_WAVE_UNROLL="0"), 128, None)]


def _wave(rx, extra, W, threads):
    form = F.wave(rx, **extra)
    return F.also(form, threads=threads) if threads else form, _inputs(9, 15, H=8 if W >= 1000 else 24, W=W)


@pytest.mark.parametrize("rx,extra,W,threads", WAVE)
def test_wave_kernel(rx, extra, W, threads, ss):
    _matrix(ss, "wave RX %s %s" % (rx, extra), *_wave(rx, extra, W, threads))


WAVE6 = [(16, None, 18), (17, None, 18), (17, "4", 20)]


def _wave6(maxd, rd, chunk):
    return F.also(F.wave(4, SSAMD_ASW_WAVE_RD=rd), chunk_d=chunk), _inputs(9, maxd)


@pytest.mark.parametrize("maxd,rd,chunk", WAVE6)
def test_wave6_kernel(maxd, rd, chunk, ss):
    """17 / 18 disparities: three groups of six per lane (asw_aggregate_wave6_kernel); WAVE_RD=4: five groups of four"""
    _matrix(ss, "wave6 D%d RD %s" % (maxd, rd), *_wave6(maxd, rd, chunk))


CHUNKS = (({}, dict(n_chunks=lambda n: n > 1)), [("quantised", 8, 600, dict(winSize=5, maxDisparity=530, gammaC=0.7)),
                                                ("black_margins", 8, 600, dict(winSize=5, maxDisparity=530, gammaC=5.0))])


def test_disparity_range_over_several_chunks(ss):
    """531 disparities: several chunks merged by atomics (a merging call also without a right pass)"""
    _matrix(ss, "531 disparities", *CHUNKS)


def test_window_of_65_on_black_margins(ss):
    """windows of 64 and more bypass asw_exact_zero_kernel's LDS tiles (EXACT_ZWIN_MAX): zero-cost pixels are escalated"""
    _matrix(ss, "window 65", {}, [("black_margins", 20, 120, dict(winSize=65, maxDisparity=8, gammaC=5.0)),
                                 ("quantised", 20, 120, dict(winSize=65, maxDisparity=8, gammaC=0.7))])


# ---- entry points and record producers at their default forms -----------------------------------------------------------------
def test_prepass_unfused(ss):
    """SSAMD_ASW_PREPASS_FUSE=0: the records come from asw_prepass_kernel instead of bgr2lab_records_pair_kernel"""
    _matrix(ss, "prepass unfused", dict(SSAMD_ASW_PREPASS_FUSE="0"), _inputs(15, 40, H=16, W=200))
    _matrix(ss, "prepass fused (default)", {}, _inputs(15, 40, H=16, W=200))


@pytest.mark.parametrize("cons", [False, True])
def test_strip_with_halo_and_two_range_launch(cons, ss):
    """_compute_device on a row strip (out_row0 > 0, halo rows either side), and the same strip with skip = (row, n): the
    rows written are the oracle's rows of the whole frame, the skipped ones are left untouched"""
    import torch
    from simplestereo_amd import _native
    H, W, p = 48, 128, dict(winSize=15, maxDisparity=31, minDisparity=0, gammaC=0.7, gammaP=17.5, consistent=cons)
    n32 = 0
    for kind in ("quantised", "black_margins"):
        L, R = T.pair(kind, H, W, p["maxDisparity"], seed=3)
        ref = OC.asw(L, R, **p)
        m = ss.passive.StereoASW(**p)
        tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        pad, r0, r1 = 7, 13, 37
        h0, h1 = r0 - pad, min(H, r1 + pad)
        a, b = tL[h0:h1].contiguous(), tR[h0:h1].contiguous()
        got = m._compute_device(a, b, out_row0=r0 - h0, out_rows=r1 - r0).cpu().numpy()
        assert _native.counter("exact_overflow") == 0
        assert np.array_equal(got, ref[r0:r1]), (kind, int(np.count_nonzero(got != ref[r0:r1])))
        out = torch.full((r1 - r0, W), -12345, dtype=torch.int16, device="cuda")
        m._compute_device(a, b, out_row0=r0 - h0, out_rows=r1 - r0, out=out, skip=(r0 - h0 + 5, 9))       # (rows of the sub-image)
        o = out.cpu().numpy()
        assert _native.counter("exact_overflow") == 0
        keep = np.ones(r1 - r0, bool); keep[5:14] = False
        assert np.all(o[~keep] == -12345)
        assert np.array_equal(o[keep], ref[r0:r1][keep]), (kind, int(np.count_nonzero(o[keep] != ref[r0:r1][keep])))
        n32 += int(np.count_nonzero(ss.passive.StereoASW(exact=False, **p).compute(L, R)[r0:r1] != ref[r0:r1]))
    print("strips cons=%d: fp32 map differs from the oracle on %d strip pixels" % (cons, n32))
    assert n32 > 0


@pytest.mark.parametrize("cons", [False, True])
def test_fused_rectify_path(cons, ss):
    """compute(raw, raw, rectify=rig): remap_lab_records_pair_kernel writes the records; the map is the oracle's on the host
    rectification (whose black margins make it tie-rich)"""
    import torch
    rig = ss.RectifiedStereoRig.fromFile(os.path.join(G, "rig_example2_rigRect.json"))
    rig.computeRectificationMaps(destDims=(161, 91))
    w, h = rig.res1
    L, R = T.pair("quantised", h, w, 30, seed=3)
    hL, hR = rig.rectifyImages(L, R)
    hL, hR = np.ascontiguousarray(hL), np.ascontiguousarray(hR)
    p = dict(winSize=11, maxDisparity=30, minDisparity=0, gammaC=0.7, gammaP=17.5, consistent=cons)
    ref = OC.asw(hL, hR, **p)
    m = ss.passive.StereoASW(**p)
    got = m.compute(torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda(), rectify=rig).cpu().numpy()
    from simplestereo_amd import _native
    assert _native.counter("exact_overflow") == 0
    n32 = int(np.count_nonzero(ss.passive.StereoASW(exact=False, **p).compute(hL, hR) != ref))
    print("fused rectify cons=%d: n32 %d, n64 %d" % (cons, n32, int(np.count_nonzero(got != ref))))
    assert np.array_equal(got, ref)
    assert n32 > 0


def test_autotune_first_and_cached_call(ss):
    """SSAMD_AUTOTUNE=1 on shapes no other test uses: the first call times trial launches (without the queue), then runs with
    it; the second call takes the cached geometry"""
    n32, fr = 0, 0
    for kind, H, W in (("quantised", 23, 131), ("black_margins", 21, 133)):
        L, R = T.pair(kind, H, W, 35, seed=3)
        for cons in (False, True):
            p = dict(winSize=17, maxDisparity=35 + cons, minDisparity=0, gammaC=0.7, gammaP=17.5, consistent=cons)
            for call in ("first", "cached"):
                a, b = _case(ss, "autotune %s" % call, L, R, p, dict(SSAMD_AUTOTUNE="1"))
                n32 += a
                fr = max(fr, b)
    assert n32 > 0 and fr > 0


def test_devices_listed_twice(ss):
    """devices=[0, 0] (test hook SSAMD_MULTI_ALLOW_REPEAT): one strip per listed device, each tie-broken on its own"""
    from simplestereo_amd import _native
    n32 = 0
    for kind in ("quantised", "black_margins"):
        L, R = T.pair(kind, 40, 128, 31, seed=3)
        for cons in (False, True):
            p = dict(winSize=15, maxDisparity=31, minDisparity=0, gammaC=0.7, gammaP=17.5, consistent=cons)
            with _native.options(SSAMD_MULTI_ALLOW_REPEAT="1"):
                got = ss.passive.StereoASW(**p).compute(L, R, devices=[0, 0])
            ref = OC.asw(L, R, **p)
            assert np.array_equal(got, ref), (kind, cons, int(np.count_nonzero(got != ref)))
            n32 += int(np.count_nonzero(ss.passive.StereoASW(exact=False, **p).compute(L, R) != ref))
    assert n32 > 0


# ---- a lone zero-cost winner (rule (d) of exact_near) --------------------------------------------------------------------------
LONE_FORMS = [("wave",) + F.wave(8), ("workgroup",) + F.workgroup_tile("4,5,0,8"), ("phase-shifted",) + F.pipe_tile(4, 5, 8)]


@pytest.mark.parametrize("name,opts,want", LONE_FORMS)
def test_lone_zero_cost_winner(name, opts, want, ss):
    """tests/_tie_inputs.py::lone_zero_pair: at pixel X the fp32 costs have exactly one 0, at D0 (every weight of its TAD-40 tap
    flushed), and the reference picks D1, whose tiny positive cost lies ~1e7 cost-image ulps above 0 -- far outside rule (a)'s
    band at a winner of 0.  Rule (d) (exact_zkey) queues it; the map is the oracle's, plain and consistent."""
    from oracle import oracle
    from simplestereo_amd import _native
    L, R, p = T.lone_zero_pair()
    H, W = L.shape[:2]
    x, d0, d1 = T.LZ_X, T.LZ_D0, T.LZ_D1
    row = F.cost_dump(L, R, p)[0, x]
    _, c64 = oracle.asw(L, R, return_costs=True, **p)
    tol = T.tol(p["winSize"], p["gammaC"])
    print("lone zero: fp32 costs at X: D0 %r, D1 %r (image %d ulps above 0, tol %d); fp64: D0 %r, D1 %r" %
          (float(row[d0]), float(row[d1]), int(row[d1:d1 + 1].view(np.uint32)[0]), tol, c64[0, x, d0], c64[0, x, d1]))
    assert row[d0] == 0.0 and np.count_nonzero(row == 0.0) == 1                       # (a)
    assert 0.0 < c64[0, x, d1] < c64[0, x, d0] and int(np.argmin(c64[0, x])) == d1     # (b)
    assert int(row[d1:d1 + 1].view(np.uint32)[0]) > tol                                 # (c)
    for cons in (False, True):
        q = dict(p, consistent=cons)
        ref = oracle.asw(L, R, **q)
        with F.forced(opts, W, H, q, want):
            d = ss.passive.StereoASW(**q).compute(L, R)
            assert _native.counter("exact_overflow") == 0
            d32 = ss.passive.StereoASW(exact=False, **q).compute(L, R)
        if not cons:
            assert int(d32[0, x]) == d0                                                 # the fp32 argmin alone is wrong here
            assert int(d[0, x]) == int(ref[0, x]) == d1, (name, int(d[0, x]))
        assert np.array_equal(d, ref), (name, cons, np.argwhere(d != ref).tolist())


def forced_rows():
    """every forced form of this file, as (form, W, H, params): tests/test_asw_forms_cpu.py asks the planner for each"""
    rows = []
    for form, inputs in ([_workgroup(*r) for r in WORKGROUP] + [_pipe(*r) for r in PIPE] + [_wave(*r) for r in WAVE] +
                         [_wave6(*r) for r in WAVE6] + [CHUNKS]):
        rows += [(form, W, H, p) for _, H, W, p in inputs]
    rows += [(TAIL, 128, H, TAIL_PARAMS) for H in TAIL_ROWS]
    L, _, p = T.lone_zero_pair()
    return rows + [((opts, want), L.shape[1], L.shape[0], p) for _, opts, want in LONE_FORMS]
