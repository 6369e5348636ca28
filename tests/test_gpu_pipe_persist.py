"""Tier T2 (GPU): the persistent form of asw_aggregate_pipe_kernel (SSAMD_ASW_PERSIST) against the plain launch of the same tiles.

In the persistent form a few workgroups draw the launch's tiles as work items from eight queues instead of one workgroup per
tile.  An item runs the instructions of the workgroup it replaces, so the fp32 argmin map and the raw cost volume must be equal
BIT FOR BIT with the form off: there is no tolerance in this file.  Worker counts: 1 (one workgroup walks all eight queues),
5 (queues without a worker of their own are drained only by workgroups that exhausted theirs; no multiple of 8) and 16.  After
every forced launch the device-side counter of finished items must have grown by exactly tiles x rows x disparity chunks: every
item was done, and done once."""
import numpy as np
import pytest
from simplestereo_amd import _native

pytestmark = pytest.mark.gpu

HOOKS = ("SSAMD_ASW_GEOM", "SSAMD_ASW_PIPE", "SSAMD_ASW_WAVE", "SSAMD_ASW_PERSIST")
WORKERS = (1, 5, 16)

# name -> XG, DG, JC (tile of 8 XG columns x 4 DG disparities, tap-column chunks), H, W, win, minD, maxD, consistent, tiles, disparity chunks
CASES = {
    "120x196-3-tiles": (15, 49, 16, 40, 250, 35, 0, 192, False, 3, 1),       # nx & 7 != 0: no tile remap; partial last tile
    "120x196-8-tiles": (15, 49, 16, 12, 960, 35, 0, 192, False, 8, 1),       # the remap branch
    "generic-merging": (6, 9, 8, 24, 100, 35, 0, 35, True, 3, 1),            # keys, atomicMin, right-referenced pass
    "two-chunks": (15, 25, 16, 16, 250, 35, 0, 192, False, 3, 2),            # the disparity chunk comes from the item
}


@pytest.fixture(scope="module")
def ss():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    import simplestereo_amd
    assert _native.lib().ssamd_device_count() >= 1
    return simplestereo_amd


def _images(H, W, seed=11):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _force(name, persist):
    XG, DG, JC, H, W, win, mind, maxd, cons, tiles, chunks = CASES[name]
    _native.set_option("SSAMD_ASW_WAVE", "0")
    _native.set_option("SSAMD_ASW_GEOM", "%d,%d" % (XG, DG))
    _native.set_option("SSAMD_ASW_PIPE", str(JC))
    _native.set_option("SSAMD_ASW_PERSIST", str(persist))
    form, geom = _native.asw_kernel_form(W, H, win, maxd, mind), _native.asw_geometry(W, H, win, maxd, mind)
    assert form["phase_shifted"] == 1 and form["chunk_columns"] == JC and form["wave_kernel"] == 0, form
    assert geom["tile_x"] == 8 * XG and geom["chunk_d"] == 4 * DG and geom["grid_x"] == tiles and geom["n_chunks"] == chunks, geom


def _unforce():
    for k in HOOKS:
        _native.set_option(k, None)


def _run(ss, name, persist, exact=False):
    """(map, raw costs) of the case with the form forced to `persist`; with a worker count, the finished-item counter is checked
    behind each of the two launches"""
    XG, DG, JC, H, W, win, mind, maxd, cons, tiles, chunks = CASES[name]
    L, R = _images(H, W)
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, minDisparity=mind, consistent=cons, exact=exact, gammaC=5.0, gammaP=17.5)
    costs = np.empty((H, W, maxd - mind + 1), np.float32)
    try:
        # first other images through the plain launch: the context's device buffers (map, keys, cost volume) are reused from call to
        # call, and a tile the launch under test missed must not find an earlier run's correct values there
        _force(name, 0)
        L2, R2 = _images(H, W, seed=12)
        m.compute(L2, R2)
        _native.check(_native.lib().ssamd_asw_costs(L2.ctypes.data, R2.ctypes.data, H, W, win, maxd, mind, m.gammaC, m.gammaP, costs.ctypes.data, -1))
        costs.fill(np.float32(-3.0))
        _force(name, persist)
        n0, l0 = _native.counter("pipe_persist_items"), _native.counter("pipe_persist_launches")
        disp = m.compute(L, R)
        n1, l1 = _native.counter("pipe_persist_items"), _native.counter("pipe_persist_launches")
        _native.check(_native.lib().ssamd_asw_costs(L.ctypes.data, R.ctypes.data, H, W, win, maxd, mind, m.gammaC, m.gammaP, costs.ctypes.data, -1))
        n2, l2 = _native.counter("pipe_persist_items"), _native.counter("pipe_persist_launches")
        entries = _native.counter("exact_entries") if exact else None
    finally:
        _unforce()
    items = tiles * H * chunks
    want = (items, 1) if persist else (0, 0)
    assert (n1 - n0, l1 - l0) == want and (n2 - n1, l2 - l1) == want, (name, persist, items, n0, n1, n2, l0, l1, l2)
    return disp, costs, entries


_plain = {}


def _plain_run(ss, name, exact=False):
    if (name, exact) not in _plain:
        _plain[(name, exact)] = _run(ss, name, 0, exact)
    return _plain[(name, exact)]


@pytest.mark.parametrize("workers", WORKERS)
@pytest.mark.parametrize("name", list(CASES))
def test_persistent_form_equals_the_plain_launch(name, workers, ss):
    want, want_c, _ = _plain_run(ss, name)
    got, got_c, _ = _run(ss, name, workers)
    assert np.array_equal(got, want), (name, workers, int((got != want).sum()))
    nan = np.isnan(want_c)                  # (candidates the reference does not evaluate)
    differ = (got_c.view(np.uint32) != want_c.view(np.uint32)) & ~nan
    assert np.array_equal(np.isnan(got_c), nan) and not differ.any(), (name, workers, int(differ.sum()))


@pytest.mark.parametrize("workers", WORKERS)
def test_default_path_with_the_persistent_form(workers, ss):
    """exact="auto": the fp32 kernels queue their near-ties for the fp64 pass.  The order of the queue's entries may depend on the
    order the tiles ran in; their number and the final map may not."""
    name = "120x196-3-tiles"
    want, _, want_entries = _plain_run(ss, name, exact="auto")
    got, _, got_entries = _run(ss, name, workers, exact="auto")
    assert np.array_equal(got, want), (workers, int((got != want).sum()))
    assert got_entries == want_entries, (workers, got_entries, want_entries)


@pytest.mark.parametrize("workers", WORKERS)
def test_two_row_ranges_with_the_persistent_form(workers, ss):
    """ssamd_asw_device_rows2 (one launch over two row bands, tests/test_gpu_rows2.py): the workgroup row -> image row mapping with
    its gap is the item's"""
    import torch
    name = "120x196-3-tiles"
    XG, DG, JC, H, W, win, mind, maxd, cons, tiles, chunks = CASES[name]
    L, R = _images(H, W)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = ss.passive.StereoASW(winSize=win, maxDisparity=maxd, minDisparity=mind, consistent=cons, exact=False, gammaC=5.0, gammaP=17.5)
    row0, rows, skip0, nskip = 3, H - 7, 12, 13
    a, b = skip0 - row0, skip0 - row0 + nskip
    try:
        _force(name, 0)
        want = m._compute_device(tL, tR, out_row0=row0, out_rows=rows)
        _force(name, workers)
        out = torch.full((rows, W), -7, dtype=torch.int16, device="cuda")
        n0 = _native.counter("pipe_persist_items")
        m._compute_device(tL, tR, out_row0=row0, out_rows=rows, out=out, skip=(skip0, nskip))
        n1 = _native.counter("pipe_persist_items")
    finally:
        _unforce()
    assert n1 - n0 == tiles * (rows - nskip) * chunks, (workers, n0, n1)
    assert torch.equal(out[:a], want[:a]) and torch.equal(out[b:], want[b:]), workers
    assert bool((out[a:b] == -7).all()), "rows between the two ranges were written"
