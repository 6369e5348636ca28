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

import _asw_forms as F

pytestmark = pytest.mark.gpu

WORKERS = (1, 5, 16)

# name -> tile (_asw_forms.PIPE_TILES: 8 XG columns x 4 DG disparities, tap-column chunks), H, W, win, minD, maxD, consistent, tiles, disparity chunks
CASES = {
    "120x196-3-tiles": ("120x196", 40, 250, 35, 0, 192, False, 3, 1),        # nx & 7 != 0: no tile remap; partial last tile
    "120x196-8-tiles": ("120x196", 12, 960, 35, 0, 192, False, 8, 1),        # the remap branch
    "generic-merging": ("48x36", 24, 100, 35, 0, 35, True, 3, 1),            # keys, atomicMin, right-referenced pass
    "two-chunks": ("120x100", 16, 250, 35, 0, 192, False, 3, 2),             # the disparity chunk comes from the item
}


def _form(name, persist):
    """the case's tile with the persistent form forced to `persist` workers (0: the plain launch), as (form, W, H, params)"""
    tile, H, W, win, mind, maxd, cons, tiles, chunks = CASES[name]
    p = dict(winSize=win, maxDisparity=maxd, minDisparity=mind, gammaC=5.0, gammaP=17.5)
    return F.also(F.pipe_tile(*F.PIPE_TILES[tile], persist=persist), grid_x=tiles, n_chunks=chunks), W, H, p


def forced_rows():
    return [_form(name, persist) for name in CASES for persist in (0,) + WORKERS]


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


def _run(ss, name, persist, exact=False):
    """(map, raw costs) of the case with the form forced to `persist`; with a worker count, the finished-item counter is checked
    behind each of the two launches"""
    tile, H, W, win, mind, maxd, cons, tiles, chunks = CASES[name]
    L, R = _images(H, W)
    p = _form(name, 0)[3]
    m = ss.passive.StereoASW(consistent=cons, exact=exact, **p)
    # first other images through the plain launch: the context's device buffers (map, keys, cost volume) are reused from call to
    # call, and a tile the launch under test missed must not find an earlier run's correct values there
    with F.forced(*_form(name, 0)):
        L2, R2 = _images(H, W, seed=12)
        m.compute(L2, R2)
        F.cost_dump(L2, R2, p)
    grown = []
    with F.forced(*_form(name, persist)):
        for launch in (lambda: m.compute(L, R), lambda: F.cost_dump(L, R, p)):
            with F.counted("pipe_persist_items") as n, F.counted("pipe_persist_launches") as ln:
                out = launch()
            grown += [out, (n.delta, ln.delta)]
        entries = _native.counter("exact_entries") if exact else None
    disp, first, costs, second = grown
    items = tiles * H * chunks
    want = (items, 1) if persist else (0, 0)
    assert first == want and second == want, (name, persist, items, first, second)
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
    assert F.same_costs(got_c, want_c) == 0, (name, workers, F.same_costs(got_c, want_c))


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
    tile, H, W, win, mind, maxd, cons, tiles, chunks = CASES[name]
    L, R = _images(H, W)
    tL, tR = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
    m = ss.passive.StereoASW(consistent=cons, exact=False, **_form(name, 0)[3])
    row0, rows, skip0, nskip = 3, H - 7, 12, 13
    a, b = skip0 - row0, skip0 - row0 + nskip
    with F.forced(*_form(name, 0)):
        want = m._compute_device(tL, tR, out_row0=row0, out_rows=rows)
    with F.forced(*_form(name, workers)):
        out = torch.full((rows, W), -7, dtype=torch.int16, device="cuda")
        with F.counted("pipe_persist_items") as n:
            m._compute_device(tL, tR, out_row0=row0, out_rows=rows, out=out, skip=(skip0, nskip))
    assert n.delta == tiles * (rows - nskip) * chunks, (workers, n.delta)
    assert torch.equal(out[:a], want[:a]) and torch.equal(out[b:], want[b:]), workers
    assert bool((out[a:b] == -7).all()), "rows between the two ranges were written"
