"""GPU: ss.unwrapping.unwrap / unwrap2D (np_unwrap_row_kernel, np_unwrap_col_kernel) and ftpPhase(unwrap="numpy") against
np.unwrap as installed -- equal means same shape and dtype, NaN at the same positions and identical 64-bit patterns everywhere
else.  The shapes are aimed with the launch plan (ssamd_np_unwrap_plan): R samples per chunk of the row form, T rows per tile
and LANES columns per workgroup of the column form, each of them met one below, at and one above, and twice over."""
import ctypes
import os

import numpy as np
import pytest

import _np_unwrap_ref as R_

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
PI = np.pi


def _plan(outer, n, inner):
    from simplestereo_amd import _native
    return _native.np_unwrap_plan(outer, n, inner)


# Sizes are expressions in R (row form: samples per chunk), T and LANES (column form: rows per tile, columns per workgroup), read
# from the plan when a test runs: collecting this file loads no native library.
ROW_WIDTHS = ["1", "2", "63", "64", "65", "R - 1", "R", "R + 1", "2 * R + 1"]
COL_HEIGHTS = ["1", "2", "T - 1", "T", "T + 1", "2 * T + 1"]
COL_WIDTHS = ["1", "63", "65", "LANES + 1"]


class _Sizes:
    def __init__(self):
        col = _plan(1, 100, 3)
        self.R, self.T, self.LANES = _plan(3, 100, 1)["chunk"], col["chunk"], col["lanes"]

    def __call__(self, expr):
        return int(eval(expr, {"R": self.R, "T": self.T, "LANES": self.LANES}))


@pytest.fixture(scope="module")
def size():
    return _Sizes()


@pytest.fixture(scope="module")
def unwrapping():
    import torch
    assert torch.cuda.is_available()
    from simplestereo_amd import unwrapping
    return unwrapping


def _numpy(p, discont=None, axis=-1, period=2 * PI):
    with np.errstate(all="ignore"):
        return np.unwrap(p, discont=discont, axis=axis, period=period)


def _all_inputs(unwrapping, shape, axis, params=((None, 2 * PI),)):
    """Every input of tests/_np_unwrap_ref.py at this shape, on host arrays; the device tensor path on the first of them."""
    import torch
    for name, p in R_.inputs(shape, axis).items():
        for discont, period in params:
            want = _numpy(p, discont, axis, period)
            got = unwrapping.unwrap(p, discont=discont, axis=axis, period=period)
            assert got is not p and R_.equal(got, want), (shape, axis, name, discont, period,
                                                          R_.differing_fraction(got, want) if got.shape == want.shape else None)
            if name == "nonfinite":                          # the NaN tail by position, not only by comparison
                assert np.array_equal(np.isnan(got), R_.nan_tail_positions(p, axis)), (shape, axis, discont, period)
            if name == "steep_ramp":
                dev = unwrapping.unwrap(torch.from_numpy(p).cuda(), discont=discont, axis=axis, period=period)
                assert dev.is_cuda and dev.dtype == torch.float64 and R_.equal(dev.cpu().numpy(), want), (shape, axis, discont, period)


def test_plan_is_what_the_shapes_assume(size):
    R, T, LANES = size.R, size.T, size.LANES
    assert _plan(3, R, 1)["form"] == "row" and _plan(T, 1, 3)["form"] == "column"
    assert R >= 128 and T >= 16 and LANES >= 16
    # the steep ramp tells a sequential sum from a blocked one at the chunk sizes in use (asserted, not assumed)
    for shape, axis, block in (((3, 2 * R + 1), 1, R), ((2 * T + 1, 3), 0, T), ((3, 129), 1, 16), ((129, 3), 0, 16)):
        p = R_.steep_ramp(shape, axis)
        frac = R_.differing_fraction(R_.blocked_unwrap(p, block, axis), np.unwrap(p, axis=axis))
        print("blocks of %d differ from np.unwrap in %.1f %% of %s" % (block, 100 * frac, shape))
        assert frac >= 0.25


@pytest.mark.parametrize("w", ROW_WIDTHS)
def test_row_form_widths(unwrapping, size, w):
    w = size(w)
    assert _plan(3, w, 1)["form"] == "row"
    _all_inputs(unwrapping, (3, w), 1)


@pytest.mark.parametrize("h", COL_HEIGHTS)
def test_column_form_heights(unwrapping, size, h):
    h = size(h)
    assert _plan(1, h, 3)["form"] == "column"
    _all_inputs(unwrapping, (h, 3), 0)


@pytest.mark.parametrize("w", COL_WIDTHS)
def test_column_form_ragged_lane_groups(unwrapping, size, w):
    """Widths that leave the last lane group of a workgroup part-filled (a single column is a line of the row form)."""
    w, T, LANES = size(w), size.T, size.LANES
    plan = _plan(1, T + 1, w)
    assert plan["form"] == ("column" if w > 1 else "row") and (w == 1 or plan["groups"] == -(-w // LANES))
    _all_inputs(unwrapping, (T + 1, w), 0)


@pytest.mark.parametrize("shape,axis", [(("3", "R + 1"), 1), (("T + 1", "3"), 0)])
def test_discont_and_period(unwrapping, size, shape, axis):
    shape = tuple(size(e) for e in shape)
    _all_inputs(unwrapping, shape, axis, params=R_.PARAMS)


@pytest.mark.parametrize("axis", [0, 1, 2, -1, -3])
def test_three_dimensions_every_axis(unwrapping, size, axis):
    shape = (3, size.T + 2, size.LANES + 5)
    _all_inputs(unwrapping, shape, axis)


def test_one_dimension_and_non_contiguous_views(unwrapping, size):
    import torch
    R, T, LANES = size.R, size.T, size.LANES
    p = R_.steep_ramp((R + 7,), 0)
    assert R_.equal(unwrapping.unwrap(p), np.unwrap(p))
    big = R_.steep_ramp((2 * T + 4, 2 * LANES + 10), 0, seed=3)
    view = big[1::2, 3:-2]
    assert not view.flags["C_CONTIGUOUS"]
    for axis in (0, 1):
        want = np.unwrap(view, axis=axis)
        assert R_.equal(unwrapping.unwrap(view, axis=axis), want)
        t = torch.from_numpy(big).cuda()[1::2, 3:-2]
        assert not t.is_contiguous()
        assert R_.equal(unwrapping.unwrap(t, axis=axis).cpu().numpy(), want)
        assert R_.equal(unwrapping.unwrap(big.T, axis=axis), np.unwrap(big.T, axis=axis))


@pytest.mark.parametrize("shape", [("65", "129"), ("2", "33", "65"), ("T + 1", "R + 1")])
def test_unwrap2d_is_the_two_call_composition(unwrapping, size, shape):
    import torch
    shape = tuple(size(e) for e in shape)
    rng = np.random.default_rng(7)
    ramp = R_.steep_ramp(shape, len(shape) - 1, seed=1) + R_.steep_ramp(shape, len(shape) - 2, seed=2)
    for p in (np.angle(np.exp(1j * ramp)), rng.normal(0, 50, shape), R_.inputs(shape, len(shape) - 1)["nonfinite"]):
        want = _numpy(_numpy(p, PI, -1), PI, -2)
        got = unwrapping.unwrap2D(p)
        assert R_.equal(got, want)
        assert R_.equal(unwrapping.unwrap2D(torch.from_numpy(p).cuda()).cpu().numpy(), want)
        if p.ndim == 3:                                      # per map
            for k in range(p.shape[0]):
                assert R_.equal(unwrapping.unwrap2D(p[k]), want[k])
        assert R_.equal(unwrapping.unwrap(unwrapping.unwrap(p, discont=PI, axis=-1), discont=PI, axis=-2), want)


def test_device_entry_point_in_place(unwrapping, size):
    """include/ssamd.h allows d_out == d_p (ftpPhase's unwrap="numpy" runs both passes in the output buffer)."""
    import torch
    from simplestereo_amd import _native
    lib = _native.lib()
    R, T, LANES = size.R, size.T, size.LANES
    for shape, axis in (((3, 2 * R + 1), 1), ((2 * T + 1, LANES + 3), 0)):
        p = R_.steep_ramp(shape, axis)
        want = np.unwrap(p, axis=axis)
        t = torch.from_numpy(p).cuda()
        outer, n, inner = (shape[0], shape[1], 1) if axis == 1 else (1, shape[0], shape[1])
        stream = torch.cuda.current_stream().cuda_stream
        _native.check(lib.ssamd_np_unwrap_device(t.data_ptr(), outer, n, inner, PI, 2 * PI, t.data_ptr(), ctypes.c_void_p(stream)))
        torch.cuda.synchronize()
        assert R_.equal(t.cpu().numpy(), want)


def test_non_default_stream(unwrapping):
    """The call runs on the current stream: it is ordered behind the kernel that produced its input on that stream, and its
    result is complete once that stream is synchronised."""
    import torch
    p = R_.steep_ramp((300, 700), 1, seed=5)
    want_x, want_y, want_xy = np.unwrap(p, axis=1), np.unwrap(p, axis=0), np.unwrap(np.unwrap(p, axis=1), axis=0)
    tp = torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        p2 = tp * 1.0                                      # produced on s just before the calls
        ox = unwrapping.unwrap(p2, axis=1)
        oy = unwrapping.unwrap(p2, axis=0)
        oxy = unwrapping.unwrap2D(p2)
        total = oxy.sum()                                  # consumed on s without a synchronisation in between
    s.synchronize()
    assert R_.equal(ox.cpu().numpy(), want_x) and R_.equal(oy.cpu().numpy(), want_y) and R_.equal(oxy.cpu().numpy(), want_xy)
    assert float(total.cpu()) == float(oxy.sum().cpu())


@pytest.mark.parametrize("name", ["w97", "bgr"])
def test_ftp_phase_unwrap_numpy(unwrapping, name):
    """ftpPhase(unwrap="numpy") is np.unwrap along x, then along y, of the library's own wrapped map, bit for bit, on host arrays
    and on device tensors; the profile slot counts its two launches."""
    import json
    import torch
    from simplestereo_amd import _native, active
    with open(os.path.join(G, "ftp_cases.json")) as f:
        rf = json.load(f)["cases"][name]["radius_factor"]
    z = np.load(os.path.join(G, "ftp_cases.npz"))
    obj, ref, fc = z[name + "__obj"], z[name + "__ref"], z[name + "__fc"]
    wrapped = active.ftpPhase(obj, ref, fc, rf)
    want = np.unwrap(np.unwrap(wrapped, discont=PI, axis=1), discont=PI, axis=0)
    lib = _native.lib()
    lib.ssamd_profile_enable(1)
    lib.ssamd_profile_reset()
    try:
        got = active.ftpPhase(obj, ref, fc, rf, unwrap="numpy")
        ms, n = _native.profile_read()
        assert n[_native.K_NPUNWRAP] == 2 and n[_native.K_FTP] == 1 and n[_native.K_UNWRAP] == 0
    finally:
        lib.ssamd_profile_enable(0)
    assert R_.equal(got, want)
    assert R_.equal(active.ftpPhase(obj, ref, fc, rf, unwrap="numpy", tau="not read"), want)
    dev = active.ftpPhase(torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda(), fc, rf, unwrap="numpy")
    assert dev.is_cuda and R_.equal(dev.cpu().numpy(), want)
    assert R_.equal(unwrapping.unwrap2D(wrapped), want)
    # the wrapped call and the IIR chain are unchanged by it
    assert R_.equal(active.ftpPhase(obj, ref, fc, rf), wrapped)
    assert R_.equal(active.ftpPhase(obj, ref, fc, rf, unwrap="iir", tau=0.8), unwrapping.infiniteImpulseResponse(wrapped, 0.8))


def test_library_refuses_other_unwrap_values(unwrapping):
    from simplestereo_amd import _native
    img = np.zeros((2, 8), dtype=np.uint8)
    f = np.full(2, 0.25)
    out = np.zeros((2, 8))
    for uw in (3, -1):
        rc = _native.lib().ssamd_ftp_phase(img.ctypes.data, 1, img.ctypes.data, 1, 2, 8, f.ctypes.data, f.ctypes.data, uw, 1.0,
                                           out.ctypes.data, -1)
        assert rc == -1
    rc = _native.lib().ssamd_ftp_phase(img.ctypes.data, 1, img.ctypes.data, 1, 2, 8, f.ctypes.data, f.ctypes.data, 2, 7.5,
                                       out.ctypes.data, -1)
    assert rc == 0                                           # tau is not read with unwrap == 2


def test_length_is_not_limited(unwrapping, size):
    """Neither form limits len: a line of 2048 chunks and a column group of 1024 tiles, the state carried across every one."""
    for shape, axis in (((1, 2048 * size.R + 3), 1), ((1024 * size.T + 1, 2), 0)):
        p = R_.steep_ramp(shape, axis, seed=9)
        want = np.unwrap(p, axis=axis)
        assert np.abs(want).max() > 1e5
        assert R_.equal(unwrapping.unwrap(p, axis=axis), want)


def _bits_equal(a, b):
    import torch
    return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))


def test_row_form_at_the_stated_limit(unwrapping):
    """A launch holds fewer than 2^32 threads: the most lines the planner accepts (2^26 - 1 waves) run, one more is refused.
    Lines of one sample, so the result is the input, bit for bit; device tensors of 512 MiB."""
    import torch
    lines = (2 ** 32 - 1) // _plan(1, 1, 1)["threads"]
    assert _plan(lines, 1, 1)["blocks"] == lines
    g = torch.Generator(device="cuda").manual_seed(1)
    p = torch.randn((lines + 1, 1), dtype=torch.float64, device="cuda", generator=g) * 50
    got = unwrapping.unwrap(p[:lines], axis=1)
    torch.cuda.synchronize()
    assert got.shape == (lines, 1) and _bits_equal(got, p[:lines])
    del got
    with pytest.raises(ValueError, match="2\\^32 threads"):
        unwrapping.unwrap(p, axis=1)
    torch.cuda.synchronize()                                 # the refusal enqueued nothing that fails later
    # lines of two samples at the same count of workgroups: against numpy at both ends, the whole of it by its properties
    p2 = p[:lines].repeat(1, 2)
    p2[:, 1] += torch.randn(lines, dtype=torch.float64, device="cuda", generator=g) * 50
    got = unwrapping.unwrap(p2, axis=1)
    for part in (slice(0, 4096), slice(lines - 4096, lines)):
        assert R_.equal(got[part].cpu().numpy(), np.unwrap(p2[part].cpu().numpy(), axis=1))
    assert _bits_equal(got[:, 0], p2[:, 0]) and float((got[:, 1] - got[:, 0]).abs().max()) <= PI * (1 + 1e-12)


def test_column_form_at_the_stated_limit(unwrapping, size):
    """The most workgroups of the column form the planner accepts (2^24 - 1 of 256 threads) run, one more is refused: as outer
    indices with two columns each (512 MiB per tensor), and as lane groups of one outer index (4 GiB per tensor); columns of two
    samples."""
    import torch
    groups = (2 ** 32 - 1) // _plan(1, 2, 2)["threads"]
    g = torch.Generator(device="cuda").manual_seed(2)
    for shape, axis in (((groups + 1, 2, 2), 1), ((2, (groups + 1) * size.LANES), 0)):
        p = torch.randn(shape, dtype=torch.float64, device="cuda", generator=g) * 50
        ok = p[:groups] if axis == 1 else p[:, :groups * size.LANES]
        assert _plan(*((groups, 2, 2) if axis == 1 else (1, 2, groups * size.LANES)))["blocks"] == groups
        got = unwrapping.unwrap(ok, axis=axis)
        torch.cuda.synchronize()
        first, second = (got[:, 0], got[:, 1]) if axis == 1 else (got[0], got[1])
        src = ok[:, 0] if axis == 1 else ok[0]
        assert _bits_equal(first.contiguous(), src.contiguous())
        assert float((second - first).abs().max()) <= PI * (1 + 1e-12)          # every step unwrapped
        for part in (slice(0, 4096), slice(-4096, None)):
            sub = (ok[part] if axis == 1 else ok[:, part]).cpu().numpy()
            gsub = (got[part] if axis == 1 else got[:, part]).cpu().numpy()
            assert R_.equal(gsub, np.unwrap(sub, axis=axis))
        with pytest.raises(ValueError, match="2\\^32 threads"):
            unwrapping.unwrap(p, axis=axis)
        torch.cuda.synchronize()
        del p, ok, got, first, second, src
