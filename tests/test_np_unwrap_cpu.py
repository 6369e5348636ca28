"""CPU: the host side of ss.unwrapping.unwrap / unwrap2D and of ftpPhase(unwrap="numpy") -- the arithmetic contract
(tests/_np_unwrap_ref.py against np.unwrap itself, and the proof that the order of the running sum is observable), the
Python-level checks (every exception before any native call), the geometry [outer][len][inner] the Python layer hands down, and
the launch planner (csrc/np_unwrap_plan.h through ssamd_np_unwrap_plan, which needs no device)."""
import ctypes
import os
import re

import numpy as np
import pytest

import _np_unwrap_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PI = np.pi

SHAPES = [((3, 129), 1), ((129, 3), 0), ((2, 70, 5), 1), ((5,), 0), ((1, 1), 1), ((2, 2), 0)]


# ---------------------------------------------------------------------------------------------- the arithmetic contract
@pytest.mark.parametrize("shape,axis", SHAPES)
def test_sequential_restatement_equals_numpy(shape, axis):
    for name, p in R.inputs(shape, axis).items():
        for discont, period in R.PARAMS:
            with np.errstate(all="ignore"):
                want = np.unwrap(p, discont=discont, axis=axis, period=period)
            assert R.equal(R.unwrap_ref(p, discont, axis, period), want), (name, discont, period)


@pytest.mark.parametrize("shape,axis", [((3, 129), 1), ((129, 3), 0), ((2, 257), 1), ((300, 2), 0)])
def test_order_of_the_running_sum_is_observable(shape, axis):
    """A 16-sample blocked scan of the same corrections differs from np.unwrap in at least a quarter of the samples of the
    steep ramp (measured: 70 % at 3 x 129 along rows, 72 % at 129 x 3 along columns): these inputs tell the orders apart."""
    p = R.steep_ramp(shape, axis)
    want = np.unwrap(p, axis=axis)
    frac = R.differing_fraction(R.blocked_unwrap(p, 16, axis), want)
    print("blocked scan differs in %.1f %% of %s along axis %d" % (100 * frac, shape, axis))
    assert frac >= 0.25
    assert R.equal(R.unwrap_ref(p, None, axis), want)
    # ... by rounding only: the two agree to a few ulp of the sums (hundreds of radians)
    assert np.abs(R.blocked_unwrap(p, 16, axis) - want).max() < 1e-10 and np.abs(want).max() > 100


def test_nan_tail_positions_are_numpys():
    for shape, axis in SHAPES:
        p = R.inputs(shape, axis)["nonfinite"]
        with np.errstate(all="ignore"):
            assert np.array_equal(np.isnan(np.unwrap(p, axis=axis)), R.nan_tail_positions(p, axis))


# ---------------------------------------------------------------------------------------------- Python-level checks
class _NoNative:
    def __getattr__(self, name):
        raise AssertionError("native call %s before the arguments were checked" % name)


@pytest.fixture
def ss_no_native(monkeypatch):
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    monkeypatch.setattr(_native, "lib", lambda: _NoNative())
    return ss


def test_exported_and_documented():
    import simplestereo_amd as ss
    from simplestereo_amd import _native
    u = ss.unwrapping
    assert {"unwrap", "unwrap2D", "infiniteImpulseResponse", "infiniteImpulseResponseBatch"} <= set(u.__all__)
    for name in ("``unwrap``", "``unwrap2D``", "ssamd_np_unwrap", "ssamd_np_unwrap_xy", "AxisError"):
        assert name in u.__doc__, name
    header = open(os.path.join(ROOT, "include", "ssamd.h")).read()
    assert "#define SSAMD_ABI_VERSION 8" in header and _native.ABI_VERSION == 8
    assert "#define SSAMD_K_NPUNWRAP %d" % _native.K_NPUNWRAP in header
    assert "#define SSAMD_K_COUNT %d" % _native.K_COUNT in header and _native.K_COUNT == _native.K_NPUNWRAP + 1
    assert "active.py:739-745" in header and "active.py:739-745" in u.unwrap2D.__doc__
    lib = _native.lib()
    for sym in ("ssamd_np_unwrap", "ssamd_np_unwrap_device", "ssamd_np_unwrap_xy", "ssamd_np_unwrap_xy_device", "ssamd_np_unwrap_plan"):
        assert hasattr(lib, sym), sym
    assert b"np_unwrap" in lib.ssamd_kernel_name(_native.K_NPUNWRAP)
    for value in ('"iir"', '"numpy"', "None"):
        assert value in ss.active.ftpPhase.__doc__


def test_unwrap_exceptions_before_any_native_call(ss_no_native):
    u = ss_no_native.unwrapping.unwrap
    p = np.zeros((4, 8))
    with pytest.raises(TypeError):
        u(p.tolist())
    for dtype in (np.float32, np.int64, np.complex128, np.float16):
        with pytest.raises(TypeError):
            u(p.astype(dtype))
    for zero_d in (np.ones(()), np.float64(1.0)):                # 0-d, as np.unwrap through diff
        with pytest.raises(ValueError):
            u(zero_d)
    with pytest.raises(ValueError):
        np.unwrap(np.ones(()))
    for axis in (2, -3, 17):
        with pytest.raises(np.exceptions.AxisError):
            u(p, axis=axis)
        with pytest.raises(np.exceptions.AxisError):
            np.unwrap(p, axis=axis)
    assert issubclass(np.exceptions.AxisError, ValueError) and issubclass(np.exceptions.AxisError, IndexError)
    for axis in (0.5, "0", None):
        with pytest.raises(TypeError):
            u(p, axis=axis)
    for period in (0, 0.0, -1.0, np.inf, -np.inf, np.nan, "1", None, 1j):
        with pytest.raises(ValueError):
            u(p, period=period)
    for discont in ("1", 1j, [1.0]):
        with pytest.raises(ValueError):
            u(p, discont=discont)
    with pytest.raises(TypeError):
        u(p, None, 0, 1.0)                                       # period is keyword-only, as in numpy


def test_unwrap2d_and_ftp_exceptions_before_any_native_call(ss_no_native):
    u2 = ss_no_native.unwrapping.unwrap2D
    for bad in (np.zeros(8), np.zeros((1, 2, 3, 4)), np.zeros(())):
        with pytest.raises(ValueError):
            u2(bad)
    with pytest.raises(TypeError):
        u2(np.zeros((4, 8), dtype=np.float32))
    with pytest.raises(TypeError):
        u2([[0.0, 1.0]])
    g = np.zeros((4, 8), dtype=np.uint8)
    f = ss_no_native.active.ftpPhase
    for bad_unwrap in ("IIR", "none", 1, True, b"iir", "Numpy", "np", b"numpy", 2):
        with pytest.raises(ValueError) as ei:
            f(g, g, 0.1, unwrap=bad_unwrap)
        assert all(v in str(ei.value) for v in ("None", '"iir"', '"numpy"'))
    with pytest.raises(ValueError):
        f(g, g, 0.1, unwrap="iir", tau=2.0)


def test_empty_arrays_give_empty_arrays(ss_no_native):
    u, u2 = ss_no_native.unwrapping.unwrap, ss_no_native.unwrapping.unwrap2D
    for shape in ((0,), (0, 8), (4, 0), (3, 0, 5)):
        for axis in range(len(shape)):
            out = u(np.zeros(shape), axis=axis)
            assert out.shape == shape and out.dtype == np.float64
            assert out.shape == np.unwrap(np.zeros(shape), axis=axis).shape
    for shape in ((0, 8), (4, 0), (0, 4, 8), (2, 0, 8)):
        assert u2(np.zeros(shape)).shape == shape
    e = np.zeros((0, 8), dtype=np.uint8)
    assert ss_no_native.active.ftpPhase(e, e, 0.1, unwrap="numpy", tau="ignored").shape == (0, 8)


# ---------------------------------------------------------------------------------------------- what reaches the library
@pytest.fixture
def seen(monkeypatch):
    from simplestereo_amd import _native
    calls = []

    class Lib:
        def ssamd_np_unwrap(self, src, outer, n, inner, discont, period, out, dev):
            calls.append(("np", src, outer, n, inner, discont, period, dev))
            return 0

        def ssamd_np_unwrap_xy(self, src, n, h, w, out, dev):
            calls.append(("xy", src, n, h, w, dev))
            return 0

        def ssamd_ftp_phase(self, obj, cho, ref, chr_, h, w, fmin, fmax, uw, tau, out, dev):
            calls.append(("ftp", cho, chr_, h, w, uw, tau, dev))
            return 0
    monkeypatch.setattr(_native, "lib", lambda: Lib())
    return calls


def test_geometry_the_python_layer_hands_down(seen):
    import simplestereo_amd as ss
    u = ss.unwrapping.unwrap

    def geometry(p, **kw):
        del seen[:]
        out = u(p, **kw)
        assert out.shape == p.shape and len(seen) == 1 and seen[0][0] == "np"
        return seen[0][2:5]
    assert geometry(np.zeros(7)) == (1, 7, 1)
    hw = np.zeros((4, 9))
    assert geometry(hw, axis=0) == (1, 4, 9) and geometry(hw, axis=-2) == (1, 4, 9)
    assert geometry(hw, axis=1) == (4, 9, 1) and geometry(hw, axis=-1) == (4, 9, 1) and geometry(hw) == (4, 9, 1)
    nhw = np.zeros((3, 4, 9))
    assert geometry(nhw, axis=0) == (1, 3, 36) and geometry(nhw, axis=1) == (3, 4, 9) and geometry(nhw, axis=2) == (12, 9, 1)
    assert geometry(nhw, axis=-3) == (1, 3, 36)
    assert geometry(np.zeros((2, 3, 4, 5)), axis=1) == (2, 3, 20)
    assert geometry(hw, axis=np.int64(1)) == (4, 9, 1)
    # defaults and pass-through of discont / period
    u(hw)
    assert seen[-1][5:] == (PI, 2 * PI, -1)
    u(hw, period=360.0)
    assert seen[-1][5:] == (180.0, 360.0, -1)
    u(hw, discont=1, period=np.float32(4))
    assert seen[-1][5:] == (1.0, 4.0, -1)
    u(hw, discont=np.nan)
    assert np.isnan(seen[-1][5]) and seen[-1][6] == 2 * PI


def test_non_contiguous_view_is_made_contiguous(seen):
    import simplestereo_amd as ss
    big = np.arange(60, dtype=np.float64).reshape(6, 10)
    view = big[::2, 1:8]                               # [3, 7], strides (160, 8)
    assert not view.flags["C_CONTIGUOUS"]
    ss.unwrapping.unwrap(view, axis=0)
    kind, src, outer, n, inner = seen[-1][:5]
    assert (outer, n, inner) == (1, 3, 7)
    handed = np.ctypeslib.as_array(ctypes.cast(src, ctypes.POINTER(ctypes.c_double)), (21,))
    assert np.array_equal(handed.reshape(3, 7), view)  # a packed copy, not the base array's memory
    t = big.T                                          # [10, 6] Fortran order
    ss.unwrapping.unwrap(t, axis=1)
    assert seen[-1][2:5] == (10, 6, 1)


def test_unwrap2d_and_ftp_numpy_hand_down(seen):
    import simplestereo_amd as ss
    ss.unwrapping.unwrap2D(np.zeros((4, 9)))
    assert seen[-1][0] == "xy" and seen[-1][2:] == (1, 4, 9, -1)
    ss.unwrapping.unwrap2D(np.zeros((3, 4, 9)))
    assert seen[-1][0] == "xy" and seen[-1][2:] == (3, 4, 9, -1)
    g = np.zeros((3, 8), dtype=np.uint8)
    ss.active.ftpPhase(g, np.zeros((3, 8, 3), dtype=np.uint8), 0.2, unwrap="numpy", tau=0.3)
    assert seen[-1] == ("ftp", 1, 3, 3, 8, 2, 1.0, -1)            # uw == 2; tau is not read
    ss.active.ftpPhase(g, g, 0.2, unwrap="numpy", tau=None)
    assert seen[-1][5] == 2
    ss.active.ftpPhase(g, g, 0.2, unwrap="iir", tau=0.3)
    assert seen[-1][5:7] == (1, 0.3)
    ss.active.ftpPhase(g, g, 0.2)
    assert seen[-1][5] == 0


# ---------------------------------------------------------------------------------------------- the planner
def _plan(outer, n, inner):
    from simplestereo_amd import _native
    return _native.np_unwrap_plan(outer, n, inner)


def _plan_rc(outer, n, inner):
    from simplestereo_amd import _native
    out = (ctypes.c_int32 * 8)()
    return _native.lib().ssamd_np_unwrap_plan(outer, n, inner, out)


@pytest.mark.parametrize("outer,n,inner", [(1, 1, 1), (1080, 1920, 1), (1, 1080, 1920), (3, 7, 5), (1, 2160, 4096), (2160, 4096, 1),
                                           (7, 1, 17), (1, 10 ** 6, 2), (5, 3, 16), (5, 3, 33), (2 ** 20, 2, 1),
                                           (2 ** 26 - 1, 2, 1), (2 ** 24 - 1, 2, 2)])
def test_plan_properties(outer, n, inner):
    p = _plan(outer, n, inner)
    assert p["form"] == ("row" if inner == 1 else "column")
    assert 0 < p["lds_bytes"] <= 160 * 1024
    assert p["threads"] % 64 == 0 and 64 <= p["threads"] <= 1024
    assert p["blocks"] * p["threads"] < 2 ** 32                              # what one HIP launch holds
    held = p["chunk"] * (1 if inner == 1 else p["lanes"])                  # samples of a chunk: a line's, or rows x columns
    assert held == p["threads"] * p["per_thread"]                          # ... are what the workgroup's threads hold
    assert p["chunk"] % 8 == 0
    if inner == 1:
        assert p["blocks"] == outer and p["lanes"] == 64                    # a wave per line
    else:
        assert p["groups"] * p["lanes"] >= inner > (p["groups"] - 1) * p["lanes"]
        assert p["blocks"] == outer * p["groups"]                           # the workgroups cover outer x inner
        assert p["lanes"] * 8 >= 128                                        # a workgroup reads whole 128-byte lines of a row
    # LDS: the corrections of a chunk as doubles, at least
    assert p["lds_bytes"] >= 8 * held


def test_plan_matches_the_kernel_sources():
    """The constants the tests aim with are the ones the kernels are built with."""
    src = open(os.path.join(ROOT, "simplestereo_amd", "csrc", "np_unwrap_plan.h")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (NPU_[A-Z_]+) = (\d+);", src)}
    row, col = _plan(2, 100, 1), _plan(2, 100, 5)
    assert row["chunk"] == consts["NPU_ROW_THREADS"] * consts["NPU_ROW_PER"] and row["threads"] == consts["NPU_ROW_THREADS"]
    assert col["lanes"] == consts["NPU_COL_LANES"] and col["threads"] == consts["NPU_COL_THREADS"]
    assert col["chunk"] == consts["NPU_COL_THREADS"] // consts["NPU_COL_LANES"] * consts["NPU_COL_PER"]


def test_plan_empty_extents_and_bad_arguments():
    for g in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (0, 0, 0)):
        assert _plan(*g)["blocks"] == 0
    for g in ((-1, 5, 5), (5, -1, 5), (5, 5, -1)):
        assert _plan_rc(*g) == -1
    from simplestereo_amd import _native
    assert _native.lib().ssamd_np_unwrap_plan(1, 1, 1, None) == -1


def test_plan_refuses_at_the_stated_limits_and_accepts_one_below():
    """2^40 samples (what the host path stages, as ssamd_iir_unwrap) and fewer than 2^32 threads per launch (HIP refuses
    gridDim.x * blockDim.x >= 2^32): SSAMD_ELIMIT beyond, accepted at the limit.  len alone is limited by neither form."""
    big = 2 ** 40
    row, col = _plan(1, 2, 1), _plan(1, 2, 2)
    max_lines = (2 ** 32 - 1) // row["threads"]
    max_groups = (2 ** 32 - 1) // col["threads"]
    assert (max_lines, max_groups) == (2 ** 26 - 1, 2 ** 24 - 1)
    assert _plan_rc(1, big, 1) == 0 and _plan_rc(1, big + 1, 1) == -5
    assert _plan_rc(1, big // 2, 2) == 0 and _plan_rc(1, big // 2, 3) == -5 and _plan_rc(2, big // 2, 1) == 0
    assert _plan_rc(2 ** 10, 2 ** 20, 2 ** 10) == 0 and _plan_rc(2 ** 10, 2 ** 20, 2 ** 10 + 1) == -5
    assert _plan_rc(2 ** 62, 2 ** 62, 2 ** 62) == -5 and _plan_rc(2 ** 63 - 1, 2, 1) == -5      # no overflow on the way
    # row form: one workgroup of 64 threads per line
    for n in (1, 2, 1000):
        assert _plan_rc(max_lines, n, 1) == 0 and _plan(max_lines, n, 1)["blocks"] == max_lines
        assert _plan_rc(max_lines + 1, n, 1) == -5
    assert (max_lines + 1) * row["threads"] == 2 ** 32
    # column form: outer x ceil(inner / lanes) workgroups of 256 threads
    lanes = col["lanes"]
    assert _plan_rc(1, 2, max_groups * lanes) == 0 and _plan(1, 2, max_groups * lanes)["groups"] == max_groups
    assert _plan_rc(1, 2, max_groups * lanes + 1) == -5
    assert _plan_rc(max_groups, 2, lanes) == 0 and _plan_rc(max_groups, 2, 2) == 0 and _plan_rc(max_groups + 1, 2, 2) == -5
    assert _plan_rc(max_groups, 2, lanes + 1) == -5
    assert (max_groups + 1) * col["threads"] == 2 ** 32
    from simplestereo_amd import _native
    assert b"2^32 threads" in _native.lib().ssamd_last_error()


def test_library_refuses_a_bad_period_and_bad_sizes_without_a_device():
    """ssamd_np_unwrap's argument checks come before the device is touched: they answer on a machine without one."""
    from simplestereo_amd import _native
    lib = _native.lib()
    a = np.zeros(4)
    for period in (0.0, -1.0, np.inf, np.nan):
        assert lib.ssamd_np_unwrap(a.ctypes.data, 1, 4, 1, 1.0, period, a.ctypes.data, -1) == -1
        assert b"period" in lib.ssamd_last_error()
    assert lib.ssamd_np_unwrap(a.ctypes.data, 1, -4, 1, PI, 2 * PI, a.ctypes.data, -1) == -1
    assert lib.ssamd_np_unwrap(a.ctypes.data, 2 ** 40, 2, 1, PI, 2 * PI, a.ctypes.data, -1) == -5
    assert lib.ssamd_np_unwrap(a.ctypes.data, 2 ** 26, 2, 1, PI, 2 * PI, a.ctypes.data, -1) == -5       # 2^32 threads
    assert lib.ssamd_np_unwrap_device(a.ctypes.data, 2 ** 24, 2, 2, PI, 2 * PI, a.ctypes.data, None) == -5
    assert lib.ssamd_np_unwrap(None, 0, 4, 1, PI, 2 * PI, None, -1) == 0      # an empty extent does nothing
    assert lib.ssamd_np_unwrap_device(None, 1, 0, 4, PI, 2 * PI, None, None) == 0
    assert lib.ssamd_np_unwrap(None, 1, 4, 1, PI, 2 * PI, a.ctypes.data, -1) == -1
    assert lib.ssamd_np_unwrap_xy(None, 0, 4, 4, None, -1) == 0 and lib.ssamd_np_unwrap_xy(None, 2, 0, 4, None, -1) == 0
    assert lib.ssamd_np_unwrap_xy(a.ctypes.data, -1, 2, 2, a.ctypes.data, -1) == -1
    assert lib.ssamd_np_unwrap_xy_device(None, 1, 2, 2, None, None) == -1
