"""GPU: ss.active.ftpPhase (ftp_phase_kernel, a band-limited direct DFT per image row) against the extended-precision truth of
tests/golden/ftp_cases.* -- every pixel, |wrap(got - truth)| within the case's recorded tolerance
16 * max(numpy's own error against that truth, pi 2^-52), read from the json -- on host arrays and on device tensors; plus
the exact properties: an empty band is 0.0, host and device agree bitwise, streams are respected, unwrap="iir" is the
unwrapper applied to the wrapped map bit for bit, and the width limit is enforced at the limit."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, G)

import _ftp_ref                                      # noqa: E402

with open(os.path.join(G, "ftp_cases.json")) as _f:
    META = json.load(_f)
CASES = META["cases"]


@pytest.fixture(scope="module")
def active():
    import torch
    assert torch.cuda.is_available()
    from simplestereo_amd import active
    return active


@pytest.fixture(scope="module")
def data():
    z = np.load(os.path.join(G, "ftp_cases.npz"))
    return {k: z[k] for k in z.files}


def _inputs(data, name):
    return data[name + "__obj"], data[name + "__ref"], data[name + "__fc"], CASES[name]["radius_factor"]


def _bitwise(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check(name, got, truth):
    assert got.dtype == np.float64 and got.shape == truth.shape
    err = _ftp_ref.wrap_err(got, truth)
    worst = float(err.max())
    print("%s: worst angle error %.3e (numpy %.3e, tolerance %.3e)" % (name, worst, CASES[name]["numpy_err"], CASES[name]["tol"]))
    assert np.isfinite(got).all()
    assert worst <= CASES[name]["tol"], (name, worst, CASES[name]["tol"], np.unravel_index(int(err.argmax()), err.shape))


# max_width has its own test below
TRUTH_CASES = sorted(n for n in CASES if n != "max_width")


@pytest.mark.parametrize("name", TRUTH_CASES)
def test_host_arrays_against_truth(active, data, name):
    obj, ref, fc, rf = _inputs(data, name)
    _check(name, active.ftpPhase(obj, ref, fc, rf), data[name + "__truth"])


@pytest.mark.parametrize("name", TRUTH_CASES)
def test_device_tensors_against_truth_and_equal_to_host(active, data, name):
    import torch
    obj, ref, fc, rf = _inputs(data, name)
    out = active.ftpPhase(torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda(), fc, rf)
    assert out.is_cuda and out.dtype == torch.float64
    got = out.cpu().numpy()
    _check(name, got, data[name + "__truth"])
    assert _bitwise(got, active.ftpPhase(obj, ref, fc, rf))


# The pair kernel at each columns-per-thread instance the fixture does not reach (it holds CPT 1 and, with max_width, 8): the
# smallest width of CPT 2, 4 and 8 (ftp_plan.h), two rows and a narrow band -- the shapes of the one-image cases cpt2_w1025,
# cpt4_w2049 and cpt8_w4097 of tests/golden/ftp_mapping_cases.  name: (w, radius_factor); fc is the frequency nearest to 0.05
# with a whole number of fringes in the row, so that no pixel at the row's ends has a small |ghat * conj(g0hat)|.
CPT_CASES = {"cpt2_w1025": (1025, 0.1), "cpt4_w2049": (2049, 0.05), "cpt8_w4097": (4097, 0.03)}
_CPT = {}


def _cpt_case(name):
    """-> (obj, ref, fc, radius_factor, truth, numpy_err, tol): the fixture's rule applied here, once -- the inputs chosen so
    that no pixel's angle is ill-conditioned, the tolerance from numpy's own distance to the extended-precision truth"""
    if name not in _CPT:
        import make_golden_ftp
        w, rf = CPT_CASES[name]
        fc = round(0.05 * w) / w
        obj, ref = make_golden_ftp.fringes(2, w, fc, seed=w)
        truth, ratio = _ftp_ref.truth_longdouble(obj, ref, fc, rf)
        assert ratio.min() >= META["min_ratio"], (name, float(ratio.min()))
        numpy_err = float(_ftp_ref.wrap_err(_ftp_ref.ftp_phase_numpy(obj, ref, fc, rf), truth).max())
        truth.setflags(write=False)
        _CPT[name] = (obj, ref, fc, rf, truth, numpy_err, META["tol_factor"] * max(numpy_err, META["tol_floor"]))
    return _CPT[name]


@pytest.mark.parametrize("name", sorted(CPT_CASES))
def test_pair_kernel_at_each_columns_per_thread_host_and_device(active, name):
    import torch
    obj, ref, fc, rf, truth, numpy_err, tol = _cpt_case(name)
    host = active.ftpPhase(obj, ref, fc, rf)
    dev = active.ftpPhase(torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda(), fc, rf)
    assert dev.is_cuda and dev.dtype == torch.float64
    for form, got in (("host", host), ("device", dev.cpu().numpy())):
        assert got.dtype == np.float64 and got.shape == truth.shape and np.isfinite(got).all()
        err = _ftp_ref.wrap_err(got, truth)
        print("%s, %s form: worst angle error %.3e (numpy %.3e, tolerance %.3e)" % (name, form, float(err.max()), numpy_err, tol))
        assert float(err.max()) <= tol, (name, form, float(err.max()), tol, np.unravel_index(int(err.argmax()), err.shape))
    assert _bitwise(dev.cpu().numpy(), host)


def test_scalar_fc_and_python_numbers(active, data):
    obj, ref, fc, rf = _inputs(data, "w97")
    a = active.ftpPhase(obj, ref, fc, rf)
    assert _bitwise(a, active.ftpPhase(obj, ref, float(fc[0]), rf))
    assert _bitwise(a, active.ftpPhase(obj, ref, [float(v) for v in fc], np.float64(rf)))


def test_non_contiguous_inputs(active, data):
    import torch
    obj, ref, fc, rf = _inputs(data, "bgr")
    a = active.ftpPhase(obj, ref, fc, rf)
    wide_o = np.zeros((obj.shape[0], obj.shape[1] + 5, 3), dtype=np.uint8)
    wide_o[:, 2:-3] = obj
    assert _bitwise(a, active.ftpPhase(wide_o[:, 2:-3], ref, fc, rf))
    t = torch.from_numpy(wide_o).cuda()[:, 2:-3]
    assert not t.is_contiguous()
    assert _bitwise(a, active.ftpPhase(t, torch.from_numpy(ref).cuda(), fc, rf).cpu().numpy())


def test_bgr_is_the_channel_maximum(active, data):
    """The BGR cases give exactly what their gray images give, and the maximum is not always channel 0."""
    for name in ("bgr", "gray_vs_bgr"):
        obj, ref, fc, rf = _inputs(data, name)
        assert ref.ndim == 3 and (ref.argmax(axis=2) != 0).any()
        assert _bitwise(active.ftpPhase(obj, ref, fc, rf), active.ftpPhase(_ftp_ref.gray(obj), _ftp_ref.gray(ref), fc, rf))


def test_empty_band_row_is_zero_and_leaves_its_neighbours(active, data):
    obj, ref, fc, rf = _inputs(data, "empty_middle_row")
    c = CASES["empty_middle_row"]
    assert c["slo"][1] > c["shi"][1] and c["slo"][0] <= c["shi"][0]
    got = active.ftpPhase(obj, ref, fc, rf)
    assert np.array_equal(got[1], np.zeros(got.shape[1])) and not np.signbit(got[1]).any()
    for y in (0, 2):                                   # each neighbour alone gives the same row, bit for bit
        alone = active.ftpPhase(obj[y:y + 1], ref[y:y + 1], fc[y:y + 1], rf)
        assert _bitwise(alone[0], got[y]) and np.abs(got[y]).max() > 1e-3
    _check("empty_middle_row", got, data["empty_middle_row__truth"])
    # every row empty
    z = active.ftpPhase(obj, ref, 0.0019, rf)
    assert np.array_equal(z, np.zeros_like(z))


def test_non_default_stream(active, data):
    """The call runs on the current stream: a kernel queued on that stream before it delays it, and its result is complete
    once that stream is synchronised."""
    import torch
    obj, ref, fc, rf = _inputs(data, "w1000")
    want = active.ftpPhase(obj, ref, fc, rf)
    tobj, tref = torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        # inputs produced on s just before the call: the call must be ordered behind them
        o2 = (tobj.to(torch.int32) + 0).to(torch.uint8)
        r2 = (tref.to(torch.int32) + 0).to(torch.uint8)
        out = active.ftpPhase(o2, r2, fc, rf)
        unw = active.ftpPhase(o2, r2, fc, rf, unwrap="iir", tau=0.8)
        total = out.sum()                              # consumed on s without a synchronisation in between
    s.synchronize()
    assert _bitwise(out.cpu().numpy(), want)
    assert float(total.cpu()) == float(out.sum().cpu())
    from simplestereo_amd import unwrapping
    assert _bitwise(unw.cpu().numpy(), unwrapping.infiniteImpulseResponse(want, 0.8))


@pytest.mark.parametrize("tau", [1, 0.8])
@pytest.mark.parametrize("name", ["w1000", "w63_fc_per_row", "empty_middle_row", "w1"])
def test_unwrap_iir_is_the_unwrapper_on_the_wrapped_map(active, data, name, tau):
    import torch
    from simplestereo_amd import unwrapping
    obj, ref, fc, rf = _inputs(data, name)
    wrapped = active.ftpPhase(obj, ref, fc, rf)
    want = unwrapping.infiniteImpulseResponse(wrapped, tau)
    assert _bitwise(active.ftpPhase(obj, ref, fc, rf, unwrap="iir", tau=tau), want)
    tobj, tref = torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda()
    dev = active.ftpPhase(tobj, tref, fc, rf, unwrap="iir", tau=tau)
    assert dev.is_cuda and _bitwise(dev.cpu().numpy(), want)
    assert _bitwise(unwrapping.infiniteImpulseResponse(active.ftpPhase(tobj, tref, fc, rf), tau).cpu().numpy(), want)
    # the wrapped call is unchanged by the unwrapping calls before it (they share scratch buffers)
    assert _bitwise(active.ftpPhase(obj, ref, fc, rf), wrapped)


def test_maximum_width_against_truth(active, data):
    import torch
    obj, ref, fc, rf = _inputs(data, "max_width")
    assert obj.shape == (2, active.MAX_WIDTH) and META["max_width"] == active.MAX_WIDTH
    got = active.ftpPhase(obj, ref, fc, rf)
    _check("max_width", got, data["max_width__truth"])
    dev = active.ftpPhase(torch.from_numpy(obj).cuda(), torch.from_numpy(ref).cuda(), fc, rf)
    assert _bitwise(dev.cpu().numpy(), got)


def test_maximum_width_plus_one_is_refused(active):
    from simplestereo_amd import _native
    w = active.MAX_WIDTH + 1
    img = np.zeros((2, w), dtype=np.uint8)
    with pytest.raises(ValueError):
        active.ftpPhase(img, img, 0.05)
    # ... and by the library itself, with SSAMD_ELIMIT
    f = np.full(2, 0.05)
    out = np.zeros((2, w))
    rc = _native.lib().ssamd_ftp_phase(img.ctypes.data, 1, img.ctypes.data, 1, 2, w, f.ctypes.data, f.ctypes.data, 0, 1.0,
                                       out.ctypes.data, -1)
    assert rc == -5 and b"8192" in _native.lib().ssamd_last_error()


def test_library_passes_the_unwrappers_error_through(active):
    from simplestereo_amd import _native
    img = np.zeros((2, 8), dtype=np.uint8)
    f = np.full(2, 0.25)
    out = np.zeros((2, 8))
    rc = _native.lib().ssamd_ftp_phase(img.ctypes.data, 1, img.ctypes.data, 1, 2, 8, f.ctypes.data, f.ctypes.data, 1, 1.5,
                                       out.ctypes.data, -1)
    assert rc == -1 and _native.lib().ssamd_last_error() == b"Wrong tau value!"


def test_many_rows_and_profile_slot(active):
    """More rows than one round of workgroups, two widths in turn (two cached twiddle tables), every row the same input:
    every row the same output; the kernel is accounted in its own profile slot."""
    from simplestereo_amd import _native
    import make_golden_ftp
    lib = _native.lib()
    assert lib.ssamd_kernel_name(_native.K_FTP) == b"ftp_phase_kernel"
    lib.ssamd_profile_enable(1)
    lib.ssamd_profile_reset()
    try:
        for w in (1100, 330, 1100):                    # 1100: two columns per thread
            o1, r1 = make_golden_ftp.fringes(1, w, 0.07, 5)
            obj, ref = np.repeat(o1, 1500, axis=0), np.repeat(r1, 1500, axis=0)
            got = active.ftpPhase(obj, ref, 0.07)
            assert _bitwise(got, np.repeat(got[:1], 1500, axis=0))
            truth, ratio = _ftp_ref.truth_longdouble(o1, r1, 0.07, 0.5)          # the fixture's rule, applied to this row
            assert ratio.min() >= META["min_ratio"]
            numpy_err = float(_ftp_ref.wrap_err(_ftp_ref.ftp_phase_numpy(o1, r1, 0.07, 0.5), truth).max())
            assert float(_ftp_ref.wrap_err(got[:1], truth).max()) <= META["tol_factor"] * max(numpy_err, META["tol_floor"])
        ms, n = _native.profile_read()
        assert n[_native.K_FTP] == 3 and n[_native.K_UNWRAP] == 0
    finally:
        lib.ssamd_profile_enable(0)
