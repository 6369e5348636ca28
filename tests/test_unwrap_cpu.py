"""CPU tier of ss.unwrapping (the reference's _unwrapping.infiniteImpulseResponse): the argument checks against the
exceptions recorded from the reference (golden/unwrap_errors.json), the documented deviations that need no device, and
the plain restatement tests/_unwrap_ref.py against every small golden the reference wrote (golden/unwrap_cases.*)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
sys.path.insert(0, G)

import _unwrap_ref                                  # noqa: E402
import make_golden_unwrap                           # noqa: E402

with open(os.path.join(G, "unwrap_errors.json")) as f:
    PROBES = json.load(f)
with open(os.path.join(G, "unwrap_cases.json")) as f:
    CASES = json.load(f)["cases"]


def _args(expr):
    return eval(expr, {"np": np, "nan": float("nan")})


@pytest.mark.parametrize("probe", PROBES, ids=[p["id"] for p in PROBES])
def test_exception_parity(probe):
    from simplestereo_amd import unwrapping
    args = _args(probe["args"])
    if probe["result"] == "raised":
        exc = {"ValueError": ValueError, "TypeError": TypeError}[probe["type"]]
        with pytest.raises(exc) as e:
            unwrapping.infiniteImpulseResponse(*args)
        assert type(e.value) is exc and str(e.value) == probe["message"]
    else:
        # accepted by the reference: passes every check here too (the computation itself is the GPU tier's)
        unwrapping._check(args[0], args[1], 2)


def test_reference_checks_in_order():
    from simplestereo_amd import unwrapping
    ids = {p["id"]: p for p in PROBES}
    assert ids["list_phase_bad_tau"]["message"] == "Invalid input format!"
    assert ids["phase_3d_bad_tau"]["message"] == "Wrong phase dimensions!"
    assert ids["tau_nan"] == {"id": "tau_nan", "args": ids["tau_nan"]["args"], "result": "accepted", "all_nan": True}
    with pytest.raises(ValueError, match="Wrong phase dimensions!"):
        unwrapping.infiniteImpulseResponse(np.zeros((3, 2, 2)), 0.5)     # the drop-in stays 2-D only
    with pytest.raises(ValueError, match="Wrong phase dimensions!"):
        unwrapping.infiniteImpulseResponseBatch(np.zeros((2, 2)), 0.5)
    with pytest.raises(ValueError, match="Wrong tau value!"):
        unwrapping.infiniteImpulseResponseBatch(np.zeros((1, 2, 2)), -1)


def test_deviation_non_float64_raises_type_error():
    from simplestereo_amd import unwrapping
    for dt in (np.float32, np.int64, np.uint8, np.complex128):
        with pytest.raises(TypeError):
            unwrapping.infiniteImpulseResponse(np.zeros((4, 5), dtype=dt), 0.5)
    # the reference's checks come first
    with pytest.raises(ValueError, match="Wrong phase dimensions!"):
        unwrapping.infiniteImpulseResponse(np.zeros(5, dtype=np.float32), 0.5)


def test_deviation_empty_maps():
    from simplestereo_amd import unwrapping
    for shape in ((0, 7), (0, 0), (5, 0)):
        out = unwrapping.infiniteImpulseResponse(np.zeros(shape), 1)
        assert out.shape == shape and out.dtype == np.float64
    out = unwrapping.infiniteImpulseResponseBatch(np.zeros((0, 4, 4)), 1)
    assert out.shape == (0, 4, 4) and out.dtype == np.float64


def test_c_abi_checks():
    """ssamd_iir_unwrap* validate their arguments before they look for a device."""
    from simplestereo_amd import _native
    lib = _native.lib()
    a = np.zeros((4, 8))
    o = np.empty_like(a)
    assert lib.ssamd_iir_unwrap(a.ctypes.data, 1, 0, 8, 0.5, o.ctypes.data, -1) == -1
    assert b"Wrong phase dimensions!" in lib.ssamd_last_error()
    assert lib.ssamd_iir_unwrap(a.ctypes.data, 1, 4, 8, 1.5, o.ctypes.data, -1) == -1
    assert b"Wrong tau value!" in lib.ssamd_last_error()
    assert lib.ssamd_iir_unwrap(a.ctypes.data, 1, 4, 16385, 0.5, o.ctypes.data, -1) == -5
    assert lib.ssamd_iir_unwrap_device(a.ctypes.data, -1, 4, 8, 0.5, o.ctypes.data, None) == -1
    assert lib.ssamd_iir_unwrap(a.ctypes.data, 0, 4, 8, 0.5, o.ctypes.data, -1) == 0     # nothing to do
    assert lib.ssamd_kernel_name(_native.K_UNWRAP) == b"iir_unwrap_kernel"


def test_golden_recipes_rebuild_the_inputs():
    z = np.load(os.path.join(G, "unwrap_cases.npz"))
    for name, c in CASES.items():
        ph = make_golden_unwrap.phase_input(c["recipe"])
        assert make_golden_unwrap.sha(ph) == c["input_sha256"], name
        if c["whole"]:
            assert make_golden_unwrap.sha(z[name + "__in"]) == c["input_sha256"], name
            assert make_golden_unwrap.sha(z[name + "__out"]) == c["output_sha256"], name
    assert {"frame1080", "frame2160"} <= set(CASES)


@pytest.mark.parametrize("name", sorted(n for n in CASES if not n.startswith("frame")))
def test_restatement_equals_reference_golden(name):
    c = CASES[name]
    if c["whole"]:
        z = np.load(os.path.join(G, "unwrap_cases.npz"))
        out = _unwrap_ref.unwrap(z[name + "__in"], c["tau"])
        assert _unwrap_ref.identical(out, z[name + "__out"])
        if np.isnan(out).any():
            return
    else:
        out = _unwrap_ref.unwrap(make_golden_unwrap.phase_input(c["recipe"]), c["tau"])
    assert make_golden_unwrap.sha(out) == c["output_sha256"]


# ---- the restated fmod of the kernel (unwrap_fmod_2pi), modelled on the host: tests/_unwrap_probes.py
def test_reciprocal_of_two_pi_is_rounded_up():
    """The double 1.0 / (2 pi) lies above the exact reciprocal of the double 2 pi: the reason why the quotient estimate is never
    too small, i.e. why the `r >= m` (x >= 0) and `r <= -m` (x < 0) corrections of unwrap_fmod_2pi are dead for every double."""
    from fractions import Fraction
    import _unwrap_probes as P
    assert Fraction(P.C) * Fraction(P.M) > 1
    # the boundary cases of the argument: x = m * 2^j has the exact quotient 2^j, and the estimate finds it
    for j in range(0, 38):                              # m * 2^38 is past the switch at 2^40
        x = P.M * 2.0 ** j
        assert int(x * P.C) == 2 ** j and P.branch(x) == "pos_direct" and P.branch(-x) == "neg_direct"


def test_fmod_model_equals_fmod_and_probes_take_every_reachable_branch():
    """The host-side model of unwrap_fmod_2pi (k from trunc(x * (1/m)), one exact fma, one correction) gives math.fmod's bits on
    every argument that the probe maps of tests/test_gpu_unwrap_limits.py pass to it, and those arguments take every branch
    that any double can take, both corrections towards zero for both signs included."""
    import math
    from fractions import Fraction
    import _unwrap_probes as P
    a = P.probes()
    assert 1.5e5 < len(a) < 3e5 and np.array_equal(a, P.probes())          # deterministic
    _, args = P.fmod_arguments(P.pair_maps(a), 1.0)
    census = P.branch_census(args)
    print("census", census)
    assert sum(census.values()) == len(args)
    for b in P.BRANCHES:
        assert (census[b] == 0) if b in P.DEAD else (census[b] >= 100), (b, census)
    # the prefilter of branch_census agrees with the exact model
    sub = args[:: max(1, len(args) // 20000)]
    exact = dict.fromkeys(P.BRANCHES, 0)
    for v in sub.tolist():
        exact[P.branch(v)] += 1
    assert exact == P.branch_census(sub)

    def fma(x, y, z):                                   # exact product and sum, rounded once
        return float(Fraction(x) * Fraction(y) + Fraction(z))

    def model(x):
        k = float(math.trunc(x * P.C))
        r = fma(-k, P.M, x)
        if x >= 0:
            if r < 0:
                k -= 1
            elif r >= P.M:
                k += 1
            else:
                return r
        else:
            if r > 0:
                k += 1
            elif r <= -P.M:
                k -= 1
            else:
                return r
        return fma(-k, P.M, x)

    fast = args[np.abs(args) < P.SWITCH]
    near = fast[np.abs(fast - np.rint(fast * P.C) * P.M) < 1e-3]           # the arguments near a multiple of 2 pi ...
    rng = np.random.default_rng(1)
    for v in np.concatenate([near[:: max(1, len(near) // 20000)], rng.choice(fast, 5000)]).tolist():   # ... and a sample of the rest
        got, want = model(v), math.fmod(v, P.M)
        assert got == want and math.copysign(1, got) == math.copysign(1, want) or (want == 0 and got == 0), v
