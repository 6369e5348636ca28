"""GPU tier of the shared plane-stack front (plane_stack_frame of graycode_kernels.hip.h, called by graycode_decode_kernel and
phaseshift_decode_kernel): the phase-shift decode reproduces, bit for bit and on both routes, what the commit before the fold
computed on the MI355X (tests/golden/phaseshift_parent_digests.json), and both decoders run every mode of the front and every
failing condition of its window (tests/_plane_stack.front_inputs, classified by tests/_graycode_ref.front) against their numpy
restatements on one camera geometry: 67 x 37, three blocks of 1024 pixels with a ragged end."""
import numpy as np
import pytest

import _graycode_ref as G
import _phaseshift_ref as P
import _plane_stack as X
import test_gpu_phaseshift as T

pytestmark = pytest.mark.gpu
PERIODS = T.META["decode"]["full"]["periods"]
TOL = T.META["tol_factor"] * max(T.PROJ) * T.META["floor"]      # the rule of the recorded tolerances at its floor: no recorded one is tighter
INPUTS = X.front_inputs()


@pytest.fixture(scope="module")
def ss():
    import simplestereo_amd
    return simplestereo_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.mark.parametrize("name", sorted(T.META["decode"]))
def test_phase_shift_decode_has_the_bits_of_the_commit_before_the_fold(ss, torch, name):
    want = X.load("phaseshift_parent_digests.json")
    assert sorted(want) == sorted(X.digest_key(n, m) for n in T.META["decode"] for m in T.MODULATIONS)
    c = T.META["decode"][name]
    stack, maps, _, _ = T._decode_case(name)
    t = torch.from_numpy(stack).cuda()
    dmaps = None if maps is None else tuple(torch.from_numpy(m).cuda() for m in maps)
    for m in T.MODULATIONS:
        host = ss.active.phaseShiftDecode(stack, c["periods"], T.PROJ, maps=maps, roi=c["roi"], min_modulation=m)
        dev = ss.active.phaseShiftDecode(t, c["periods"], T.PROJ, maps=dmaps, roi=c["roi"], min_modulation=m)
        assert X.digest(host) == want[X.digest_key(name, m)], (name, m, "host route")
        assert X.digest(dev.cpu().numpy()) == want[X.digest_key(name, m)], (name, m, "device route")


def test_the_inputs_reach_every_path_of_the_front():
    modes, failed = set(), set()
    for _, maps, box in INPUTS:
        mode, fails = G.front(37, 67, box, maps)
        modes |= set(mode.tolist())
        failed |= {c for c in fails if fails[c].any()}
    assert modes == {G.GRAY_ROW4, G.GRAY_BYTES, G.GRAY_TAPS, G.GRAY_WINDOW} and failed == set(G.WINDOW_CONDITIONS)
    assert set(G.front(37, 67, INPUTS[1][2])[0].tolist()) == {G.GRAY_ROW4} and INPUTS[1][2] == (3, 5, 64, 30)


@pytest.mark.parametrize("at", range(len(INPUTS)), ids=[i[0] for i in INPUTS])
def test_both_decoders_through_the_front(ss, torch, at):
    name, maps, (x0, y0, w, h) = INPUTS[at]
    dmaps = None if maps is None else tuple(torch.from_numpy(m).cuda() for m in maps)

    def seen(stack):
        return (stack if maps is None else G.remap_stack(stack, *maps))[:, y0:y0 + h, x0:x0 + w]

    gray = G.random_stack(31, 14, 37, 67)
    want = G.decode(seen(gray), 13, 6, 5)
    assert 0 < (want[..., 0] >= 0).sum() < want[..., 0].size
    roi = (x0, y0, x0 + w, y0 + h)                                              # Gray code reads end coordinates
    got = ss.active.grayCodeDecode(gray, (13, 6), maps=maps, roi=roi)
    dev = ss.active.grayCodeDecode(torch.from_numpy(gray).cuda(), (13, 6), maps=dmaps, roi=roi)
    assert got.dtype == np.int32 and np.array_equal(got, want) and np.array_equal(dev.cpu().numpy(), want)

    phase = P.scene(41, (67, 37), T.PROJ, PERIODS)
    want, tie = P.decode(seen(phase), PERIODS, T.PROJ, details=True)
    assert tie.max() <= T.META["tie_max"]                                       # no k of the input hangs on a rounding
    got = ss.active.phaseShiftDecode(phase, PERIODS, T.PROJ, maps=maps, roi=(x0, y0, w, h))
    dev = ss.active.phaseShiftDecode(torch.from_numpy(phase).cuda(), PERIODS, T.PROJ, maps=dmaps, roi=(x0, y0, w, h))
    assert got.shape == want.shape == (h, w, 2) and not np.isnan(got).any() and not np.isnan(want).any()
    err = float(np.abs(got - want).max())
    print("%s: worst |p - restatement| %.3e (tolerance %.3e), worst tie %.3f" % (name, err, TOL, float(tie.max())))
    assert err <= TOL
    assert P.same_bits(dev.cpu().numpy(), got)
