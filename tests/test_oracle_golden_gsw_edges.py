"""CPU tier: the oracle against what the unmodified reference answered at the edges of GSW's parameters (negative and
overflowing gammas, zero / negative / infinite / subnormal / NaN caps, no relaxation at all), with the literal relaxation loops
and with the closed-form weights alike.  The reference returns only the map after its left-right check and filling; an oracle
that reproduces every one of these maps line by line is what tests/test_gpu_gsw_raw.py takes the RAW winners from."""
import hashlib

import numpy as np
import pytest

import _gsw_edges as edges


@pytest.fixture(scope="module")
def maps():
    return edges.recorded_maps()


def test_fixture_is_complete(maps):
    assert sorted(maps) == edges.CASE_IDS and len(edges.CASE_IDS) == 2 * 14
    assert sorted(edges.recorder.parameter_sets()) == sorted({c.split("__", 1)[1] for c in edges.CASE_IDS})
    for cid, d in maps.items():
        assert d.dtype == np.int16 and list(d.shape) == edges.META[cid]["shape"]
        assert hashlib.sha256(d.tobytes()).hexdigest() == edges.META[cid]["sha256"], cid
        assert edges.META[cid]["params"] == edges.recorder.parameter_sets()[cid.split("__", 1)[1]]


@pytest.mark.parametrize("closed", [False, True], ids=["literal", "closed"])
@pytest.mark.parametrize("cid", edges.CASE_IDS)
def test_oracle_equals_the_reference_at_parameter_edges(cid, closed, maps):
    from oracle import oracle
    a, b = edges.pair(cid)
    d, left, right = oracle.gsw(a, b, closed=closed, return_raw=True, **edges.params(cid))
    assert np.array_equal(d, maps[cid])
    assert np.array_equal(d, oracle.gsw(a, b, closed=closed, **edges.params(cid)))      # the raw outputs change nothing
    W = a.shape[1]
    assert left.min() >= 0 and right.min() >= 0 and right.max() <= W - 1
    assert (left <= np.arange(W)[None, :]).all()                                          # x - dBest with 0 <= dBest <= x


def test_nan_cap_and_unreached_infinite_weights_win_nothing(maps):
    """what the two degenerate sets mean in the raw winners: every cost NaN (or inf), dBest stays 0 in both passes"""
    from oracle import oracle
    for cid in ("noise_16x40__fmax_nan", "noise_16x40__gamma_-7_iterations_0", "synth_20x48__fmax_nan"):
        a, b = edges.pair(cid)
        _, left, right = oracle.gsw(a, b, closed=False, return_raw=True, **edges.params(cid))
        assert np.array_equal(left, np.broadcast_to(np.arange(a.shape[1], dtype=np.int16), left.shape)), cid
        assert not right.any(), cid
