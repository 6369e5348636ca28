"""GPU tier: the order and the wording of the argument checks at the C ABI are pinned.  tests/golden/abi_errors.json holds the
return code and the ssamd_last_error() text of every call of tests/golden/make_golden_abi_errors.py, most of which break two rules
at once, as the library answered them BEFORE its host side was cut into sections.  No call gets as far as a kernel launch: buffers
of a few hundred bytes, images of 8 x 16."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FAMILIES = ["np_unwrap", "ftp_cloud", "ftp_phase", "iir_unwrap", "device_matchers", "rig", "host_matchers", "library"]


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_abi_errors", os.path.join(GOLDEN, "make_golden_abi_errors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "abi_errors.json")) as f:
        return _recorder(), json.load(f)


def test_the_fixture_holds_the_cases_of_its_recorder(recorded):
    rec, rows = recorded
    assert [{k: r[k] for k in ("family", "entry", "args")} for r in rows] == rec.CASES
    assert sorted({r["family"] for r in rows}) == sorted(FAMILIES)
    assert all((r["error"] is None) == (r["rc"] == 0) for r in rows)


@pytest.mark.parametrize("family", FAMILIES)
def test_return_code_and_message_of_every_bad_call(recorded, family):
    from simplestereo_amd import _native
    rec, rows = recorded
    bad = []
    for r in (r for r in rows if r["family"] == family):
        rc, err = rec.call(r, _native)
        if (rc, err) != (r["rc"], r["error"]):
            bad.append("%s%r: got %d %r, recorded %d %r" % (r["entry"], tuple(r["args"]), rc, err, r["rc"], r["error"]))
    assert not bad, "\n".join(bad)
