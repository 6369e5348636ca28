"""The GSW parameter-edge fixture (tests/golden/gsw_edge_cases.{json,npz}, recorded from the reference by
tests/golden/make_golden_gsw_edges.py): its cases with their generated inputs."""
import hashlib
import importlib.util
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

_spec = importlib.util.spec_from_file_location("make_golden_gsw_edges", os.path.join(GOLDEN, "make_golden_gsw_edges.py"))
recorder = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(recorder)

with open(os.path.join(GOLDEN, "gsw_edge_cases.json")) as _f:
    META = json.load(_f)
CASE_IDS = sorted(META)
_inputs = None


def params(cid):
    """the case's keyword arguments for oracle.gsw / StereoGSW (fMax is text in the fixture: "nan", "inf", "-0.0")"""
    p = dict(META[cid]["params"])
    p["fMax"] = float(p["fMax"])
    return p


def pair(cid):
    """the case's generated image pair, checked against the hash the recorder saw"""
    global _inputs
    if _inputs is None:
        _inputs = recorder.inputs()
    a, b = _inputs[META[cid]["input"]]
    assert hashlib.sha256(a.tobytes() + b.tobytes()).hexdigest() == META[cid]["input_sha256"], cid
    return a, b


def recorded_maps():
    with np.load(os.path.join(GOLDEN, "gsw_edge_cases.npz")) as z:
        return {k: z[k] for k in z.files}
