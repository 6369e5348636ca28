"""GPU tier: the ASW path does not depend on the host's libm.

Rounds 1-5 built the proximity tables with the host's `exp` and the sRGB byte table with the host's `powf`: on a host whose libm is
not glibc's FMA build the exact mode silently stopped returning the goldens' maps.  Since round 6 both tables come from glibc's
algorithms restated in csrc/glibc_math.hip.h (host side), as the device's weights always did.  Here the ASW operators run in a process
whose `exp`, `expf`, `exp2`, `exp2f`, `powf` are REPLACED by garbage (`pow` / `log` are left alone: the interpreter itself needs them) (an LD_PRELOAD shim compiled on the spot) and must
still return the reference's maps: G1 / G2 (Tsukuba, cases.npz) and the class-default photograph P4a (99.90 % on the fp32 path)."""
import json
import os
import shutil
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
/* every libm entry point the ASW path could be tempted to call returns garbage -- and counts the calls */
#include <stdio.h>
static volatile long calls;
double exp(double x) { ++calls; return 0.125 + x * 1e-3; }
float expf(float x) { ++calls; return 0.25f; }
double exp2(double x) { ++calls; return 3.0; }
float exp2f(float x) { ++calls; return 3.0f; }
float powf(float x, float y) { ++calls; return 0.5f; }
long ssamd_test_poisoned_libm_calls(void) { return calls; }
"""

DRIVER = r"""
import ctypes, json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
shim = ctypes.CDLL(sys.argv[2])
libm = ctypes.CDLL("libm.so.6"); libm.exp.restype = ctypes.c_double; libm.exp.argtypes = [ctypes.c_double]
import simplestereo_amd as ss
G = os.path.join(sys.argv[1], "tests", "golden")
maps = np.load(os.path.join(G, "cases.npz")); meta = json.load(open(os.path.join(G, "cases.json")))
z = np.load(os.path.join(G, "tsukuba_pair.npz"))
L, R = np.ascontiguousarray(z["left"]), np.ascontiguousarray(z["right"])
out = {"poison_active": ctypes.CDLL(None).exp is not None}
# is the poison really what a C caller of exp() in this process gets?
e = ctypes.CDLL(None).exp; e.restype = ctypes.c_double; e.argtypes = [ctypes.c_double]
out["exp_of_1"] = e(1.0)
for cid in ("G1", "G2"):
    p = {k: v for k, v in meta[cid]["params"].items() if k != "algo"}
    d = ss.passive.StereoASW(**p).compute(L, R)
    out[cid] = int(np.count_nonzero(d != maps[cid]))
pm = json.load(open(os.path.join(G, "photo_cases.json")))["P4a"]
pairs = np.load(os.path.join(G, "photo_pairs.npz"))
a, b = np.ascontiguousarray(pairs[pm["pair"] + "_L"]), np.ascontiguousarray(pairs[pm["pair"] + "_R"])
p = {k: v for k, v in pm["params"].items() if k != "algo"}
d = ss.passive.StereoASW(**p).compute(a, b)
out["P4a"] = int(np.count_nonzero(d != np.load(os.path.join(G, "photo_cases.npz"))["P4a"]))
d32 = ss.passive.StereoASW(exact=False, **p).compute(a, b)
out["P4a_fp32"] = int(np.count_nonzero(d32 != np.load(os.path.join(G, "photo_cases.npz"))["P4a"]))
print("RESULT " + json.dumps(out))
"""


@pytest.mark.skipif(shutil.which("gcc") is None, reason="needs gcc for the LD_PRELOAD shim")
def test_asw_maps_with_the_process_libm_poisoned(tmp_path):
    src = tmp_path / "poison.c"
    src.write_text(SHIM)
    so = tmp_path / "libpoison.so"
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-fno-builtin", "-o", str(so), str(src)])
    drv = tmp_path / "driver.py"
    drv.write_text(DRIVER)
    # the shim goes first; whatever the environment already preloads stays preloaded behind it
    preload = " ".join([str(so)] + ([os.environ["LD_PRELOAD"]] if os.environ.get("LD_PRELOAD") else []))
    env = dict(os.environ, LD_PRELOAD=preload, SSAMD_AUTOTUNE="0")
    r = subprocess.run([sys.executable, str(drv), ROOT, str(so)], capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert abs(res["exp_of_1"] - 0.126) < 1e-9, res                 # the shim IS what exp() resolves to in that process
    assert res["G1"] == 0 and res["G2"] == 0 and res["P4a"] == 0, res
    assert res["P4a_fp32"] > 0                                      # (the fp32 argmin alone misses pixels there: the pass did the work)
