"""Record the reference's phase unwrapper (``simplestereo._unwrapping.infiniteImpulseResponse``) on exact inputs.

    python tests/golden/make_golden_unwrap.py /path/to/_unwrapping.cpython-XY-x86_64-linux-gnu.so

The module is the reference's ``simplestereo/_unwrapping.cpp`` compiled OUTSIDE this tree, e.g.

    g++ -O2 -fpermissive -shared -fPIC -I"$(python -c 'import sysconfig; print(sysconfig.get_paths()["include"])')" \\
        -I"$(python -c 'import numpy; print(numpy.get_include())')" simplestereo/_unwrapping.cpp \\
        -o /tmp/ref/_unwrapping"$(python -c 'import sysconfig; print(sysconfig.get_config_var("EXT_SUFFIX"))')"

(-fpermissive: the numpy 2 headers need it; a plain x86-64 -O2 build, so no fused multiply-adds.)  The reference's flag
allocation writes past its first row (``_unwrapping.cpp:80-93``) and corrupts the heap, so every case runs in a FRESH child
process and calls from a FRESH thread (its own malloc arena); a case whose child still dies is skipped and listed.  Every
surviving output is asserted bit-identical to ``tests/_unwrap_ref.py`` before it is written.

Writes ``unwrap_cases.npz`` (small cases: input and output), ``unwrap_cases.json`` (every case: recipe, tau, sha256 of input and
output; the full frames and the widest maps by sha256 only) and ``unwrap_errors.json`` (the exceptions of the checks).

Inputs use only ``+ * fmod`` on dyadic coefficients and an explicit integer hash (no sin, no numpy generator streams), so
``phase_input(recipe)`` rebuilds them bit for bit anywhere.
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))          # tests/: _unwrap_ref


def _hash(y, x, seed):
    """32-bit integer hash of (y, x, seed), uint64 arithmetic modulo 2^64 (explicit: no generator streams)."""
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    v = (y.astype(np.uint64) * np.uint64(0x9E3779B1) + x.astype(np.uint64) * np.uint64(0x85EBCA77) + np.uint64(seed) * np.uint64(0xC2B2AE3D)) & M
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(12)
    v = (v * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    v ^= v >> np.uint64(15)
    return v


def phase_input(recipe):
    """recipe = dict(h, w, seed, ax, ay, axy, noise, wrap, special): ax*x + ay*y + axy*x*y + noise*(hash - 2^15) 2^-16, reduced
    by fmod(., 2 pi) when wrap; coefficients are dyadic, so every product below is exact and the few sums are ordinary fp64
    additions.  special = 1 puts NaN / +inf / -inf at hashed positions."""
    h, w = recipe["h"], recipe["w"]
    y, x = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    noise = (_hash(y, x, recipe["seed"]) & np.uint64(0xFFFF)).astype(np.float64) + (-32768.0)
    v = x.astype(np.float64) * recipe["ax"] + y.astype(np.float64) * recipe["ay"]
    v = v + (x * y).astype(np.float64) * recipe["axy"]
    v = v + noise * (recipe["noise"] * 2.0 ** -16)
    if recipe["wrap"]:
        v = np.fmod(v, 2 * np.pi)
    if recipe.get("special"):
        k = _hash(y, x, recipe["seed"] + 7) % np.uint64(23)
        v[k == 0] = np.nan
        v[k == 1] = np.inf
        v[k == 2] = -np.inf
    return np.ascontiguousarray(v, dtype=np.float64)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def sha_canonical_nan(a):
    a = np.array(a, dtype=np.float64)
    a[np.isnan(a)] = np.nan
    return sha(a)


def _recipe(h, w, seed, ax=0.4375, ay=0.3125, axy=0.0, noise=0.5, wrap=1, special=0):
    return dict(h=h, w=w, seed=seed, ax=ax, ay=ay, axy=axy, noise=noise, wrap=wrap, special=special)


# (name, recipe, tau, stored whole)
CASES = []
for i, (h, w) in enumerate([(1, 1), (1, 7), (1, 50), (7, 1), (50, 1), (2, 2), (2, 3), (3, 2), (5, 1), (33, 65), (64, 80), (37, 53)]):
    for tau in (1.0, 0.8) if h * w > 4 else (1.0, 0.25):
        CASES.append(("s%dx%d_t%g" % (h, w, tau), _recipe(h, w, 10 + i), tau, True))
# band edges of the kernel (bands of up to 1024 rows; narrower maps than ~40 columns crash the reference's heap)
for i, h in enumerate((63, 64, 65, 1023, 1024, 1025)):
    CASES.append(("band%d" % h, _recipe(h, 40, 40 + i, ax=1.0625, ay=0.5625), 0.8, h < 100))
for tau in (0.0, 0.25, 0.5, 0.8, 1.0):
    CASES.append(("tau%g" % tau, _recipe(24, 40, 60, ax=0.8125, ay=-0.6875, axy=0.015625, noise=1.5), tau, True))
CASES.append(("ramp", _recipe(4, 2500, 70, ax=1.6875, ay=0.25, noise=0.25), 1.0, True))          # |u| ~ 4200 rad
CASES.append(("ramp_t05", _recipe(4, 2500, 71, ax=1.6875, ay=0.25, noise=0.25), 0.5, False))
CASES.append(("big", _recipe(20, 30, 80, ax=137.5, ay=-311.25, axy=1.5, noise=2.0 ** 13, wrap=0), 0.8, True))   # |phase| ~ 1e4
CASES.append(("big_t1", _recipe(20, 30, 81, ax=-263.0, ay=171.75, noise=2.0 ** 14, wrap=0), 1.0, True))
CASES.append(("special", _recipe(40, 64, 90, special=1), 0.8, True))
CASES.append(("frame1080", _recipe(1080, 1920, 100, ax=0.0859375, ay=0.03125, axy=2.0 ** -12), 0.8, False))
CASES.append(("frame2160", _recipe(2160, 4096, 101, ax=0.0703125, ay=-0.046875, axy=2.0 ** -13), 1.0, False))
# the kernel's widest map with its tallest band (LDS line of 16384 doubles + 2 x 1024 exchange slots = 147456 bytes), and a
# wide map with NaN / +-inf (a line of 12000 doubles: above 64 KiB; two bands of rows when the band height is capped at 64)
CASES.append(("frame_wide16384", _recipe(1024, 16384, 102, ax=0.0390625, ay=0.0546875, axy=2.0 ** -14), 0.8, False))
CASES.append(("frame_wide_special", _recipe(70, 12000, 103, ax=0.0703125, ay=0.3125, special=1), 0.8, False))

_CHILD = r"""
import sys, threading, importlib.util, numpy as np
spec = importlib.util.spec_from_file_location("_unwrapping", sys.argv[1])
mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
ph = np.load(sys.argv[2]); tau = float(sys.argv[4]); res = {}
def run():
    res["out"] = mod.infiniteImpulseResponse(ph, tau)
t = threading.Thread(target=run); t.start(); t.join()
np.save(sys.argv[3], np.asarray(res["out"], dtype=np.float64))
"""

_PROBE = r"""
import sys, json, threading, importlib.util, numpy as np
spec = importlib.util.spec_from_file_location("_unwrapping", sys.argv[1])
mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
args = eval(sys.argv[2], {"np": np, "nan": float("nan")}); res = {}
def run():
    try:
        out = mod.infiniteImpulseResponse(*args)
        res["r"] = {"result": "accepted", "all_nan": bool(np.isnan(np.asarray(out)).all())}
    except Exception as e:
        res["r"] = {"result": "raised", "type": type(e).__name__, "message": str(e)}
t = threading.Thread(target=run); t.start(); t.join()
print(json.dumps(res["r"]))
"""

# (probe id, python expression of the argument tuple, evaluated with np and nan)
PROBES = [
    ("list_phase", "([[0.0, 1.0], [2.0, 3.0]], 1.0)"),
    ("list_phase_bad_tau", "([[0.0, 1.0], [2.0, 3.0]], 5.0)"),
    ("tau_str", "(np.zeros((2, 3)), 'a')"),
    ("tau_numeric_str", "(np.zeros((2, 3)), '0.5')"),
    ("tau_none", "(np.zeros((2, 3)), None)"),
    ("phase_1d", "(np.zeros(5), 1.0)"),
    ("phase_3d", "(np.zeros((2, 3, 4)), 1.0)"),
    ("phase_3d_bad_tau", "(np.zeros((2, 3, 4)), 5.0)"),
    ("tau_negative", "(np.zeros((2, 3)), -0.1)"),
    ("tau_above_one", "(np.zeros((2, 3)), 1.5)"),
    ("tau_int", "(np.arange(6.0).reshape(2, 3), 1)"),
    ("tau_int_zero", "(np.arange(6.0).reshape(2, 3), 0)"),
    ("tau_bool", "(np.arange(6.0).reshape(2, 3), True)"),
    ("tau_nan", "(np.arange(6.0).reshape(2, 3), nan)"),
]


def main(modpath):
    import _unwrap_ref
    tmp = tempfile.mkdtemp()
    meta, arrays, skipped = {}, {}, []
    for name, recipe, tau, whole in CASES:
        ph = phase_input(recipe)
        fin, fout = os.path.join(tmp, name + "_in.npy"), os.path.join(tmp, name + "_out.npy")
        np.save(fin, ph)
        p = subprocess.run([sys.executable, "-c", _CHILD, modpath, fin, fout, repr(tau)], capture_output=True, text=True)
        if p.returncode != 0:
            skipped.append({"case": name, "returncode": p.returncode, "stderr": p.stderr.strip().splitlines()[-1:] })
            print("skip", name, p.returncode, p.stderr.strip()[-200:])
            continue
        out = np.load(fout)
        ref = _unwrap_ref.unwrap(ph, tau)
        assert _unwrap_ref.identical(out, ref), name
        meta[name] = dict(recipe=recipe, tau=tau, whole=whole, input_sha256=sha(ph), output_sha256=sha(out))
        if not whole and np.isnan(out).any():
            # NaN sign and payload are the processor's business (x86 makes inf - inf a negative NaN): a map stored by hash
            # alone also gets the hash of its output with every NaN replaced by numpy's
            meta[name]["output_sha256_canonical_nan"] = sha_canonical_nan(out)
        if whole:
            arrays[name + "__in"] = ph
            arrays[name + "__out"] = out
        print("ok", name, ph.shape, "max|u| %.1f" % float(np.nanmax(np.abs(np.where(np.isfinite(out), out, 0)))))
    np.savez_compressed(os.path.join(HERE, "unwrap_cases.npz"), **arrays)
    with open(os.path.join(HERE, "unwrap_cases.json"), "w") as f:
        json.dump({"cases": meta, "skipped": skipped}, f, indent=1, sort_keys=True)
    errors = []
    for pid, expr in PROBES:
        p = subprocess.run([sys.executable, "-c", _PROBE, modpath, expr], capture_output=True, text=True)
        assert p.returncode == 0, (pid, p.returncode, p.stderr[-300:])
        errors.append(dict(id=pid, args=expr, **json.loads(p.stdout.strip().splitlines()[-1])))
        print(pid, errors[-1])
    with open(os.path.join(HERE, "unwrap_errors.json"), "w") as f:
        json.dump(errors, f, indent=1)


if __name__ == "__main__":
    main(os.path.abspath(sys.argv[1]))
