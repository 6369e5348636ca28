#!/usr/bin/env python3
"""Is the device code of the working tree the device code of another revision?  (build container: CPU only)

    python tools/isa_compare.py [--map OLD=NEW]... [REV]          # REV defaults to HEAD~1

Exports REV's simplestereo_amd/csrc and include with `git archive`, compiles the translation units of
simplestereo_amd/build.py (its flags, its per-unit -mllvm options) of both trees to gfx950 assembly, and compares the
listings kernel by kernel: comments, blank lines and assembler directives are dropped, labels, instructions and each
kernel's descriptor (.amdhsa_*: registers, LDS, scratch) are kept.  Block labels carry the function's index in its unit
(.LBB<i>_<j>): the index is dropped, and so is the kernel's own entry label, so removing or renaming a kernel does not make
the others differ.  --map OLD=NEW (repeatable) replaces the substring OLD by NEW in REV's symbols before the kernels are
paired: a dropped template parameter changes the mangled names.  Prints one table row per unit and the names of the kernels
that differ or exist on one side only; exits 1 if there are any.
"""
import argparse
import io
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simplestereo_amd.build import HIPCC_FLAGS, UNITS  # noqa: E402

CSRC = os.path.join("simplestereo_amd", "csrc")


def start_listings(tree, out_dir):
    """One compiler process per unit of `tree`; returns [(unit, listing path, process)]."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + ["--cuda-device-only", "-S", "-Wno-unused-command-line-argument"]
    os.makedirs(out_dir)
    jobs = []
    for src, extra in UNITS:
        lst = os.path.join(out_dir, os.path.splitext(src)[0] + ".s")
        cmd = [hipcc] + flags + extra + ["-o", lst, os.path.join(tree, CSRC, src)]
        jobs.append((src, lst, subprocess.Popen(cmd)))
    return jobs


_TYPE = re.compile(r"\.type\s+(\S+),@function")
_DESC = re.compile(r"\.amdhsa_kernel\s+(\S+)")


_LBB = re.compile(r"\.LBB\d+_")


def kernels(listing, renames=()):
    """{symbol: (instruction and label lines, descriptor lines)} of one listing, its symbols renamed by (old, new) substrings."""
    out, name, desc = {}, None, None
    for raw in open(listing):
        line = raw.split(";", 1)[0].strip()
        for old, new in renames:
            line = line.replace(old, new)
        line = _LBB.sub(".LBB_", line)
        if not line or line == "%s:" % name:
            continue
        m = _TYPE.match(line)
        if m:
            name = m.group(1)
            out.setdefault(name, ([], []))
            continue
        m = _DESC.match(line)
        if m:
            desc = out.setdefault(m.group(1), ([], []))[1]
            continue
        if line == ".end_amdhsa_kernel":
            desc = None
        elif desc is not None:
            desc.append(" ".join(line.split()))
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name is not None and (not line.startswith(".") or line.endswith(":")):
            out[name][0].append(" ".join(line.split()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("rev", nargs="?", default="HEAD~1")
    ap.add_argument("--map", action="append", default=[], metavar="OLD=NEW", help="substring replacement in REV's symbols")
    args = ap.parse_args()
    renames = [tuple(m.split("=", 1)) for m in args.map]
    with tempfile.TemporaryDirectory(prefix="isa_compare_") as tmp:
        old_tree = os.path.join(tmp, "old")
        tar = subprocess.check_output(["git", "-C", ROOT, "archive", args.rev, CSRC, "include"])
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(old_tree)
        jobs = start_listings(old_tree, os.path.join(tmp, "lst_old")) + start_listings(ROOT, os.path.join(tmp, "lst_new"))
        failed = [p.args[-1] for _, _, p in jobs if p.wait() != 0]
        if failed:
            sys.exit("isa_compare: hipcc failed on " + ", ".join(failed))
        n = len(UNITS)
        bad = 0
        print(f"| unit | kernels {args.rev} / new | instructions {args.rev} / new | kernels differing |")
        print("|---|---|---|---|")
        for (src, lst_old, _), (_, lst_new, _) in zip(jobs[:n], jobs[n:]):
            old, new = kernels(lst_old, renames), kernels(lst_new)
            count = lambda ks: sum(1 for k in ks.values() for ln in k[0] if not ln.endswith(":"))
            diff = sorted(k for k in old.keys() | new.keys() if old.get(k) != new.get(k))
            print(f"| `{src}` | {len(old)} / {len(new)} | {count(old)} / {count(new)} | {len(diff)} |", flush=True)
            for k in diff:
                side = "" if k in old and k in new else " (only in %s)" % (args.rev if k in old else "the working tree")
                what = "" if side or old[k][0] != new[k][0] else " (descriptor only)"
                print(f"  differs: {k}{side}{what}")
            bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
