#!/usr/bin/env python
"""Build tools/mbr_host.cpp (the bodies of csrc/mbr.hip as a host program) and run it over the case list of tests/_mbr_ref.py: every
integer output must equal the float64 oracle's, every float lie within its bound, and --adversarial (lens beyond T and negative, rows
of separators only, ids at the int64 extremes, NaN and +-inf scores, poisoned workspaces) must exit 0.  No GPU, nothing loaded into Python.

    python tools/mbr_host.py [--sanitize] [--cxx c++] [--keep DIR]

--sanitize builds with -fsanitize=address,undefined (the stand-alone binary carries its own runtime)."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mbr_ref as R  # noqa: E402


def build(cxx, exe, sanitize=False):
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "voice100_amd", "csrc"), "-x", "c++",
           os.path.join(ROOT, "tools", "mbr_host.cpp"), "-o", exe]
    if sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True)


def run_cases(exe, tmp, cases):
    """the messages of what differs from the oracle on `cases`"""
    fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "results.bin")
    with open(fin, "wb") as f:
        R.write_cases(f, cases)
    subprocess.run([exe, fin, fout], check=True)
    bad = []
    for (name, ids, lens, scores, kw), got in zip(cases, R.read_results(open(fout, "rb").read(), cases)):
        bad += R.check(name, got, R.oracle(ids, lens, scores, **kw), ids, lens, scores)[0]
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--cxx", default=os.environ.get("CXX", "c++"))
    ap.add_argument("--keep", default=None, help="directory for the binary and the case files (default: a temporary one)")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="mbr_host_")
    os.makedirs(tmp, exist_ok=True)
    exe = os.path.join(tmp, "mbr_host")
    build(args.cxx, exe, args.sanitize)
    cases = R.case_list()
    bad = run_cases(exe, tmp, cases)
    for line in bad:
        print("MISMATCH", line)
    print(f"{len(cases)} cases, {len(bad)} differences from the oracle")
    subprocess.run([exe, "--adversarial"], check=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
