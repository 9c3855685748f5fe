#!/usr/bin/env python
"""Build tools/cut_points_host.cpp (the walk of csrc/cut_points.hip as a host program) and run it over the case list of
tests/_cut_points_ref.py: every table must equal the numpy mirror's, and --adversarial must exit 0.  No GPU, nothing loaded into Python.

    python tools/cut_points_host.py [--sanitize] [--cxx c++] [--keep DIR]

--sanitize builds with -fsanitize=address,undefined (the stand-alone binary carries its own runtime)."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _cut_points_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--cxx", default=os.environ.get("CXX", "c++"))
    ap.add_argument("--keep", default=None, help="directory for the binary and the case files (default: a temporary one)")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="cut_points_host_")
    os.makedirs(tmp, exist_ok=True)
    exe = os.path.join(tmp, "cut_points_host")
    cmd = [args.cxx, "-O1", "-g", "-std=c++20", "-pthread", "-I" + os.path.join(ROOT, "voice100_amd", "csrc"),
           os.path.join(ROOT, "tools", "cut_points_host.cpp"), "-o", exe]
    if args.sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True)
    rows = []
    for name, x, lengths, kw in R.case_list():
        B, T, V = x.shape
        for b in range(B):
            n = T if lengths is None else int(min(max(int(lengths[b]), 0), T))
            rows.append((f"{name} [{b}]", x[b], n, kw))
    fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "tables.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(rows)))
        for _, x, n, kw in rows:
            gap = kw.get("min_gap", 25)
            f.write(struct.pack("<6if", x.shape[0], n, kw.get("max_frames", 3000), 0 if gap is None else gap, kw.get("pad", 5),
                                kw.get("min_frames", 50), kw.get("margin", 0.0)))
            f.write(R.margins(x[:n], kw.get("blank", 0)).astype("<f4").tobytes())
    subprocess.run([exe, fin, fout], check=True)
    got = np.fromfile(fout, dtype="<i4")
    at, bad = 0, 0
    for name, x, n, kw in rows:
        s, e, f, cnt = R.mirror(x[None, :max(n, 1)], [n], **kw)
        k = int(got[at])
        tab = got[at + 1:at + 1 + 3 * k].reshape(3, k)
        past = got[at + 1 + 3 * k:at + 3 + 3 * k]
        at += 3 + 3 * k
        ok = k == int(cnt[0]) and np.array_equal(tab[0], s[0]) and np.array_equal(tab[1], e[0]) and np.array_equal(tab[2], f[0]) and not past.any()
        bad += not ok
        if not ok:
            print(f"MISMATCH {name}: {k} segments, the mirror has {int(cnt[0])}")
    assert at == got.size
    print(f"{len(rows)} rows, {bad} differ from the mirror")
    subprocess.run([exe, "--adversarial"], check=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
