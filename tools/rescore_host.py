#!/usr/bin/env python
"""Build tools/rescore_host.cpp (the body of csrc/rescore.hip as a host program) and run it over the case list of tests/_rescore_ref.py:
every count and rank must equal the float64 oracle's, every score lie within its bound, and --adversarial (damaged tables) must exit 0.
No GPU, nothing loaded into Python.

    python tools/rescore_host.py [--sanitize] [--cxx c++] [--keep DIR]

--sanitize builds with -fsanitize=address,undefined (the stand-alone binary carries its own runtime)."""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rescore_ref as R  # noqa: E402


def write_case(f, lm, ids, lens, scores, kw):
    B, nbest, T = ids.shape
    pool = lm.pool.numpy()[:lm.pool_len]
    wtab, ng = lm.word_table.numpy().reshape(-1), lm.ngram_table.numpy()
    f.write(struct.pack("<10i", B, nbest, T, lm.order, int(lm.has_bos), int(lm.has_eos), int(kw.get("use_eos", True)), pool.size,
                        wtab.size, ng.size))
    f.write(struct.pack("<qdd", kw.get("sep", R.SEP), kw.get("lm_weight", 0.5), kw.get("word_bonus", 0.0)))
    for a, dt in ((lm.meta, "<i8"), (pool, "<i8"), (wtab, "<i4"), (ng, "<i4"), (ids, "<i8"), (lens, "<i4"), (scores, "<f4")):
        f.write(np.ascontiguousarray(a).astype(dt).tobytes())


def compare(name, got, ref, ids, lens, scores):
    """The checks of tests/test_gpu_rescore.py on one case; returns the messages of what differs."""
    bad = []
    order = got["order"].astype(np.int64)
    for k in ("order", "n_words", "n_oov"):
        if not np.array_equal(got[k], ref[k]):
            bad.append(f"{name}: {k} differs from the oracle")
    rows = np.arange(ids.shape[0])[:, None]
    if not (np.array_equal(got["ids"], ids[rows, order]) and np.array_equal(got["lens"], lens[rows, order])
            and np.array_equal(got["first"].view(np.int32), scores[rows, order].view(np.int32))):
        bad.append(f"{name}: ids, lens or first_scores are not the gather by order")
    for k, b in (("scores", "bound_score"), ("word_lm_scores", "bound_lm")):
        both_inf = np.isinf(ref[k]) & (got[k] == ref[k])
        with np.errstate(invalid="ignore"):              # (-inf) - (-inf) where both say "no hypothesis"
            err = np.where(both_inf, 0.0, np.abs(got[k].astype(np.float64) - ref[k]))
        if not np.all(err <= ref[b]):
            bad.append(f"{name}: {k} is {float(np.nanmax(err / np.maximum(ref[b], 1e-300))):.3g} bounds away")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sanitize", action="store_true")
    ap.add_argument("--cxx", default=os.environ.get("CXX", "c++"))
    ap.add_argument("--keep", default=None, help="directory for the binary and the case files (default: a temporary one)")
    args = ap.parse_args()
    tmp = args.keep or tempfile.mkdtemp(prefix="rescore_host_")
    os.makedirs(tmp, exist_ok=True)
    exe = os.path.join(tmp, "rescore_host")
    cmd = [args.cxx, "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "voice100_amd", "csrc"), "-x", "c++",
           os.path.join(ROOT, "tools", "rescore_host.cpp"), "-o", exe]
    if args.sanitize:
        cmd[1:1] = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    subprocess.run(cmd, check=True)
    cases = R.case_list()
    lm, packed = R.flip_case()
    cases = cases + [("the planted flip", lm, packed[0], packed[1], packed[2], {})]
    fin, fout = os.path.join(tmp, "cases.bin"), os.path.join(tmp, "results.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for _, lm, ids, lens, scores, kw in cases:
            write_case(f, lm, ids, lens, scores, kw)
    subprocess.run([exe, fin, fout], check=True)
    raw = open(fout, "rb").read()
    at, bad = 0, []
    for name, lm, ids, lens, scores, kw in cases:
        B, nbest, T = ids.shape
        got = {}
        for k, dt, n in (("order", "<i4", B * nbest), ("n_words", "<i4", B * nbest), ("n_oov", "<i4", B * nbest), ("lens", "<i4", B * nbest),
                         ("scores", "<f4", B * nbest), ("first", "<f4", B * nbest), ("word_lm_scores", "<f4", B * nbest), ("ids", "<i8", B * nbest * T)):
            got[k] = np.frombuffer(raw, dtype=dt, count=n, offset=at).reshape((B, nbest, T) if k == "ids" else (B, nbest))
            at += n * np.dtype(dt).itemsize
        bad += compare(name, got, R.oracle(lm, ids, lens, scores, **kw), ids, lens, scores)
    assert at == len(raw)
    for line in bad:
        print("MISMATCH", line)
    print(f"{len(cases)} cases, {len(bad)} differences from the oracle")
    subprocess.run([exe, "--adversarial"], check=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
