#!/usr/bin/env python3
"""Time the resumable beam search (decode.ctc_beam_search_long / CTCBeamStream, the STREAM form of csrc/beam.hip, K32) beside the one
call it must equal and beside K31's cut-and-batch decode, and check that the one call itself pays nothing for it.

Arms, all in one process, alternating over --rounds rounds:
  (a) ctc_beam_search_long(chunk=4096) beside ctc_beam_search on the same 32 x 4096 x 29 seeded logits, beams 4 / 16 / 64, without
      and with an order-3 NGramLM.fit model: one push and one read against one launch.  Expected at 1.0;
  (b) the same at chunk=256: 16 pushes, i.e. the overhead per push (the slice's copy, the launch, the state's round trip);
  (c) one and four planted 30-minute recordings (90 000 frames, tools/bench_transcribe_long.py's generator) at beam 16, without and
      with the LM, through ctc_beam_search_long, beside LongASRPipeline.segments(timed=False) of the same logits (K31: cut at the
      pauses, decode the pieces as a batch).  The long form is serial per recording, so it is expected to be tens of times SLOWER;
      it buys exactness and one LM context.  How many of the recordings give the same best transcript either way is reported;
  (d) tools/bench_beam.py's headline shape (32 x 512 x 29 seeded, beams 4 / 16 / 64): v100_ctc_beam_search called through this tree's
      library and, with --parent-lib, through a library built from the parent commit, same tensors, same process.  Must be 1.0.
Before anything is timed the outputs of the two sides of (a), (b) and (d) must be equal bit for bit.  A timing is a window of
back-to-back calls between two device events; per arm every round, the median and the spread (max - min) / median are reported;
a ratio counts only beyond the project's bar, max(3 %, 3 x the larger spread).
Not measured here: a profiler run, a trained model, real recordings.
    python tools/bench_beam_stream.py [--rounds 5] [--parent-lib PATH] [--out profiles/beam_stream_bench.json]
    python tools/bench_beam_stream.py --resources-only      # no GPU: the compiler's resource report of beam.hip, into the same file
"""
import argparse
import ctypes
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

V = 29
WIDTHS = (4, 16, 64)
CUT = dict(max_frames=3000, min_gap=25, margin=0.0, pad=5, min_frames=50)


def resource_report():
    """VGPRs, SGPRs, scratch and static LDS of the four instantiations, from hipcc's -Rpass-analysis=kernel-resource-usage."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "voice100_amd", "csrc", "beam.hip")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.dirname(src),
           "-mllvm", "-pragma-unroll-threshold=1000000", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-c", src,
           "-o", os.devnull]
    text = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: \S*ctc_beam_kernelILb(\d)ELb(\d)E", line)
        if m:
            name = ("lm" if m.group(1) == "1" else "plain") + ("_stream" if m.group(2) == "1" else "")
            out[name] = {}
        for key, pat in (("vgprs", r" VGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"),
                         ("scratch_bytes_per_lane", r"ScratchSize \[bytes/lane\]: (\d+)"), ("static_lds_bytes", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("occupancy_waves_per_simd", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                out[name][key] = int(m.group(1))
    return out


def window(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                                 # ms per call


def summary(times):
    med = statistics.median(times)
    return {"rounds_ms": [round(t, 4) for t in times], "median_ms": round(med, 4), "spread": round((max(times) - min(times)) / med, 4)}


def ratio(res, num, den):
    bar = max(0.03, 3 * max(res[num]["spread"], res[den]["spread"]))
    r = res[num]["median_ms"] / res[den]["median_ms"]
    return {"ratio": round(r, 4), "bar": round(bar, 4), "inside_the_bar": bool(abs(r - 1) <= bar)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libvoice100_hip.so built from the parent commit, for arm (d)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_stream_bench.json"))
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    prior = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            prior = json.load(f)
    if args.resources_only:
        prior["compiler_resource_report"] = resource_report()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(prior, indent=1) + "\n")
        print(json.dumps(prior["compiler_resource_report"], indent=1))
        return
    import numpy as np
    import torch
    import _cut_points_ref as cut_ref
    from _beam_ref import seeded_logits
    from voice100_amd import _native as N
    from voice100_amd.decode import ctc_beam_search, ctc_beam_search_long
    from voice100_amd.infer import LongASRPipeline, join_ids
    from voice100_amd.lm import NGramLM
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_stream.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")

    def bits(t):
        return t.view(torch.int32) if t.dtype == torch.float32 else t

    def equal(a, b):
        return len(a) == len(b) and all(torch.equal(bits(p), bits(q)) for p, q in zip(a, b))

    # (c)'s recordings first: the LM is fitted on the first one's text, as in tools/bench_transcribe_long.py
    T_LONG = 90000
    rows = [cut_ref.planted(200 + b, T_LONG, V, speech=(100, 300), amp=20.0) for b in range(4)]
    long_logits = torch.from_numpy(np.stack([r[0] for r in rows])).to(dev)
    tab = cut_ref.mirror(rows[0][0][None], None, **CUT)
    texts = []
    for s, e in zip(tab[0][0], tab[1][0]):
        seq = rows[0][1][s:e]
        seq = seq[np.concatenate([[True], seq[1:] != seq[:-1]])]
        texts.append([int(v) for v in seq if v != 0])
    lm = NGramLM.fit(texts, V, 3).compile().to(dev)
    lms = {"plain": {}, "lm": dict(lm=lm)}

    arms, checks = {}, {}
    # (a), (b)
    T = 4096
    for w in WIDTHS:
        x = torch.from_numpy(seeded_logits(T, V, w, 3, 32)).to(dev)
        for kind, kw in lms.items():
            want = ctc_beam_search(x, None, w, 1, **kw)
            for chunk in (4096, 256):
                checks[f"long_chunk{chunk}_{kind}_W{w}_equals_one_call"] = equal(ctc_beam_search_long(x, None, w, 1, chunk=chunk, **kw), want)
                arms[f"long_chunk{chunk}_{kind}_W{w}"] = (lambda x=x, w=w, kw=kw, chunk=chunk: ctc_beam_search_long(x, None, w, 1, chunk=chunk, **kw), 2)
            arms[f"one_call_{kind}_W{w}"] = (lambda x=x, w=w, kw=kw: ctc_beam_search(x, None, w, 1, **kw), 2)
    # (c)
    agreement = {}
    for kind, kw in lms.items():
        pipe = LongASRPipeline(None, frame_seconds=0.02, beam_size=16, **kw, **CUT)
        same = 0
        for b in range(4):
            ids, n = ctc_beam_search_long(long_logits[b:b + 1], None, 16, 1, **kw)[:2]
            seg = pipe.segments(logits=long_logits[b], timed=False)
            sids, sn = seg["ids"].cpu(), seg["ids_len"].cpu()
            joined = join_ids([sids[i, :int(sn[i])].tolist() for i in range(sids.shape[0])], None)
            same += ids[0, 0, :int(n[0, 0])].cpu().tolist() == joined
        agreement[f"beam16_{kind}"] = {"recordings": 4, "best_transcript_equals_cut_and_batch": same}
        for nrec in (1, 4):
            x = long_logits[:nrec].contiguous()
            arms[f"long_{nrec}x90000_{kind}_W16"] = (lambda x=x, kw=kw: ctc_beam_search_long(x, None, 16, 1, **kw), 1)
            arms[f"cut_and_batch_{nrec}x90000_{kind}_W16"] = (lambda p=pipe, nrec=nrec: [p.segments(logits=long_logits[b], timed=False)
                                                                                     for b in range(nrec)], 1)
    # (d): the C entry point through this tree's library and through the parent's
    protos = N.parse_header()["v100_ctc_beam_search"]
    libs = {"this_tree": N.load()}
    if args.parent_lib:
        libs["parent"] = ctypes.CDLL(os.path.abspath(args.parent_lib))
    T_HEAD = 512
    for w in WIDTHS:
        x = torch.from_numpy(seeded_logits(T_HEAD, V, w, 3, 32)).to(dev)
        outs = {}
        for tag, lib in libs.items():
            fn = lib.v100_ctc_beam_search
            fn.argtypes, fn.restype = [t for t, _ in protos], ctypes.c_int
            ws = torch.empty((N.helper("v100_ctc_beam_workspace_bytes", 32, T_HEAD, V, w),), dtype=torch.uint8, device=dev)
            ids = torch.empty((32, 1, T_HEAD), dtype=torch.int64, device=dev)
            n, sc = torch.empty((32, 1), dtype=torch.int32, device=dev), torch.empty((32, 1), device=dev)

            def call(fn=fn, x=x, ws=ws, ids=ids, n=n, sc=sc, w=w):
                rc = fn(x.data_ptr(), None, ws.data_ptr(), ids.data_ptr(), n.data_ptr(), sc.data_ptr(), 32, T_HEAD, V, w, 1, 0, N.stream_ptr())
                if rc:
                    raise SystemExit(f"bench_beam_stream.py: v100_ctc_beam_search returned {rc}")
            call()
            torch.cuda.synchronize()
            outs[tag] = (ids.clone(), n.clone(), sc.clone())
            arms[f"headline_{tag}_W{w}"] = (call, 40)
        if "parent" in outs:
            checks[f"headline_W{w}_equals_parent"] = equal(outs["this_tree"], outs["parent"])
    if not all(checks.values()):
        raise SystemExit(f"bench_beam_stream.py: outputs differ at the timed shapes: {[k for k, v in checks.items() if not v]}")

    for fn, _ in arms.values():
        window(fn, 1)
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, (fn, iters) in arms.items():
            times[k].append(window(fn, iters))
    res = {k: dict(summary(v), calls_per_window=arms[k][1]) for k, v in times.items()}

    ratios = {}
    for w in WIDTHS:
        for kind in lms:
            for chunk in (4096, 256):
                ratios[f"long_chunk{chunk}_over_one_call_{kind}_W{w}"] = ratio(res, f"long_chunk{chunk}_{kind}_W{w}", f"one_call_{kind}_W{w}")
            ratios[f"one_call_us_per_frame_{kind}_W{w}"] = round(res[f"one_call_{kind}_W{w}"]["median_ms"] * 1e3 / T, 3)
        if "parent" in libs:
            ratios[f"headline_this_tree_over_parent_W{w}"] = ratio(res, f"headline_this_tree_W{w}", f"headline_parent_W{w}")
    for kind in lms:
        for nrec in (1, 4):
            r = ratio(res, f"long_{nrec}x90000_{kind}_W16", f"cut_and_batch_{nrec}x90000_{kind}_W16")
            r["long_us_per_frame"] = round(res[f"long_{nrec}x90000_{kind}_W16"]["median_ms"] * 1e3 / T_LONG, 3)
            ratios[f"long_over_cut_and_batch_{nrec}x90000_{kind}_W16"] = r

    out = {"tool": "tools/bench_beam_stream.py", "device": torch.cuda.get_device_name(0),
           "shapes": {"a_b": [32, T, V], "c": [[1, T_LONG, V], [4, T_LONG, V]], "d": [32, T_HEAD, V], "W": list(WIDTHS), "nbest": 1,
                      "stream_bytes_per_row_90000_W16": int(N.helper("v100_ctc_beam_stream_workspace_bytes", 1, T_LONG, V, 16))},
           "method": f"windows of back-to-back calls between device events, {args.rounds} alternating rounds, one warm-up call per arm; "
                     "whole calls with their allocations (the stream's zeroed workspace included)",
           "outputs_equal_at_timed_shapes": checks, "long_form_against_cut_and_batch": agreement, "arms": res, "ratios": ratios,
           "parent_library": bool(args.parent_lib),
           "not_measured": ["a profiler run", "a trained model", "real recordings"]}
    if "compiler_resource_report" in prior:
        out["compiler_resource_report"] = prior["compiler_resource_report"]
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
