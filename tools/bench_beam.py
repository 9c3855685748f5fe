#!/usr/bin/env python3
"""Time the CTC prefix beam search (decode.ctc_beam_search, csrc/beam.hip, K24) beside the host recursion it replaces and beside the
greedy decode, and record how far its scores are from the float64 oracle.

Shape: B = 32 utterances x 512 output frames (asr_en_base on 1024 input frames), V = 29, on two kinds of logits:
  "seeded"  standard_normal * 3 from the tests' generator (tests/_beam_ref.py, default_rng(1000 T + 10 V + W));
  "model"   AudioToTextCTC(64, 512, 29, 512), eval mode, seeded weights on seeded input [32, 1024, 64].
Arms, for W = 4, 16 and 64 with nbest = 1, in one process:
  (a) ctc_beam_search: the one launch (workspace and output allocation included: it is the call a user makes);
  (b) what a user does without it: .cpu(), then the oracle's plain (non-forking) recursion per utterance, on the host clock;
  (c) ctc_greedy_decode on the same logits: the floor.
Before anything is timed, (a) is compared with the oracle at the timed shape: where the forking oracle has ONE leaf (no near-tie at
the beam's edge anywhere) the ids of (a) must equal those of (b); where it has several, (a) must be one of them; more than
--leaves leaves: undecided, counted (at 512 frames most utterances have a near-tie at the beam's edge in some frame, so the count of
best transcripts equal to the plain host recursion's, and the worst score difference from it, are reported for all 32 as well).
(a) and (c) are timed as in tools/bench_edit_distance.py: windows of at least --window seconds of back-to-back calls between device
events, --rounds alternating rounds, median and spread (max - min) / median per arm.  The bar:
(b) / (a) - 1 > max(3 %, 3 x the larger spread).  The eval forward is timed in the same run.  score_rel_err_max is the worst
|device score - oracle score| / max(1, |oracle score|) over the tests' seeded cases (all shapes of tests/_beam_ref.py).
Not measured here: the kernel alone under a profiler (the figures are whole calls).
    python tools/bench_beam.py [--window 0.5] [--rounds 7] [--host-rounds 2] [--leaves 16] [--out profiles/beam_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _beam_ref import REL, SHAPES, accept, beam_search, beam_search_fork, seeded_case, seeded_logits  # noqa: E402
from voice100_amd.decode import ctc_beam_search, ctc_greedy_decode  # noqa: E402

B, T, V = 32, 512, 29
WIDTHS = (4, 16, 64)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                                     # ms per call


def iters_for(fn, seconds):
    per_call = max(window(fn, 3), 1e-4)
    return max(3, int(seconds * 1e3 / per_call) + 1)


def summary(times):
    med = statistics.median(times)
    return {"rounds_ms": [round(t, 5) for t in times], "median_ms": round(med, 5), "spread": round((max(times) - min(times)) / med, 4)}


def rows(ids, lens):
    ids, lens = ids.cpu().numpy(), lens.cpu().numpy()
    return [tuple(int(v) for v in ids[b, :lens[b]]) for b in range(ids.shape[0])]


def score_error_on_test_cases(dev):
    """The worst relative score difference from the float64 oracle over the tests' seeded cases (the best-matching leaf of each)."""
    worst, cases, undecided = 0.0, 0, 0
    for i, (t, v, w, scale, nbest, n) in enumerate(SHAPES):
        x, leaves = seeded_case(i)
        ids, lens, scores = (o.cpu().numpy() for o in ctc_beam_search(torch.from_numpy(x).to(dev), None, w, nbest))
        for b in range(n):
            if leaves[b] is None:
                undecided += 1
                continue
            hyps = [tuple(int(c) for c in ids[b, r, :lens[b, r]]) for r in range(nbest)]
            ok, err = accept(leaves[b], hyps, [float(s) for s in scores[b]])
            if not ok:
                raise SystemExit(f"bench_beam.py: the device result of test shape {SHAPES[i]}, case {b}, matches no leaf of the oracle")
            worst = max(worst, err)
            cases += 1
    return worst, cases, undecided


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--leaves", type=int, default=16, help="the forking oracle gives up beyond this many leaves (undecided)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")

    from voice100_amd.asr import AudioToTextCTC
    torch.manual_seed(0)
    model = AudioToTextCTC(64, 512, V, 512).to(dev).eval()
    audio = torch.randn(B, 1024, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    with torch.no_grad():
        model_logits = model(audio).float().contiguous()
    assert tuple(model_logits.shape) == (B, T, V), tuple(model_logits.shape)
    inputs = {("seeded", w): torch.from_numpy(seeded_logits(T, V, w, 3, B)).to(dev) for w in WIDTHS}
    inputs.update({("model", w): model_logits for w in WIDTHS})

    err, err_cases, err_undecided = score_error_on_test_cases(dev)

    # correctness at the timed shape, and what the beam changes against greedy
    agreement, host = {}, {}
    for (kind, w), x in inputs.items():
        ids, lens, scores = ctc_beam_search(x, None, w, 1)
        got, sc = rows(ids[:, 0], lens[:, 0]), scores[:, 0].cpu().numpy()
        greedy = rows(*ctc_greedy_decode(x))
        xc = x.cpu().numpy()
        single = several = undecided = 0
        plain = [beam_search(xc[b], w)[0] for b in range(B)]
        for b in range(B):
            leaves = beam_search_fork(xc[b], w, max_leaves=args.leaves)
            if leaves is None:
                undecided += 1
                continue
            ok, _ = accept(leaves, [got[b]], [float(sc[b])])
            if len(leaves) == 1:
                single += 1
                ok = ok and got[b] == plain[b][0]
            else:
                several += 1
            if not ok:
                raise SystemExit(f"bench_beam.py: {kind} logits, W = {w}, utterance {b}: the launch and the oracle disagree")
        agreement[f"{kind}_W{w}"] = {"one_leaf_ids_equal_host": single, "several_leaves_one_matches": several, "undecided": undecided,
                                     "best_ids_equal_host_plain_recursion": sum(g == p[0] for g, p in zip(got, plain)),
                                     "best_score_rel_diff_from_host_max": float(max(abs(float(s) - p[1]) / max(1.0, abs(p[1]))
                                                                                    for s, p in zip(sc, plain))),
                                     "transcripts_that_differ_from_greedy": sum(g != h for g, h in zip(greedy, got)),
                                     "mean_transcript_length": round(float(np.mean([len(h) for h in got])), 1)}
        t = []
        for _ in range(args.host_rounds):                                # arm (b): copy to the host, then the recursion per utterance
            t0 = time.perf_counter()
            xh = x.cpu().numpy()
            for b in range(B):
                beam_search(xh[b], w)
            t.append((time.perf_counter() - t0) * 1e3)
        host[f"{kind}_W{w}"] = dict(summary(t), calls_per_window=1, clock="host perf_counter, .cpu() copy included")

    arms = {}
    for (kind, w), x in inputs.items():
        arms[f"beam_{kind}_W{w}"] = lambda x=x, w=w: ctc_beam_search(x, None, w, 1)
    for kind in ("seeded", "model"):
        arms[f"greedy_{kind}"] = lambda x=inputs[(kind, 16)]: ctc_greedy_decode(x)
    with torch.no_grad():
        arms["forward"] = lambda: model(audio)
        for fn in arms.values():
            window(fn, 3)
        iters = {k: iters_for(fn, args.window) for k, fn in arms.items()}
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                times[k].append(window(fn, iters[k]))
    res = {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}
    res["forward"].update(model="AudioToTextCTC(64, 512, 29, 512), eval", frames=[B, 1024])
    noise = max(v["spread"] for k, v in res.items() if k != "forward")
    bar = max(0.03, 3 * noise)
    ratios = {}
    for kind in ("seeded", "model"):
        for w in WIDTHS:
            a = res[f"beam_{kind}_W{w}"]["median_ms"]
            ratios[f"{kind}_W{w}"] = {"launch_ms": a, "host_ms": host[f"{kind}_W{w}"]["median_ms"],
                                      "host_over_launch": round(host[f"{kind}_W{w}"]["median_ms"] / a, 1),
                                      "clears_the_bar": bool(host[f"{kind}_W{w}"]["median_ms"] / a - 1 > bar),
                                      "launch_over_greedy": round(a / res[f"greedy_{kind}"]["median_ms"], 1),
                                      "share_of_forward": round(a / res["forward"]["median_ms"], 4),
                                      "us_per_frame": round(a * 1e3 / T, 3)}

    out = {"tool": "tools/bench_beam.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "T": T, "V": V, "W": list(WIDTHS), "nbest": 1},
           "method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds; "
                     f"host arm: {args.host_rounds} calls on the host clock; forking oracle capped at {args.leaves} leaves",
           "score_rel_err_max": err, "score_rel_err_cases": err_cases, "score_rel_err_undecided": err_undecided,
           "fork_threshold_rel": REL, "fork_threshold_over_score_error": round(REL / err, 1) if err > 0 else None,
           "agreement_at_timed_shape": agreement, "arms": res, "host_arm": host, "largest_spread": noise, "bar": round(bar, 4),
           "summary": ratios, "not_measured": "the kernel alone under a profiler; figures are whole calls with their allocations"}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
