#!/usr/bin/env python3
"""Time the fused CTC prefix beam search (decode.ctc_beam_search(lm=...), csrc/beam.hip, K25) beside the same launch without an LM and
beside the host recursion it replaces, record how far its scores are from the float64 oracle, and check on a synthetic task that the
LM lowers the error rate.

Shape: K24's, B = 32 utterances x 512 output frames, V = 29, logits standard_normal * 3 from the tests' generator
(tests/_beam_ref.py), W = 4, 16 and 64 with nbest = 1.  LMs: NGramLM.fit of order 3 and of order 5 on 2000 seeded strings from a
random first-order chain over the 28 labels; lm_weight 0.5, length_bonus 0.5, use_eos.  Arms, in one process:
  (a) the fused launch, per LM order (workspace and output allocation included: it is the call a user makes);
  (b) the launch without an LM on the same logits; (a) / (b) is what the LM costs per frame;
  (c) what a user does without (a): .cpu(), then the oracle's plain (non-forking) float64 recursion with the LM per utterance, on the
      host clock.  The host reads the compiled automaton (one table row per new prefix), the cheapest form a host can use.
(a) and (b) are timed as in tools/bench_beam.py: windows of at least --window seconds of back-to-back calls between device events,
--rounds alternating rounds, median and spread (max - min) / median per arm.  The bar: (c) / (a) - 1 > max(3 %, 3 x the larger spread);
(a) / (b) has no bar.  Before anything is timed, the best hypothesis of (a) at the timed shape is compared with the plain host
recursion (equal ids counted, worst score difference), and score_rel_err_max is taken over every cell of the GPU parity test
(tests/_beam_lm_ref.py: shapes x settings x {random automaton, fit LM}) against the forking oracle.

The learnable task: reference strings of 40 labels from the same chain (a draw disjoint from the LM's training strings); logits are
the one-hot reference (each label one frame, a blank frame after it) at 20 nats plus standard_normal * --noise; CER through ErrorRate
for the greedy decode, the beam without an LM and the beam with the order-3 LM over a small grid of (lm_weight, length_bonus), W = 16.
The figures are a property of this task, not a pinned bar.
Not measured here: the kernel alone under a profiler (the figures are whole calls).
    python tools/bench_beam_lm.py [--window 0.3] [--rounds 5] [--host-rounds 1] [--noise 6.5] [--out profiles/beam_lm_bench.json]
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
import _beam_lm_ref as R  # noqa: E402
from _beam_ref import REL, seeded_logits  # noqa: E402
from voice100_amd.decode import ctc_beam_search, ctc_greedy_decode  # noqa: E402
from voice100_amd.infer import ErrorRate  # noqa: E402
from voice100_amd.lm import NGramLM  # noqa: E402

B, T, V = 32, 512, 29
WIDTHS = (4, 16, 64)
ORDERS = (3, 5)
ALPHA, BETA = 0.5, 0.5


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


def chain(rng):
    """A random first-order source over the 28 labels: (initial distribution, transition matrix), a few likely successors each."""
    return rng.dirichlet(np.full(V - 1, 0.5)), rng.dirichlet(np.full(V - 1, 0.08), size=V - 1)


def draw(rng, source, count, length):
    init, trans = source
    out = []
    for _ in range(count):
        s = [int(rng.choice(V - 1, p=init))]
        for _ in range(length - 1):
            s.append(int(rng.choice(V - 1, p=trans[s[-1]])))
        out.append([c + 1 for c in s])                                   # label ids 1 .. 28; 0 is the blank
    return out


def score_error_on_test_cells(dev):
    worst, cases, undecided = 0.0, 0, 0
    for i, (t, v, w) in enumerate(R.GPU_SHAPES):
        nbest = R.shape_params(t, v, w)[1]
        for j, (alpha, beta, _) in enumerate(R.SETTINGS):
            for kind in ("automaton", "fit"):
                x, lm, leaves = R.seeded_case(i, j, kind)
                lm = (NGramLM.from_tables(*lm[:3], start=lm[3]) if kind == "automaton" else lm.compile())
                lm = NGramLM.from_tables(lm.logp, lm.next, lm.final, lm.start).to(dev)
                out = [o.cpu().numpy() for o in ctc_beam_search(torch.from_numpy(x).to(dev), None, w, nbest, lm=lm, lm_weight=alpha,
                                                                length_bonus=beta)]
                for b in range(x.shape[0]):
                    if leaves[b] is None:
                        undecided += 1
                        continue
                    hyps = [tuple(int(c) for c in out[0][b, r, :out[1][b, r]]) for r in range(nbest)]
                    ok, err = R.accept(leaves[b], hyps, *([float(s) for s in out[k][b]] for k in (2, 3, 4)))
                    if not ok:
                        raise SystemExit(f"bench_beam_lm.py: test cell {(t, v, w)}, {(alpha, beta)}, {kind}, case {b} matches no leaf")
                    worst = max(worst, err)
                    cases += 1
    return worst, cases, undecided


def learnable_task(dev, rng, source, lm, noise, count=64, length=40, W=16):
    refs = draw(rng, source, count, length)
    frames = 2 * length
    x = rng.standard_normal((count, frames, V)) * noise
    for b, ref in enumerate(refs):
        x[b, np.arange(0, frames, 2), ref] += 20.0
        x[b, 1::2, 0] += 20.0
    x = torch.from_numpy(x.astype(np.float32)).to(dev)
    ref = torch.tensor(refs, dtype=torch.int64, device=dev)
    ref_len = torch.full((count,), length, dtype=torch.int32, device=dev)

    def cer(ids, lens):
        meter = ErrorRate(sep=None)
        meter.update(ids.contiguous(), lens.contiguous(), ref, ref_len)
        return round(meter.compute()["cer"], 5)

    out = {"utterances": count, "labels_each": length, "frames_each": frames, "noise": noise, "W": W,
           "cer_greedy": cer(*ctc_greedy_decode(x))}
    ids, lens, _ = ctc_beam_search(x, None, W, 1)
    out["cer_beam_no_lm"] = cer(ids[:, 0], lens[:, 0])
    grid = {}
    for alpha in (0.5, 1.0):
        for beta in (0.0, 1.0, 2.0):
            ids, lens = ctc_beam_search(x, None, W, 1, lm=lm, lm_weight=alpha, length_bonus=beta)[:2]
            grid[f"lm_weight_{alpha}_length_bonus_{beta}"] = cer(ids[:, 0], lens[:, 0])
    out["cer_beam_lm_order3"] = grid
    out["cer_beam_lm_order3_best"] = min(grid.values())
    out["lm_beam_below_both"] = bool(out["cer_beam_lm_order3_best"] < min(out["cer_greedy"], out["cer_beam_no_lm"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.3, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=1)
    ap.add_argument("--noise", type=float, default=6.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_lm_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam_lm.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")

    rng = np.random.default_rng(2025)
    source = chain(rng)
    train = draw(rng, source, 2000, 40)
    lms, looks, info = {}, {}, {}
    for n in ORDERS:
        t0 = time.perf_counter()
        host = NGramLM.fit(train, V, n).compile()
        looks[n] = R.AutomatonLM(host.logp.numpy(), host.next.numpy(), host.final.numpy(), host.start)
        info[f"order{n}"] = {"states": host.num_states, "table_bytes": host.num_states * V * 8,
                             "ngrams": [len(t) for t in host.ngrams], "fit_and_compile_s": round(time.perf_counter() - t0, 2)}
        lms[n] = NGramLM.from_tables(host.logp, host.next, host.final, host.start).to(dev)

    err, err_cases, err_undecided = score_error_on_test_cells(dev)
    task = learnable_task(dev, rng, source, lms[3], args.noise)

    inputs = {w: torch.from_numpy(seeded_logits(T, V, w, 3, B)).to(dev) for w in WIDTHS}
    agreement, host_arm = {}, {}
    for n in ORDERS:
        for w, x in inputs.items():
            xc = x.cpu().numpy()
            ids, lens, scores, ctc, lmsc = (o.cpu().numpy() for o in ctc_beam_search(x, None, w, 1, lm=lms[n], lm_weight=ALPHA,
                                                                                      length_bonus=BETA))
            plain_ids, plain_lens, _ = (o.cpu().numpy() for o in ctc_beam_search(x, None, w, 1))
            t, best = [], None
            for _ in range(args.host_rounds):                            # arm (c)
                t0 = time.perf_counter()
                xh = x.cpu().numpy()
                best = [R.beam_search(xh[b], w, looks[n], ALPHA, BETA)[0] for b in range(B)]
                t.append((time.perf_counter() - t0) * 1e3)
            host_arm[f"order{n}_W{w}"] = dict(summary(t), clock="host perf_counter, .cpu() copy included")
            got = [tuple(int(v) for v in ids[b, 0, :lens[b, 0]]) for b in range(B)]
            agreement[f"order{n}_W{w}"] = {
                "best_ids_equal_host_plain_recursion": sum(g == h[0] for g, h in zip(got, best)),
                "best_score_rel_diff_from_host_max": float(max(abs(float(scores[b, 0]) - best[b][1]) / max(1.0, abs(best[b][1]))
                                                               for b in range(B))),
                "transcripts_that_differ_from_the_beam_without_lm":
                    sum(got[b] != tuple(int(v) for v in plain_ids[b, 0, :plain_lens[b, 0]]) for b in range(B)),
                "mean_transcript_length": round(float(np.mean([len(g) for g in got])), 1)}
            assert xc.shape == (B, T, V)

    arms = {}
    for w, x in inputs.items():
        arms[f"plain_W{w}"] = lambda x=x, w=w: ctc_beam_search(x, None, w, 1)
        for n in ORDERS:
            arms[f"lm_order{n}_W{w}"] = lambda x=x, w=w, n=n: ctc_beam_search(x, None, w, 1, lm=lms[n], lm_weight=ALPHA, length_bonus=BETA)
    for fn in arms.values():
        window(fn, 3)
    iters = {k: iters_for(fn, args.window) for k, fn in arms.items()}
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, iters[k]))
    res = {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}
    noise = max(v["spread"] for v in res.values())
    bar = max(0.03, 3 * noise)
    ratios = {}
    for n in ORDERS:
        for w in WIDTHS:
            a, b = res[f"lm_order{n}_W{w}"]["median_ms"], res[f"plain_W{w}"]["median_ms"]
            c = host_arm[f"order{n}_W{w}"]["median_ms"]
            ratios[f"order{n}_W{w}"] = {"fused_ms": a, "plain_ms": b, "host_ms": c, "fused_over_plain": round(a / b, 3),
                                        "host_over_fused": round(c / a, 1), "clears_the_bar": bool(c / a - 1 > bar),
                                        "us_per_frame": round(a * 1e3 / T, 3), "lm_us_per_frame": round((a - b) * 1e3 / T, 3)}

    out = {"tool": "tools/bench_beam_lm.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "T": T, "V": V, "W": list(WIDTHS), "nbest": 1, "lm_weight": ALPHA, "length_bonus": BETA, "use_eos": True},
           "method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds; "
                     f"host arm: {args.host_rounds} call(s) on the host clock",
           "lm": info, "score_rel_err_max": err, "score_rel_err_cases": err_cases, "score_rel_err_undecided": err_undecided,
           "fork_threshold_rel": REL, "fork_threshold_over_score_error": round(REL / err, 1) if err > 0 else None,
           "agreement_at_timed_shape": agreement, "arms": res, "host_arm": host_arm, "largest_spread": noise, "bar": round(bar, 4),
           "summary": ratios, "learnable_task": task,
           "not_measured": "the kernel alone under a profiler; figures are whole calls with their allocations"}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
