#!/usr/bin/env python3
"""Time the synthesis scores (metrics.dtw_score, csrc/dtw.hip, K27) beside the two ways to get the same numbers without it, then
SynthesisScore.update beside the TTSPipeline forward it follows in an evaluation loop.

Shape: B = 32 utterances of 25-dimensional mel-cepstra, c0 left out (skip=1); hypothesis lengths uniform in [600, 1000] frames; each
reference is its hypothesis under a smooth random time warp of up to +-15 % plus noise; F0 tracks with voiced and unvoiced stretches.
Arms, in one process:
  (a) dtw_score: one library call gives cost, path length and the four path sums of every pair;
  (b) stock ops, batched over B: torch.cdist in float64 on the device (from differences, one call per utterance: see stock_dtw),
      the recurrence one anti-diagonal at a time on the device
      (about ten torch ops per anti-diagonal), then the moves copied to the host and the backtrace and the sums there in numpy,
      vectorised over B (a backtrace on the device would be one group of launches per path cell; it was not timed);
  (c) what a user does today: .cpu(), then the tests' float64 oracle (tests/_dtw_ref.py) per utterance, on the host clock.
Before anything is timed the arms' outputs are compared at the timed shape: (b) against (c) to 1e-12, (a) against (c) within the
derived bound (Du + 4) 2^-24 on the cost and exactly on the path-dependent outputs of the decided rows (tests/test_gpu_dtw.py).
(a) and (b) are timed as in tools/bench_edit_distance.py: windows of at least --window seconds of back-to-back calls between device
events, --rounds alternating rounds, median and spread (max - min) / median per arm.  The bar: (b) / (a) - 1 > max(3 %, 3 x the
larger spread of one arm), in this run, against arm (b).
    python tools/bench_tts_score.py [--window 0.5] [--rounds 7] [--out profiles/tts_score_bench.json]
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
from _dtw_ref import path_sums, score_batch  # noqa: E402
from voice100_amd.metrics import SynthesisScore, dtw_score  # noqa: E402

B, D, SKIP, F0_FLOOR = 32, 25, 1, 30.0
DU = D - SKIP


def make_batch(seed=0):
    rng = np.random.default_rng(seed)
    n = rng.integers(600, 1001, B)
    n[0] = 1000
    m = np.clip(np.round(n * (1 + rng.uniform(-0.15, 0.15, B))), 1, None).astype(np.int64)
    m[0] = 1150
    Tx, Ty = int(n.max()), int(m.max())
    x, y = np.zeros((B, Tx, D), np.float32), np.zeros((B, Ty, D), np.float32)
    f0x, f0y = np.zeros((B, Tx), np.float32), np.zeros((B, Ty), np.float32)
    for b in range(B):
        t = np.arange(n[b])[:, None] / 9.0
        a = np.sin(t * rng.uniform(0.5, 2.0, D) + rng.random(D) * 6) + 0.3 * rng.standard_normal((n[b], D))
        f = np.where(np.sin(np.arange(n[b]) / 11.0 + rng.random() * 6) > 0.2, 0.0,
                     120 + 40 * np.sin(np.arange(n[b]) / 17.0) + 3 * rng.standard_normal(n[b]))
        u = np.linspace(0.0, 1.0, m[b])
        u = u + 0.15 * np.sin(2 * np.pi * (u * rng.uniform(0.5, 1.5) + rng.random())) * u * (1 - u) * 4        # the smooth warp
        w = np.clip(np.round(np.maximum.accumulate(u) * (n[b] - 1)), 0, n[b] - 1).astype(np.int64)
        x[b, :n[b]], y[b, :m[b]] = a, a[w] + 0.1 * rng.standard_normal((m[b], D))
        f0x[b, :n[b]] = f
        f0y[b, :m[b]] = np.where(rng.random(m[b]) < 0.05, 0.0, f[w] * (1 + 0.02 * rng.standard_normal(m[b])))
    return x, n.astype(np.int32), y, m.astype(np.int32), f0x, f0y


def stock_dtw(x64, y64, xl, yl, f0x, f0y):
    """The same quantities in stock ops: x64 / y64 [B, T, Du] float64 on the device, xl / yl [B] int64 there; f0x / f0y numpy.
    Returns (cost [B] float64 tensor, list of paths, list of path sums)."""
    dev = x64.device
    Bn, Tx, Ty = x64.shape[0], x64.shape[1], y64.shape[1]
    # from differences, as the definition asks (the default mode goes through |x|^2 + |y|^2 - 2 x.y at these sizes).  One call per
    # utterance: the single batched call in this mode returned zeros for rows 3 .. 31 at [32, 1000, 24] x [32, 1150, 24] on this stack
    d = torch.stack([torch.cdist(x64[b], y64[b], compute_mode="donot_use_mm_for_euclid_dist") for b in range(Bn)])
    C = torch.full((Bn, Tx + 1, Ty + 1), float("inf"), dtype=torch.float64, device=dev)  # shifted by one; row / column 0 absent
    C[:, 0, 0] = 0.0                                                                      # the virtual predecessor of (0,0)
    mv = torch.zeros((Bn, Tx, Ty), dtype=torch.uint8, device=dev)
    two = torch.tensor(2, dtype=torch.uint8, device=dev)
    for s in range(Tx + Ty - 1):
        i = torch.arange(max(0, s - Ty + 1), min(Tx, s + 1), device=dev)
        j = s - i
        diag, up, left = C[:, i, j], C[:, i, j + 1], C[:, i + 1, j]
        m2 = torch.minimum(diag, up)
        mv[:, i, j] = torch.where(left < m2, two, (up < diag).to(torch.uint8))
        C[:, i + 1, j + 1] = d[:, i, j] + torch.minimum(m2, left)
    bi = torch.arange(Bn, device=dev)
    cost = C[bi, xl, yl]
    moves, n, m = mv.cpu().numpy(), xl.cpu().numpy(), yl.cpu().numpy()                    # the backtrace on the host, over B at once
    i, j = n - 1, m - 1
    steps = [(i.copy(), j.copy())]
    live = (i > 0) | (j > 0)
    rows = np.arange(Bn)
    while live.any():
        k = np.where(i == 0, 2, np.where(j == 0, 1, moves[rows, i, j]))
        i = np.where(live & (k != 2), i - 1, i)
        j = np.where(live & (k != 1), j - 1, j)
        steps.append((i.copy(), j.copy()))
        live = (i > 0) | (j > 0)
    si, sj = np.stack([a for a, _ in steps]), np.stack([c for _, c in steps])            # [P_max, B], from the end
    paths, sums = [], []
    for b in range(Bn):
        first = int(np.argmax((si[:, b] == 0) & (sj[:, b] == 0))) + 1                    # cells until (0,0) is first reached
        p = list(zip(si[:first, b][::-1].tolist(), sj[:first, b][::-1].tolist()))
        paths.append(p)
        sums.append(path_sums(p, f0x[b], f0y[b], F0_FLOOR))
    return cost, paths, sums


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                                     # ms per call


def iters_for(fn, seconds):
    per_call = max(window(fn, 2), 1e-4)
    return max(2, int(seconds * 1e3 / per_call) + 1)


def summary(times):
    med = statistics.median(times)
    return {"rounds_ms": [round(t, 5) for t in times], "median_ms": round(med, 5), "spread": round((max(times) - min(times)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tts_score_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tts_score.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    data = make_batch()
    x, xl, y, yl, f0x, f0y = data
    xd, xld, yd, yld, f0xd, f0yd = (torch.from_numpy(a).to(dev) for a in data)
    x64, y64, xl64, yl64 = xd[:, :, SKIP:].double().contiguous(), yd[:, :, SKIP:].double().contiguous(), xld.long(), yld.long()

    def arm_a():
        return dtw_score(xd, xld, yd, yld, f0xd, f0yd, skip=SKIP, f0_floor=F0_FLOOR)

    def arm_b():
        return stock_dtw(x64, y64, xl64, yl64, f0x, f0y)

    def arm_c():
        c = [t.cpu().numpy() for t in (xd, xld, yd, yld, f0xd, f0yd)]
        return score_batch(*c, skip=SKIP, f0_floor=F0_FLOOR)

    sa = dtw_score(xd, xld, yd, yld, f0xd, f0yd, skip=SKIP, f0_floor=F0_FLOOR, return_path=True)
    cost_b, paths_b, sums_b = arm_b()
    sc = arm_c()
    bound = (DU + 4) * 2.0 ** -24
    decided = [r["margin"] > 2 * bound for r in sc]
    ca, pa = sa.cost.cpu().numpy(), sa.path.cpu().numpy()
    ia = [t.cpu().numpy() for t in (sa.path_len, sa.voiced, sa.vuv_errors)]
    fa = [t.cpu().numpy() for t in (sa.f0_sq_cents, sa.f0_sq_hz)]
    close = lambda u, v, tol: abs(u - v) <= tol * abs(v)  # noqa: E731
    equal = {
        "cost_a_vs_c_within_bound": all(close(ca[b], r["cost"], bound) for b, r in enumerate(sc)),
        "path_outputs_a_vs_c_on_decided_rows": all(
            ia[0][b] == r["path_len"] and ia[1][b] == r["voiced"] and ia[2][b] == r["vuv_errors"]
            and pa[b, :r["path_len"]].tolist() == [list(p) for p in r["path"]]
            and close(fa[0][b], r["f0_sq_cents"], 1e-9) and close(fa[1][b], r["f0_sq_hz"], 1e-9)
            for b, r in enumerate(sc) if decided[b]),
        "cost_b_vs_c": all(close(float(cost_b[b]), r["cost"], 1e-12) for b, r in enumerate(sc)),
        "path_b_vs_c": all(paths_b[b] == r["path"] for b, r in enumerate(sc)),
        "sums_b_vs_c": all(sums_b[b][:2] == (r["voiced"], r["vuv_errors"]) and close(sums_b[b][2], r["f0_sq_cents"], 1e-12)
                           and close(sums_b[b][3], r["f0_sq_hz"], 1e-12) for b, r in enumerate(sc)),
    }
    if not all(equal.values()):
        raise SystemExit(f"bench_tts_score.py: the arms disagree at the timed shape: {equal}")

    arms = {"dtw_score": arm_a, "stock_ops": arm_b}
    window(arm_a, 3)
    iters = {k: iters_for(fn, args.window) for k, fn in arms.items()}
    times = {k: [] for k in arms}
    host = []
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, iters[k]))
        t0 = time.perf_counter()
        arm_c()
        host.append((time.perf_counter() - t0) * 1e3)
    res = {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}
    res["host_reference"] = dict(summary(host), calls_per_window=1, clock="host perf_counter, .cpu() copies included")
    a, b, c = (res[k]["median_ms"] for k in ("dtw_score", "stock_ops", "host_reference"))
    noise = max(res["dtw_score"]["spread"], res["stock_ops"]["spread"])
    bar = max(0.03, 3 * noise)

    from voice100_amd.infer import TTSPipeline
    from voice100_amd.tts import AlignTextToAudioModel, TextToAlignTextModel
    from voice100_amd.vocoder import WORLDVocoder
    torch.manual_seed(0)
    chain = TTSPipeline(TextToAlignTextModel(vocab_size=29, hidden_size=512).to(dev).eval(),
                        AlignTextToAudioModel(vocab_size=29, hidden_size=512, use_mcep=True).to(dev).eval(),
                        WORLDVocoder(use_mcep=True).to(dev), synthesize=False)
    text, text_len = torch.randint(1, 29, (B, 100), device=dev), torch.full((B,), 100, dtype=torch.int64, device=dev)
    meter = SynthesisScore(chain.vocoder, F0_FLOOR)
    steps = {"synthesis_score_update": lambda: meter.update(f0xd, xd, xld, f0yd, yd, yld), "forward": lambda: chain(text, text_len)}
    with torch.no_grad():
        fwd_frames = int(chain(text, text_len)["frames"].sum())
        for k, fn in steps.items():
            window(fn, 3)
            n = iters_for(fn, args.window)
            res[k] = dict(summary([window(fn, n) for _ in range(args.rounds)]), calls_per_window=n)
    res["forward"].update(model="TTSPipeline(TextToAlignTextModel(29, 512), AlignTextToAudioModel(29, 512, use_mcep=True)), eval, "
                                "synthesis off, random weights", text=[B, 100], frames=fwd_frames)

    out = {"tool": "tools/bench_tts_score.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "D": D, "skip": SKIP, "Tx": int(x.shape[1]), "Ty": int(y.shape[1]), "hyp_frames": int(xl.sum()),
                     "ref_frames": int(yl.sum()), "cells": int((xl.astype(np.int64) * yl).sum()), "path_pairs": int(ia[0].sum()),
                     "voiced_pairs": int(ia[1].sum()), "vuv_errors": int(ia[2].sum()), "undecided_rows": int(B - sum(decided))},
           "method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds; "
                     "host_reference: one call per round on the host clock",
           "stock_ops_backtrace": "on the host, numpy over B at once, inside the timed region (the device variant was not timed)",
           "outputs_equal_at_timed_shape": equal, "arms": res,
           "stock_ops_over_dtw_score": round(b / a, 2), "host_reference_over_dtw_score": round(c / a, 1),
           "largest_spread_of_a_or_b": noise, "bar": round(bar, 4), "dtw_score_clears_the_bar": bool(b / a - 1 > bar),
           "synthesis_score_update_share_of_forward": round(res["synthesis_score_update"]["median_ms"] / res["forward"]["median_ms"], 4)}
    text_out = json.dumps(out, indent=1)
    print(text_out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text_out + "\n")


if __name__ == "__main__":
    main()
