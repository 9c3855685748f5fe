#!/usr/bin/env python3
"""Time the forced-alignment step (decode.ctc_align, csrc/align.hip, K20) beside the path the tree offered before it, then the
whole AlignPipeline.

Shape: B = 32 utterances of T = 800 frames (16 s of speech at 50 frames/s), Lmax = 200 labels, V = 29, ragged lengths (frames
uniform in [T / 2, T], labels in [Lmax / 4, Lmax], one full row each), random log-softmax data.  Arms, in one process:
  (a) ctc_align: one library launch (plus the allocation of its outputs and workspace);
  (b) the composition: decode.ctc_best_path (the older kernel, its label gather included) and the stock ops that derive the
      durations from the path (a mask of the valid frames and a scatter_add).
Before anything is timed the two arms' outputs are compared for equality at the timed shape (score bit for bit).  Then, after a
warm-up, --rounds rounds alternate the arms; each timing is one window of at least --window seconds of back-to-back calls
between two device events, ended by a device synchronise.  Reported per arm: every round, the median and the spread
(max - min) / median -- the spread of repeating ONE arm is the yardstick a difference between the arms is read against.
Last, AlignPipeline (forward, log_softmax, ctc_align) with AudioAlignCTC at its defaults (audio 64, hidden 128, 2 layers) on
B x 2T input frames, timed the same way, so the kernel's share of the step can be read.
    python tools/bench_align.py [--window 0.5] [--rounds 7] [--out profiles/align_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice100_amd.decode import ctc_align, ctc_best_path  # noqa: E402

B, T, LMAX, V = 32, 800, 200, 29


def composition(lp, labels, in_len, lab_len):
    """Today's path without ctc_align: the older kernel, then labels (inside ctc_best_path) and durations by stock ops."""
    score, path, best = ctc_best_path(lp, labels, in_len, lab_len)
    valid = (torch.arange(lp.shape[1], device=lp.device)[None, :] < in_len[:, None]).to(torch.int32)
    align = torch.zeros((lp.shape[0], 2 * labels.shape[1] + 1), dtype=torch.int32, device=lp.device)
    align.scatter_add_(1, path.long(), valid)
    return score, path, best, align


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                                 # ms per call


def iters_for(fn, seconds):
    per_call = max(window(fn, 10), 1e-4)
    return max(10, int(seconds * 1e3 / per_call) + 1)


def summary(times):
    med = statistics.median(times)
    return {"rounds_ms": [round(t, 5) for t in times], "median_ms": round(med, 5), "spread": round((max(times) - min(times)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "align_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_align.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lp = torch.log_softmax(torch.randn(B, T, V, generator=gen), -1).to(dev)
    labels = torch.randint(1, V, (B, LMAX), generator=gen).to(dev)
    in_len = torch.randint(T // 2, T + 1, (B,), generator=gen)
    lab_len = torch.randint(LMAX // 4, LMAX + 1, (B,), generator=gen)
    in_len[0], lab_len[0] = T, LMAX
    lab_len = torch.minimum(lab_len, in_len - 1)
    in_len, lab_len = in_len.to(dev, torch.int32), lab_len.to(dev, torch.int32)

    new = ctc_align(lp, labels, in_len, lab_len)
    old = composition(lp, labels, in_len, lab_len)
    equal = {name: bool(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b))
             for name, a, b in zip(("score", "path", "best_labels", "align"), new, old)}
    if not all(equal.values()):
        raise SystemExit(f"bench_align.py: the arms disagree at the timed shape: {equal}")

    arms = {"ctc_align": lambda: ctc_align(lp, labels, in_len, lab_len), "composition": lambda: composition(lp, labels, in_len, lab_len)}
    for fn in arms.values():
        window(fn, 20)
    iters = {k: iters_for(fn, args.window) for k, fn in arms.items()}
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, iters[k]))
    res = {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}
    ratio = res["composition"]["median_ms"] / res["ctc_align"]["median_ms"]
    noise = max(res["ctc_align"]["spread"], res["composition"]["spread"])

    from voice100_amd.align import AudioAlignCTC
    from voice100_amd.infer import AlignPipeline
    torch.manual_seed(0)
    model = AudioAlignCTC(64, V, 128, 2, 1e-3).to(dev).eval()
    audio = torch.randn(B, 2 * T, 64, device=dev)
    audio_len = torch.clamp(2 * in_len.long(), max=2 * T)
    pipe = AlignPipeline(model)
    run_pipe = lambda: pipe(audio, audio_len, labels, lab_len)  # noqa: E731
    window(run_pipe, 5)
    n_pipe = iters_for(run_pipe, args.window)
    pipe_times = [window(run_pipe, n_pipe) for _ in range(args.rounds)]
    res["align_pipeline"] = dict(summary(pipe_times), calls_per_window=n_pipe, model="AudioAlignCTC(64, 29, 128, 2)", audio_frames=2 * T)

    out = {"tool": "tools/bench_align.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "T": T, "Lmax": LMAX, "V": V, "frames": int(in_len.sum()), "labels": int(lab_len.sum())},
           "method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds",
           "outputs_equal_at_timed_shape": equal, "arms": res,
           "composition_over_ctc_align": round(ratio, 3), "largest_spread_of_one_arm": noise,
           "ctc_align_not_slower_beyond_spread": bool(res["ctc_align"]["median_ms"] <= res["composition"]["median_ms"] * (1 + noise)),
           "ctc_align_share_of_pipeline": round(res["ctc_align"]["median_ms"] / res["align_pipeline"]["median_ms"], 4)}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
