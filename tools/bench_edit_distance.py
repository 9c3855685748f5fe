#!/usr/bin/env python3
"""Time transcript scoring (decode.edit_distance_both, csrc/edit_distance.hip, K23) beside the two ways to get the same numbers
without it, then ErrorRate.update beside the forward pass it follows in a validation step.

Shape: B = 32 utterances; reference lengths uniform in [150, 300] ids over [1, 29) with id 1 (the space) about every sixth
position; hypotheses = the references with about 10 % random edits, then cut or continued with more text of the same kind to
lengths uniform in [256, 512] (a decoder that ran on past the end of the text: the body of each pair aligns as a 10 % error model
would, the tail is a run of insertions); one full row each.  Arms, in one process:
  (a) edit_distance_both: one library launch gives the character and the word level;
  (b) stock ops on the device, batched over B: per hypothesis row t = min(prev + 1, prev_shifted + neq), d = cummin(t - j) + j,
      one group of torch ops per row, once per level.  The word ids of (b) come from a HOST pre-pass kept out of the timed region;
  (c) what a user does today: .cpu(), then the tests' host reference (tests/_edit_ref.py) per utterance, timed on the host clock.
Before anything is timed the three arms' outputs are compared for equality at the timed shape.  (a) and (b) are timed as in
tools/bench_align.py: windows of at least --window seconds of back-to-back calls between device events, --rounds alternating
rounds, median and spread (max - min) / median per arm.  The bar: (b) / (a) - 1 > max(3 %, 3 x the larger spread of one arm).
    python tools/bench_edit_distance.py [--window 0.5] [--rounds 7] [--out profiles/edit_distance_bench.json]
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
from _edit_ref import score_rows, split_words, word_ids  # noqa: E402
from voice100_amd.decode import edit_distance_both  # noqa: E402

B, V, SEP = 32, 29, 1


def make_batch(seed=0):
    rng = np.random.default_rng(seed)
    text = lambda n: np.where(rng.random(n) < 1 / 6, SEP, rng.integers(2, V, n)).tolist()  # noqa: E731
    hyp_target = rng.integers(256, 513, B)
    ref_target = rng.integers(150, 301, B)
    hyp_target[0], ref_target[0] = 512, 300
    hyps, refs = [], []
    for b in range(B):
        ref = text(int(ref_target[b]))
        hyp = []
        for x in ref:                                                    # about 10 % edits
            u = rng.random()
            if u < 0.033:
                continue
            hyp.append(int(rng.integers(1, V)) if u < 0.066 else x)
            if u > 0.967:
                hyp.append(int(rng.integers(1, V)))
        hyp = (hyp + text(512))[:int(hyp_target[b])]                     # the decoder ran on: insertions at the end
        hyps.append(hyp)
        refs.append(ref)
    pad = lambda rows, w: np.array([r + [0] * (w - len(r)) for r in rows], np.int64)  # noqa: E731
    return (pad(hyps, 512), np.array([len(h) for h in hyps], np.int32), pad(refs, 300), np.array([len(r) for r in refs], np.int32))


def stock_levenshtein(h, hn, r, rn):
    """Batched row recursion in stock ops: h [B, n] / r [B, m] int64 token ids, hn / rn [B] int64 -> dist [B] int64."""
    m = r.shape[1]
    j = torch.arange(m + 1, device=h.device)
    d = j.expand(h.shape[0], m + 1).contiguous()
    col = rn[:, None]
    res = d.gather(1, col)[:, 0]                                         # the empty hypothesis
    t = torch.empty_like(d)
    for i in range(1, h.shape[1] + 1):
        t[:, 0] = i
        torch.minimum(d[:, 1:] + 1, d[:, :-1] + (r != h[:, i - 1:i]), out=t[:, 1:])
        d = torch.cummin(t - j, dim=1).values + j
        res = torch.where(hn == i, d.gather(1, col)[:, 0], res)
    return res


def host_word_ids(h, hl, r, rl):
    """Host pre-pass of arm (b): padded word-id batches of both sides."""
    hw, rw = [], []
    for b in range(h.shape[0]):
        a, c = word_ids(split_words(h[b, :hl[b]], SEP), split_words(r[b, :rl[b]], SEP))
        hw.append(a)
        rw.append(c)
    pad = lambda rows, fill: np.array([x + [fill] * (max(map(len, rows)) - len(x)) for x in rows], np.int64)  # noqa: E731
    return pad(hw, -1), np.array([len(x) for x in hw]), pad(rw, -2), np.array([len(x) for x in rw])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edit_distance_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_edit_distance.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    h, hl, r, rl = make_batch()
    hd, hld, rd, rld = (torch.from_numpy(x).to(dev) for x in (h, hl, r, rl))
    wh, whn, wr, wrn = (torch.from_numpy(x).to(dev) for x in host_word_ids(h, hl, r, rl))
    hl64, rl64 = hld.long(), rld.long()

    def arm_a():
        return edit_distance_both(hd, hld, rd, rld, SEP)

    def arm_b():
        return stock_levenshtein(hd, hl64, rd, rl64), stock_levenshtein(wh, whn, wr, wrn)

    def arm_c():
        hc, hlc, rc, rlc = hd.cpu().numpy(), hld.cpu().numpy(), rd.cpu().numpy(), rld.cpu().numpy()
        return score_rows(hc, hlc, rc, rlc), score_rows(hc, hlc, rc, rlc, SEP)

    dist, hyp_n, ref_n = arm_a()
    sb = arm_b()
    sc = arm_c()
    equal = {"chars_a_vs_c": [t[0].tolist() for t in (dist, hyp_n, ref_n)] == sc[0],
             "words_a_vs_c": [t[1].tolist() for t in (dist, hyp_n, ref_n)] == sc[1],
             "chars_b_vs_c": sb[0].tolist() == sc[0][0], "words_b_vs_c": sb[1].tolist() == sc[1][0]}
    if not all(equal.values()):
        raise SystemExit(f"bench_edit_distance.py: the arms disagree at the timed shape: {equal}")

    arms = {"edit_distance_both": arm_a, "stock_ops": arm_b}
    for fn in arms.values():
        window(fn, 3)
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
    a, b, c = (res[k]["median_ms"] for k in ("edit_distance_both", "stock_ops", "host_reference"))
    noise = max(res["edit_distance_both"]["spread"], res["stock_ops"]["spread"])
    bar = max(0.03, 3 * noise)

    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.infer import ErrorRate
    torch.manual_seed(0)
    model = AudioToTextCTC(64, 512, V, 512).to(dev).eval()
    audio = torch.randn(B, 1024, 64, device=dev)
    meter = ErrorRate(SEP)
    steps = {"error_rate_update": lambda: meter.update(hd, hld, rd, rld), "forward": lambda: model(audio)}
    with torch.no_grad():
        for k, fn in steps.items():
            window(fn, 5)
            n = iters_for(fn, args.window)
            res[k] = dict(summary([window(fn, n) for _ in range(args.rounds)]), calls_per_window=n)
    res["forward"].update(model="AudioToTextCTC(64, 512, 29, 512), eval", frames=[B, 1024])

    out = {"tool": "tools/bench_edit_distance.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "Th": 512, "Tr": 300, "hyp_ids": int(hl.sum()), "ref_ids": int(rl.sum()), "hyp_words": int(hyp_n[1].sum()),
                     "ref_words": int(ref_n[1].sum()), "char_errors": int(dist[0].sum()), "word_errors": int(dist[1].sum())},
           "method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds; "
                     "host_reference: one call per round on the host clock",
           "stock_ops_word_ids": "host pre-pass, outside the timed region",
           "outputs_equal_at_timed_shape": equal, "arms": res,
           "stock_ops_over_edit_distance": round(b / a, 2), "host_reference_over_edit_distance": round(c / a, 1),
           "largest_spread_of_a_or_b": noise, "bar": round(bar, 4), "edit_distance_clears_the_bar": bool(b / a - 1 > bar),
           "error_rate_update_share_of_forward": round(res["error_rate_update"]["median_ms"] / res["forward"]["median_ms"], 4)}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
