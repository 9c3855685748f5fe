#!/usr/bin/env python
"""K26, decode.ctc_segment: its error against the float64 oracle over the tests' parity cases, and its time at K24's shape
(B = 32 x 512 frames, V = 29) against the alternatives.  Writes profiles/ctc_segment_bench.json.

Errors: the largest |log_prob| error (relative), |duration| and |log_confidence| errors (absolute) over the parity cases of
tests/_ctc_segment_ref.py (the base grid x V in {2, 29, 71, 128} x scales {0.1, 3, 10}, the state-per-thread seams, and the planted
alignments, whose frame probabilities lie within 1e-7 of 1 and whose log_prob of ~1e-5 is judged against max(1, |log_prob|)).  The
tests' tolerances are these maxima x 8 rounded up to one digit, and a boundary counts as decided when its oracle margin exceeds
max(8 x the duration error, 1e-5).

Time: logits peaked on a seeded frame sequence (a label holds 1-3 frames, 0-4 blanks between labels: ~100 labels in 512 frames)
plus standard_normal noise; the hypotheses are the greedy decode.  Arms, whole calls with their allocations:
  (a) decode.ctc_segment;
  (b) the same quantities from a batched log-domain forward-backward in stock torch ops on the device (float64), checked equal to
      (a) on the decided boundaries;
  (c) .cpu() plus the float64 numpy oracle per utterance, on the host clock;
  (d) torch.log_softmax + decode.ctc_align, the hard-alignment neighbour (a yardstick, not a bar);
  (e) the eval forward of AudioToTextCTC(64, 512, 29, 512);
and ASRPipeline.segments against ASRPipeline.__call__, greedy and with beam_size = 16.
Windows of >= --window seconds of back-to-back calls between device events, --rounds alternating rounds, median and spread
(max - min) / median per arm.  The bar: slower / (a) - 1 > max(3 %, 3 x the larger spread).  --errors-only skips the timing."""
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
import _ctc_segment_ref as R  # noqa: E402
from voice100_amd.decode import ctc_align, ctc_greedy_decode, ctc_segment  # noqa: E402

B, T, V = 32, 512, 29
NEG = float("-inf")


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


def to_numpy(seg):
    return {k: v.cpu().numpy() for k, v in seg._asdict().items() if v is not None}


def errors_on_parity_cases(dev):
    worst = {"log_prob_rel": 0.0, "duration_abs": 0.0, "log_confidence_abs": 0.0}
    per_case, margins = [], []
    cases = [(T_, L_, V_) + R.parity_case(T_, L_, V_) for T_, L_, V_ in R.PARITY]
    for L_, V_ in R.PLANTED:                                             # the planted alignments: probabilities within 1e-7 of 1
        x, labels = R.planted_case(L_, V_)[:2]
        cases.append((x.shape[1], L_, V_, x, labels))
    for T_, L_, V_, x, labels in cases:
        ref = R.segment_batch(x, None, labels, None)
        got = to_numpy(ctc_segment(torch.from_numpy(x).to(dev), None, torch.from_numpy(labels).to(dev), None))
        c = R.compare(got, ref, 0.0)
        per_case.append({"T": T_, "L": L_, "V": V_, "feasible_rows": int(ref["feasible"].sum()),
                         **{k: c[k] for k in worst}})
        for k in worst:
            worst[k] = max(worst[k], c[k])
        margins.append((got, ref))
    margin = max(8 * worst["duration_abs"], 1e-5)
    tally = {"boundaries": 0, "undecided": 0, "wrong": 0}
    for got, ref in margins:
        c = R.compare(got, ref, margin)
        for k in tally:
            tally[k] += c[k]
    return worst, margin, tally, per_case


def peaked_logits(seed=0, peak=6.0):
    """[B, T, V] fp32: a seeded frame sequence (labels of 1-3 frames, 0-4 blanks between them: ~100 labels in 512 frames) with `peak`
    nats on its class, plus standard_normal noise."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, T, V)).astype(np.float32)
    for b in range(B):
        frames = np.zeros(T, np.int64)                                   # blank where no label is planted
        t = int(rng.integers(0, 5))
        while t < T:
            n = int(rng.integers(1, 4))
            frames[t:t + n] = int(rng.integers(1, V))
            t += n + int(rng.integers(0, 5))
        x[b, np.arange(T), frames] += peak
    return x


def shift(a, k, fill):
    out = torch.full_like(a, fill)
    if k > 0:
        out[:, k:] = a[:, :-k]
    else:
        out[:, :k] = a[:, -k:]
    return out


def stock_segment(logits, labels, label_lengths, blank=0, sep=1):
    """Arm (b): decode.ctc_segment's quantities in stock torch ops on the device, float64, log domain, every row T frames."""
    dev = logits.device
    lp = torch.log_softmax(logits.double(), -1)
    Bn, Tn, _ = lp.shape
    L = labels.shape[1]
    S = 2 * L + 1
    ll = label_lengths.long()
    z = torch.full((Bn, S), blank, dtype=torch.long, device=dev)
    z[:, 1::2] = labels
    valid = torch.arange(S, device=dev)[None] < (2 * ll + 1)[:, None]
    em = lp.gather(2, z[:, None, :].expand(Bn, Tn, S)).masked_fill(~valid[:, None, :], NEG)
    skip = torch.zeros((Bn, S), dtype=torch.bool, device=dev)
    skip[:, 3::2] = z[:, 3::2] != z[:, 1:-2:2]
    skip_out = shift(skip, -2, False)
    alpha = torch.full((Bn, Tn, S), NEG, dtype=torch.float64, device=dev)
    enter = torch.full_like(alpha, NEG)
    alpha[:, 0, :2] = em[:, 0, :2]
    enter[:, 0, :2] = 0.0
    for t in range(1, Tn):
        a = alpha[:, t - 1]
        enter[:, t] = torch.logaddexp(shift(a, 1, NEG), shift(a, 2, NEG).masked_fill(~skip, NEG))
        alpha[:, t] = em[:, t] + torch.logaddexp(a, enter[:, t])
    ends = torch.stack((2 * ll, (2 * ll - 1).clamp_min(0)), 1)
    fin = alpha[:, -1].gather(1, ends)
    logp = torch.where(ll > 0, torch.logaddexp(fin[:, 0], fin[:, 1]), fin[:, 0])
    beta = torch.full_like(alpha, NEG)
    leave = torch.full_like(alpha, NEG)
    last_states = torch.zeros((Bn, S), dtype=torch.bool, device=dev).scatter_(1, ends, True)
    beta[:, -1] = torch.where(last_states, 0.0, NEG)
    leave[:, -1] = beta[:, -1]
    for t in range(Tn - 2, -1, -1):
        bt = em[:, t + 1] + beta[:, t + 1]
        leave[:, t] = torch.logaddexp(shift(bt, -1, NEG), shift(bt, -2, NEG).masked_fill(~skip_out, NEG))
        beta[:, t] = torch.logaddexp(bt, leave[:, t])
    norm = logp[:, None, None]
    lab = slice(1, None, 2)
    gamma = torch.exp(alpha[:, :, lab] + beta[:, :, lab] - norm).nan_to_num(0.0)
    onset = torch.exp(enter[:, :, lab] + em[:, :, lab] + beta[:, :, lab] - norm).nan_to_num(0.0)
    last = torch.exp(alpha[:, :, lab] + leave[:, :, lab] - norm).nan_to_num(0.0)
    inside = torch.arange(L, device=dev)[None] < ll[:, None]
    dur = gamma.sum(1) * inside
    numer = (gamma * em[:, :, lab].masked_fill(gamma <= 0, 0.0)).sum(1) * inside
    start = ((onset.cumsum(1) >= 0.5).int().argmax(1) * inside).int()
    end = (((last.cumsum(1) >= 0.5).int().argmax(1) + 1) * inside).int()
    log_conf = torch.where(inside, numer / dur, torch.zeros_like(dur))
    is_lab = (labels != sep) & inside
    first = is_lab & ~shift(is_lab, 1, False)
    final = is_lab & ~shift(is_lab, -1, False)
    wid = (first.long().cumsum(1) - 1).clamp_min(0)
    NW = (L + 1) // 2
    zf = lambda: torch.zeros((Bn, NW), dtype=torch.float64, device=dev)  # noqa: E731
    wd, wn = zf().scatter_add_(1, wid, dur * is_lab), zf().scatter_add_(1, wid, numer * is_lab)
    idx = torch.arange(L, device=dev)[None].expand(Bn, L)
    wfirst = zf().scatter_add_(1, wid, (idx * first).double()).int()
    wlast = zf().scatter_add_(1, wid, (idx * final).double()).int()
    wstart = zf().scatter_add_(1, wid, (start * first).double()).int()
    wend = zf().scatter_add_(1, wid, (end * final).double()).int()
    n_words = first.sum(1).int()
    has = torch.arange(NW, device=dev)[None] < n_words[:, None]
    return {"log_prob": logp.float(), "start": start, "end": end, "duration": dur.float(), "log_confidence": log_conf.float(),
            "word_first": wfirst, "word_count": ((wlast - wfirst + 1) * has).int(), "word_start": wstart, "word_end": wend,
            "word_log_confidence": torch.where(has, wn / wd, torch.zeros_like(wd)).float(), "n_words": n_words}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-rounds", type=int, default=2)
    ap.add_argument("--errors-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_segment_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ctc_segment.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")

    worst, margin, tally, per_case = errors_on_parity_cases(dev)
    out = {"tool": "tools/bench_ctc_segment.py", "device": torch.cuda.get_device_name(0),
           "errors": {"cases": len(R.PARITY) + len(R.PLANTED), "rows_per_parity_case": len(R.SCALES), **worst, "decided_margin": margin, **tally,
                      "undecided_share": round(tally["undecided"] / max(tally["boundaries"], 1), 5), "per_case": per_case}}
    if tally["wrong"]:
        print(json.dumps(out["errors"], indent=1))
        raise SystemExit("bench_ctc_segment.py: decided boundaries differ from the oracle")
    if not args.errors_only:
        out.update(timing(args, dev))
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


def timing(args, dev):
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.infer import ASRPipeline
    x = torch.from_numpy(peaked_logits()).to(dev)
    ids, n = ctc_greedy_decode(x)
    L = int(n.max())
    labels = ids[:, :L].contiguous()
    counts = n.cpu().numpy()

    # the timed shape is right: (a) against the oracle, (b) against (a) on the decided boundaries
    xh, lh = x.cpu().numpy(), labels.cpu().numpy()
    ref = R.segment_batch(xh, None, lh, counts)
    got = to_numpy(ctc_segment(x, None, labels, n))
    stock = {k: v.cpu().numpy() for k, v in stock_segment(x, labels, n).items()}
    _, margin, _, _ = errors_on_parity_cases(dev)
    agree = {"launch_vs_oracle": R.compare(got, ref, margin), "stock_vs_oracle": R.compare(stock, ref, margin)}
    if agree["launch_vs_oracle"]["wrong"] or agree["stock_vs_oracle"]["wrong"]:
        raise SystemExit(f"bench_ctc_segment.py: the timed shape disagrees with the oracle: {agree}")
    for k in ("word_first", "word_count", "n_words"):
        if not np.array_equal(got[k], stock[k]):
            raise SystemExit(f"bench_ctc_segment.py: {k} of the stock arm differs from the launch")

    host = []
    for _ in range(args.host_rounds):                                    # arm (c)
        t0 = time.perf_counter()
        R.segment_batch(x.cpu().numpy(), None, labels.cpu().numpy(), n.cpu().numpy())
        host.append((time.perf_counter() - t0) * 1e3)

    torch.manual_seed(0)
    model = AudioToTextCTC(64, 512, V, 512).to(dev).eval()
    audio = torch.randn(B, 1024, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    fs = 0.02
    greedy, beam = ASRPipeline(model, frame_seconds=fs), ASRPipeline(model, beam_size=16, frame_seconds=fs)
    arms = {"segment": lambda: ctc_segment(x, None, labels, n),
            "stock_ops": lambda: stock_segment(x, labels, n),
            "ctc_align": lambda: ctc_align(torch.log_softmax(x, -1), labels, None, n),
            "forward": lambda: model(audio),
            "pipeline_call_greedy": lambda: greedy(audio), "pipeline_segments_greedy": lambda: greedy.segments(audio),
            "pipeline_call_beam16": lambda: beam(audio), "pipeline_segments_beam16": lambda: beam.segments(audio)}
    with torch.no_grad():
        for fn in arms.values():
            window(fn, 2)
        iters = {k: iters_for(fn, args.window) for k, fn in arms.items()}
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                times[k].append(window(fn, iters[k]))
    res = {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}
    res["host_oracle"] = dict(summary(host), calls_per_window=1, clock="host perf_counter, .cpu() copies included")
    a = res["segment"]["median_ms"]
    noise = max(res[k]["spread"] for k in ("segment", "stock_ops"))
    bar = max(0.03, 3 * noise)
    pipe_len = int(greedy(audio)[1].max())
    return {"shape": {"B": B, "T": T, "V": V, "Lmax": L, "labels_min_mean_max": [int(counts.min()), round(float(counts.mean()), 1),
                                                                                  int(counts.max())]},
            "method": f"windows of >= {args.window} s of back-to-back whole calls between device events, {args.rounds} alternating "
                      f"rounds; host arm: {args.host_rounds} calls on the host clock",
            "agreement_at_timed_shape": agree, "arms": res, "bar": round(bar, 4),
            "summary": {"segment_ms": a, "us_per_frame": round(a * 1e3 / T, 3),
                        "stock_over_segment": round(res["stock_ops"]["median_ms"] / a, 1),
                        "stock_clears_the_bar": bool(res["stock_ops"]["median_ms"] / a - 1 > bar),
                        "host_over_segment": round(res["host_oracle"]["median_ms"] / a, 1),
                        "host_clears_the_bar": bool(res["host_oracle"]["median_ms"] / a - 1 > max(bar, 3 * res["host_oracle"]["spread"])),
                        "segment_over_ctc_align": round(a / res["ctc_align"]["median_ms"], 2),
                        "share_of_forward": round(a / res["forward"]["median_ms"], 4),
                        "pipeline_segments_over_call_greedy": round(res["pipeline_segments_greedy"]["median_ms"] /
                                                                    res["pipeline_call_greedy"]["median_ms"], 3),
                        "pipeline_segments_over_call_beam16": round(res["pipeline_segments_beam16"]["median_ms"] /
                                                                    res["pipeline_call_beam16"]["median_ms"], 3),
                        "pipeline_longest_hypothesis": pipe_len},
            "not_measured": "the kernel alone under a profiler (figures are whole calls with their allocations); a trained model "
                            "(the pipeline arms run seeded weights, whose greedy hypotheses are short); Lmax > 255 (more than one "
                            "state pair per thread) was timed nowhere"}


if __name__ == "__main__":
    main()
