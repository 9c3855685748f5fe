#!/usr/bin/env python
"""K33, decode.ctc_segment_long: its error against the banded float64 oracle over the tests' case lists, and its time on four
recordings of 90,000 planted frames (30 minutes at 20 ms) with 25,000 labels each, V = 29, band 256.  Writes
profiles/ctc_segment_long_bench.json.

Errors: the largest |log_prob| error (relative to max(1, |log_prob|)), |duration| and |log_confidence| errors (absolute) per group of
tests/_ctc_segment_long_ref.py's cases: the exact form, the moving window (diffuse and planted), the exponent-range case and the
20,000-frame case.  The tests' tolerances beyond K26's shapes are the last two groups' maxima x 8 rounded up to one digit, and a
boundary counts as decided when its oracle margin exceeds max(8 x the duration error, 1e-5), which must stay <= 1e-3.

Time, whole calls with their allocations, one call per window between device events, --rounds alternating rounds, median and
spread (max - min) / median per arm:
  (a)  decode.ctc_segment_long with the corridor given (the two launches alone), at bands 64 / 256 / 1024, and
  (a+) with neither path nor corridor: log_softmax + decode.ctc_align_long (band 2048) + ctc_corridor + the launches;
  (b)  the same banded recurrence (alpha and beta rows only, no posteriors, no reductions: a lower bound) in stock torch ops on the
       device in float64, timed on the first --slice frames and SCALED by T / slice;
  (c)  the float64 numpy oracle on the host clock, one recording, times four;
  (d)  log_softmax + decode.ctc_align_long alone, the hard-alignment neighbour, and K31's way to the same kind of numbers: the
       recording cut into pieces of at most 3,000 frames (here at the planted path's blanks) and decode.ctc_segment on the batch of
       pieces, which gives times and confidences per piece, each piece's posterior blind to its neighbours.
The bar for a ratio: slower / faster - 1 > max(3 %, 3 x the larger spread).  Not measured: a profiler run, a trained model's logits,
real recordings.  --errors-only skips the timing."""
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
import _align_long_ref as AR  # noqa: E402
import _ctc_segment_long_ref as LR  # noqa: E402
import _ctc_segment_ref as R  # noqa: E402
from voice100_amd.decode import ctc_align_long, ctc_corridor, ctc_segment, ctc_segment_long  # noqa: E402

B, T, L, V, BAND = 4, 90000, 25000, 29, 256
# the compiler's resource summary of csrc/ctc_segment_long.hip for gfx950 (-Rpass-analysis=kernel-resource-usage), transcribed by hand:
# nothing keeps it in step with the kernel, and the record says so
RESOURCES = {"ctc_segment_long_kernel<1> (band <= 512)": {"vgprs": 99, "lds_bytes": 49168, "scratch_bytes": 0},
             "ctc_segment_long_kernel<2> (band <= 1024)": {"vgprs": 120, "lds_bytes": 49168, "scratch_bytes": 0},
             "ctc_segment_long_words_kernel": {"vgprs": 40, "lds_bytes": 1024, "scratch_bytes": 0}}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(times):
    med = statistics.median(times)
    return {"rounds_ms": [round(t, 3) for t in times], "median_ms": round(med, 3), "spread": round((max(times) - min(times)) / med, 4)}


def to_numpy(seg):
    return {k: v.cpu().numpy() for k, v in seg._asdict().items() if v is not None}


def device(dev, x, labels, lo, band):
    return to_numpy(ctc_segment_long(torch.from_numpy(x).to(dev), None, torch.from_numpy(labels).to(dev), None,
                                     lo=torch.from_numpy(np.asarray(lo, np.int32)).to(dev), band=band))


def error_groups(dev):
    groups = {}

    def add(name, got, ref):
        g = groups.setdefault(name, {"log_prob_rel": 0.0, "duration_abs": 0.0, "log_confidence_abs": 0.0, "cases": 0, "pairs": []})
        c = R.compare(got, ref, 0.0)
        for k in ("log_prob_rel", "duration_abs", "log_confidence_abs"):
            g[k] = max(g[k], c[k])
        g["cases"] += 1
        g["pairs"].append((got, ref))
    for T_, L_, V_ in LR.EXACT:
        x, labels = R.parity_case(T_, max(L_, 1), V_)
        if L_ == 0:
            continue                                     # (no label: log_prob alone, covered by the tests)
        band = 64 * ((2 * L_ + 1 + 63) // 64)
        lo = np.zeros((3, (T_ + 15) // 16), np.int32)
        add("exact", device(dev, x, labels, lo, band), R.segment_batch(x, None, labels, None))
    for T_, L_, V_ in LR.MOVING:
        for name, (x, labels) in (("moving_diffuse", LR.diffuse_case(T_, L_, V_)), ("moving_planted", LR.planted_case(T_, L_, V_, 6.0)[:2])):
            lo = np.stack([LR.viterbi_corridor(x[r], labels[r], LR.MOVING_BAND)[0] for r in range(len(x))])
            add(name, device(dev, x, labels, lo, LR.MOVING_BAND), LR.segment_batch_banded(x, None, labels, None, lo, LR.MOVING_BAND))
    x, labels = LR.overflow_case()
    lo = np.zeros((1, (x.shape[1] + 15) // 16), np.int32)
    add("overflow", device(dev, x, labels, lo, 64), LR.segment_batch_banded(x, None, labels, None, lo, 64))
    T_, L_, V_, W_, nats = LR.LONG
    x, labels, path = LR.planted_case(T_, L_, V_, nats)
    lo = LR.corridor(path, T_, L_, W_)[None]
    add("long", device(dev, x, labels, lo, W_), LR.segment_batch_banded(x, None, labels, None, lo, W_))
    for g in groups.values():
        g["decided_margin"] = max(8 * g["duration_abs"], 1e-5)
        tally = {"boundaries": 0, "undecided": 0, "wrong": 0}
        for got, ref in g.pop("pairs"):
            c = R.compare(got, ref, g["decided_margin"])
            for k in tally:
                tally[k] += c[k]
        g.update(tally)
    return groups


def stock_recurrence(logits, labels, lo, band, frames):
    """Arm (b): alpha and beta rows of the banded lattice over the first `frames` frames in stock torch ops, float64, log domain."""
    dev = logits.device
    Bn = logits.shape[0]
    W = band
    lp = torch.log_softmax(logits[:, :frames].double(), -1)
    n = 2 * labels.shape[1] + 1
    ext = torch.zeros((Bn, n + W + 2), dtype=torch.int64, device=dev)
    ext[:, 1:n:2] = labels
    skip = torch.zeros((Bn, n + W + 2), dtype=torch.bool, device=dev)
    skip[:, 3:n:2] = ext[:, 3:n:2] != ext[:, 1:n - 2:2]
    ar = torch.arange(W, device=dev)[None]
    neg = torch.full((Bn, W), float("-inf"), dtype=torch.float64, device=dev)
    rows = []
    a = neg.clone()
    a[:, :2] = torch.gather(lp[:, 0], 1, ext[:, :2])
    prev_lo = lo[:, 0].long()
    for t in range(1, frames):
        cur = lo[:, t >> 4].long()
        idx = cur[:, None] + ar
        z, sk = torch.gather(ext, 1, idx), torch.gather(skip, 1, idx)
        src = idx - prev_lo[:, None]                     # the slot of each state in the row before
        def take(row, k):
            s = src - k
            ok = (s >= 0) & (s < W)
            return torch.where(ok, torch.gather(row, 1, s.clamp(0, W - 1)), neg)
        a = torch.gather(lp[:, t], 1, z) + torch.logaddexp(torch.logaddexp(take(a, 0), take(a, 1)), torch.where(sk, take(a, 2), neg))
        a = torch.where(idx < n, a, neg)
        rows.append(a)
        prev_lo = cur
    b = neg.clone()
    for t in range(frames - 2, -1, -1):                  # the same work downwards (the end condition does not change the cost)
        cur = lo[:, t >> 4].long()
        idx = cur[:, None] + ar
        z, sk = torch.gather(ext, 1, idx), torch.gather(skip, 1, idx)
        b = torch.gather(lp[:, t], 1, z) + torch.logaddexp(torch.logaddexp(b, b.roll(-1, 1)), torch.where(sk, b.roll(-2, 1), neg))
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slice", type=int, default=1000)
    ap.add_argument("--errors-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_segment_long_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    groups = error_groups(dev)
    for name, g in groups.items():
        print(name, json.dumps(g))
    assert all(g["wrong"] == 0 for g in groups.values())
    result = {"kernel": "K33 decode.ctc_segment_long", "errors": groups, "resources": RESOURCES,
              "resources_note": "not measured by this tool: transcribed by hand from the compiler's remarks "
                                "(-Rpass-analysis=kernel-resource-usage) at the time of writing; rebuild with that flag to check them",
              "rule": "test tolerance = 8 x the measured maximum, rounded up to one digit; decided margin = max(8 x duration error, 1e-5) <= 1e-3",
              "not_measured": ["a profiler run", "a trained model's logits", "real recordings"]}
    if not args.errors_only:
        mats = [AR.planted(1000 + b, T, L, V, nats=6.0) for b in range(B)]
        x = torch.from_numpy(np.stack([m[0] for m in mats])).to(dev)
        labels = torch.from_numpy(np.stack([m[1] for m in mats])).to(dev)
        path = torch.from_numpy(np.stack([m[2] for m in mats])).to(dev)
        lens = torch.full((B,), L, dtype=torch.int32, device=dev)
        los = {W: ctc_corridor(path, None, lens, W) for W in (64, 256, 1024)}
        arms = {f"a_launch_band_{W}": (lambda W=W: ctc_segment_long(x, None, labels, None, lo=los[W], band=W)) for W in (64, 256, 1024)}
        arms["a_plus_aligner_and_corridor"] = lambda: ctc_segment_long(x, None, labels, None, band=BAND)
        arms["d_align_long"] = lambda: ctc_align_long(torch.log_softmax(x, -1), labels, band=2048)
        arms["b_stock_recurrence_slice"] = lambda: stock_recurrence(x, labels, los[BAND], BAND, args.slice)
        # K31's way: pieces of at most 3,000 frames, cut where the planted path sits in a blank; every piece with its own labels
        pieces = []
        for b in range(B):
            p, t0 = mats[b][2], 0
            while t0 < T:
                t1 = min(T, t0 + 3000)
                while t1 < T and t1 > t0 + 1 and p[t1] % 2:
                    t1 -= 1
                i0, i1 = (int(p[t0]) + 1) // 2, (int(p[t1 - 1]) + 1) // 2      # labels wholly inside [t0, t1)
                pieces.append((b, t0, t1, i0, i1))
                t0 = t1
        Tp, Lp = max(p[2] - p[1] for p in pieces), max(p[4] - p[3] for p in pieces)
        px = torch.zeros((len(pieces), Tp, V), device=dev)
        pl = torch.zeros((len(pieces), max(Lp, 1)), dtype=torch.int64, device=dev)
        pt = torch.tensor([p[2] - p[1] for p in pieces], dtype=torch.int32, device=dev)
        pn = torch.tensor([p[4] - p[3] for p in pieces], dtype=torch.int32, device=dev)
        for k, (b, t0, t1, i0, i1) in enumerate(pieces):
            px[k, :t1 - t0] = x[b, t0:t1]
            pl[k, :i1 - i0] = labels[b, i0:i1]
        arms["d_cut_and_batch_ctc_segment"] = lambda: [ctc_segment(px[k:k + 32], pt[k:k + 32], pl[k:k + 32], pn[k:k + 32])
                                                        for k in range(0, len(pieces), 32)]
        for fn in arms.values():                         # warm-up: allocations, code objects
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in arms}
        for _ in range(args.rounds):
            for k, fn in arms.items():
                times[k].append(timed(fn))
        timing = {k: summary(v) for k, v in times.items()}
        scale = T / args.slice
        timing["b_stock_recurrence_scaled"] = {"median_ms": round(timing["b_stock_recurrence_slice"]["median_ms"] * scale, 1),
                                               "note": f"the slice of {args.slice} frames x {scale:g}; alpha and beta rows only"}
        seg = ctc_segment_long(x, None, labels, None, lo=los[BAND], band=BAND)
        assert bool(seg.ok.all())
        t0 = time.perf_counter()
        ref = LR.segment_batch_banded(mats[0][0][None], None, mats[0][1][None], None, los[BAND][:1].cpu().numpy(), BAND)
        host = time.perf_counter() - t0
        timing["c_numpy_oracle_host"] = {"one_recording_s": round(host, 2), "four_recordings_ms": round(4e3 * host, 0), "note": "one row timed, times four"}
        got = {k: v[:1] for k, v in to_numpy(seg).items()}
        c = R.compare(got, ref, 1e-5)
        timing["workload_check_row0"] = c
        a = timing[f"a_launch_band_{BAND}"]["median_ms"]
        timing["ratios_to_a"] = {k: round(v["median_ms"] / a, 3) for k, v in timing.items() if isinstance(v, dict) and "median_ms" in v}
        timing["workload"] = {"B": B, "T": T, "L": L, "V": V, "band": BAND, "pieces": len(pieces), "piece_frames": Tp, "piece_labels": Lp,
                              "workspace_MB": round(12 * B * T * BAND / 2 / 1e6, 1)}
        result["timing"] = timing
        for k, v in timing.items():
            print(k, json.dumps(v))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
