#!/usr/bin/env python3
"""Time the ragged log-mel launch (MelSpectrogramAudioTransform.transform(waveform, lengths), v100_log_mel_fused_len, K21) beside the
two things the tree offered before it.

Input: B = 32 seeded utterances of 5 to 16 s at 16 kHz (one of each extreme), randn * 0.1, in one [B, N] tensor, N = 256000 samples,
zero beyond each utterance; the lengths as an int32 tensor on the device (what audio_io.load_batch returns), so T = 1 + N // hop in
every arm and the arms write the same number of bytes.  Arms, in one process:
  (a) ragged:       transform(x, lengths) -- one launch, the batch the reference's collate builds;
  (b) dense_padded: transform(x) on the same zero-padded tensor -- the yardstick for the same bytes, NOT the same result: the
                    frames at and after each utterance's end are those of the zeros, not the reference's;
  (c) loop:         what gave the right batch before -- transform(x[b, :n]) per utterance, then pad_sequence with log(1e-6);
  (a_full) ragged_full: transform(x_full, lengths = N everywhere) on a tensor without padding, against
  (b_full) dense_full:  transform(x_full) -- the same work plus one length load per frame.  The bar on the ragged kernel is this
                    pair: (a_full) may be slower than (b_full) by no more than the larger of 3 % and three times the measured
                    spread of the two arms.
Before anything is timed the outputs are compared at the timed shape: (a) equals (c) and (a_full) equals (b_full), bit for bit.
Then, after a warm-up, --rounds rounds alternate the arms; each timing is one window of at least --window seconds of back-to-back
calls between two device events, ended by a device synchronise.  Reported per arm: every round, the median and the spread
(max - min) / median.
    python tools/bench_mel_ragged.py [--window 0.5] [--rounds 7] [--out profiles/mel_ragged_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
from torch.nn.utils.rnn import pad_sequence

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice100_amd.mel import MelSpectrogramAudioTransform  # noqa: E402

B, SR, MIN_S, MAX_S = 32, 16000, 5, 16


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "mel_ragged_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mel_ragged.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    tr = MelSpectrogramAudioTransform().to(dev)
    gen = torch.Generator().manual_seed(0)
    N = MAX_S * SR
    lengths = torch.randint(MIN_S * SR, N + 1, (B,), generator=gen)
    lengths[0], lengths[1] = N, MIN_S * SR
    x_full = (torch.randn(B, N, generator=gen) * 0.1).to(dev)
    x = x_full * (torch.arange(N)[None, :] < lengths[:, None]).to(dev)       # zero beyond each utterance
    host = lengths.tolist()
    lens = lengths.to(dev, torch.int32)
    full = torch.full((B,), N, dtype=torch.int32, device=dev)
    blank = math.log(tr.log_offset)

    def loop():
        return pad_sequence([tr.transform(x[b, :n]) for b, n in enumerate(host)], batch_first=True, padding_value=blank)

    arms = {"ragged": lambda: tr.transform(x, lens), "dense_padded": lambda: tr.transform(x), "loop": loop,
            "ragged_full": lambda: tr.transform(x_full, full), "dense_full": lambda: tr.transform(x_full)}

    got, got_len = arms["ragged"]()
    want = arms["loop"]()
    got_full, got_full_len = arms["ragged_full"]()
    equal = {"ragged_vs_loop": bool(torch.equal(got, want)),
             "ragged_lengths": got_len.tolist() == [1 + n // tr.hop_length for n in host],
             "ragged_full_vs_dense_full": bool(torch.equal(got_full, arms["dense_full"]())),
             "ragged_full_lengths": got_full_len.tolist() == [1 + N // tr.hop_length] * B}
    if not all(equal.values()):
        raise SystemExit(f"bench_mel_ragged.py: the arms disagree at the timed shape: {equal}")
    padded_wrong = int((arms["dense_padded"]() != got).any(dim=2).sum())      # frames of (b) that are not the reference's

    for fn in arms.values():
        window(fn, 5)
    iters = {k: iters_for(fn, args.window) for k, fn in arms.items()}
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, iters[k]))
    res = {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}

    ratio = res["ragged_full"]["median_ms"] / res["dense_full"]["median_ms"]
    allowed = max(0.03, 3.0 * max(res["ragged_full"]["spread"], res["dense_full"]["spread"]))
    frames = sum(1 + n // tr.hop_length for n in host)
    out = {"tool": "tools/bench_mel_ragged.py", "device": torch.cuda.get_device_name(0),
           "shape": {"B": B, "N": N, "T": 1 + N // tr.hop_length, "n_mels": tr.n_mels, "seconds": [MIN_S, MAX_S],
                     "samples": int(lengths.sum()), "frames_of_utterances": frames, "frames_of_batch": B * (1 + N // tr.hop_length)},
           "method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds",
           "outputs_equal_at_timed_shape": equal, "dense_padded_frames_that_differ_from_the_reference": padded_wrong, "arms": res,
           "ragged_over_dense_padded": round(res["ragged"]["median_ms"] / res["dense_padded"]["median_ms"], 4),
           "loop_over_ragged": round(res["loop"]["median_ms"] / res["ragged"]["median_ms"], 3),
           "bar": {"what": "ragged_full / dense_full: all lengths = N, the dense kernel's work plus one length load per frame",
                   "ragged_full_over_dense_full": round(ratio, 4),
                   "allowed_excess": round(allowed, 4), "rule": "max(3 %, 3 x the larger spread of the two arms)",
                   "met": bool(ratio <= 1.0 + allowed)}}
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
