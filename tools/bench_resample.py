#!/usr/bin/env python3
"""Time the device resampler (csrc/resample.hip) beside the library's copy yardstick.

B = 16 utterances of 10 s, for 44.1 -> 16 kHz, 48 -> 16 kHz and 16 -> 22.05 kHz.  Each v100_resample_sinc launch reads its input once and
writes its output once, so the yardstick is v100_copy_probe moving the same bytes: a copy of (input + output) / 2 bytes reads and writes
input + output bytes in all.  Both rotate through enough buffer sets to pass 256 MiB (the Infinity Cache), alternate in rounds after a
warm-up (clocks up, code objects loaded), and are timed with device events around `--iters` launches; the median round is reported.
No time here is a pass criterion: the figure to read is the ratio to the copy.
    python tools/bench_resample.py [--iters 40] [--rounds 5] [--out profiles/resample_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice100_amd import _native as N  # noqa: E402
from voice100_amd import audio_io as A  # noqa: E402

B, SECONDS = 16, 10
PAIRS = ((44100, 16000), (48000, 16000), (16000, 22050))
L3_BYTES = 256 << 20


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    lines = [f"# tools/bench_resample.py: B = {B} x {SECONDS} s, {args.iters} launches per round, median of {args.rounds} rounds, device events",
             f"# device: {torch.cuda.get_device_name(0)}; resample tile {A.resample_tile()} outputs per workgroup",
             "# pair            in_MB  out_MB  resample_ms  resample_GB/s  copy_ms  copy_GB/s  resample/copy"]
    for orig, new in PAIRS:
        k = A.resample_kernel(orig, new)
        n_in = SECONDS * orig
        n_out = A.resample_out_len(n_in, orig, new)
        nbytes = 4 * B * (n_in + n_out)
        sets = L3_BYTES // nbytes + 2
        xs = [torch.randn(B, n_in, device=dev) for _ in range(sets)]
        half = (nbytes // 2 + 15) & ~15
        src = [torch.empty(half, dtype=torch.uint8, device=dev).zero_() for _ in range(sets)]
        dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(sets)]

        def run_resample(i):
            A.resample(xs[i % sets], orig, new)

        def run_copy(i):
            N.call("v100_copy_probe", src[i % sets], dst[i % sets], half)
        for i in range(2 * sets):
            run_resample(i)
            run_copy(i)
        torch.cuda.synchronize()
        t_res, t_copy = [], []
        for _ in range(args.rounds):
            t_res.append(timed(run_resample, args.iters))
            t_copy.append(timed(run_copy, args.iters))
        r, c = statistics.median(t_res), statistics.median(t_copy)
        lines.append(f"{orig:>6}->{new:<6}  {4 * B * n_in / 1e6:7.2f} {4 * B * n_out / 1e6:7.2f}  {r:11.4f}  {nbytes / r / 1e6:13.1f}  {c:7.4f}  "
                     f"{2 * half / c / 1e6:9.1f}  {r / c:13.2f}     (o/n {k.o}/{k.n}, {k.L} taps, rounds {min(t_res):.4f}..{max(t_res):.4f} ms)")
        del xs, src, dst
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
