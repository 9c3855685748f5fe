#!/usr/bin/env python3
"""Time WORLDStat.update (csrc/world_stat.hip, K19) beside the stock-op statement of the reference's formula and the copy yardstick.

Shapes (B, T, S, A): the configs' WORLD batch (16, 1000, 257, 1), mel-cepstrum features (16, 1000, 25, 1), the 22.05 kHz vocoder
(16, 1000, 513, 2) and a 256-utterance batch (256, 1000, 257, 1) that no cache holds.  Per shape, in one process, after a warm-up:
rounds that alternate
  (a) update: two library launches;
  (b) the reference's arithmetic (voice100/calc_stat.py:42-56) in stock torch ops on the same device tensors -- its fp32 masks,
      products and sums, added into double accumulators on the device;
  (c) for the large shape, v100_copy_probe moving the same bytes (a copy of n / 2 bytes reads and writes n in all).
Each timing is one window of at least --window seconds of back-to-back calls between two device events, ended by a device
synchronise; the calls rotate through enough input sets to pass 256 MiB (the Infinity Cache).  Reported: the median window.
Lengths are uniform in [T / 2, T] with one full row, so about a quarter of each batch is padding that update never reads; the
GB/s column counts the bytes of the valid frames only.
    python tools/bench_world_stat.py [--window 0.5] [--rounds 5] [--shape B,T,S,A ...] [--out profiles/world_stat_bench.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice100_amd import _native as N  # noqa: E402
from voice100_amd.calc_stat import WORLDStat  # noqa: E402

SHAPES = ((16, 1000, 257, 1), (16, 1000, 25, 1), (16, 1000, 513, 2), (256, 1000, 257, 1))
L3_BYTES = 256 << 20


class StockStat:
    """The reference's accumulation step, op for op, with its accumulators as double tensors on the device."""

    def __init__(self, S, A, device):
        z = lambda n: torch.zeros(n, dtype=torch.double, device=device)  # noqa: E731
        self.f0_sum, self.f0_sqrsum, self.f0_count, self.logspc_count = z(1), z(1), z(1), z(1)
        self.logspc_sum, self.logspc_sqrsum, self.codeap_sum, self.codeap_sqrsum = z(S), z(S), z(A), z(A)

    @torch.no_grad()
    def update(self, f0, f0_len, logspc, codeap):
        mask = (torch.arange(f0.shape[1], device=f0.device)[None, :] < f0_len[:, None]).to(f0.dtype)
        f0mask = (f0 > 30.0).float() * mask
        codeapmask = (codeap < -0.2).float() * mask[:, :, None]
        self.f0_sum += torch.sum(f0 * f0mask)
        self.f0_sqrsum += torch.sum(f0 ** 2 * f0mask)
        self.f0_count += torch.sum(f0mask)
        self.logspc_sum += torch.sum(torch.sum(logspc * mask[:, :, None], axis=1), axis=0)
        self.logspc_sqrsum += torch.sum(torch.sum(logspc ** 2 * mask[:, :, None], axis=1), axis=0)
        self.logspc_count += torch.sum(mask)
        self.codeap_sum += torch.sum(torch.sum(codeap * codeapmask, axis=1), axis=0)
        self.codeap_sqrsum += torch.sum(torch.sum(codeap ** 2 * codeapmask, axis=1), axis=0)


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters                                 # ms per call


def iters_for(fn, seconds):
    per_call = max(window(fn, 20), 1e-4)
    return max(20, int(seconds * 1e3 / per_call) + 1)


def make_set(B, T, S, A, dev, gen):
    lens = torch.randint(T // 2, T + 1, (B,), generator=gen)
    lens[0] = T
    voiced = torch.rand(B, T, generator=gen) >= 0.4
    f0 = torch.where(voiced, 80.0 + 200.0 * torch.rand(B, T, generator=gen), torch.zeros(())).to(dev)
    logspc = torch.randn(B, T, S, device=dev) * 2.0 - 8.0
    codeap = torch.where(torch.rand(B, T, A, device=dev) < 0.6, -0.3 - 20.0 * torch.rand(B, T, A, device=dev),
                         -1e-3 * torch.rand(B, T, A, device=dev))
    return f0, lens.to(dev, torch.int32), logspc, codeap, int(lens.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shape", action="append", help="B,T,S,A (repeatable) instead of the four standard shapes")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "world_stat_bench.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_world_stat.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    lines = [f"# tools/bench_world_stat.py: windows of >= {args.window} s of back-to-back calls, device events, median of {args.rounds} alternating rounds",
             f"# device: {torch.cuda.get_device_name(0)}; (a) WORLDStat.update, (b) the reference's formula in stock torch ops, (c) v100_copy_probe of the same bytes",
             "# B    T    S    A   batch_MB  valid_MB  parts  update_ms  valid_GB/s  stock_ms  stock/update  copy_ms  update/copy"]
    ok = True
    for B, T, S, A in ([tuple(int(v) for v in s.split(",")) for s in args.shape] if args.shape else SHAPES):
        nbytes = 4 * B * T * (1 + S + A)
        sets = L3_BYTES // nbytes + 2
        data = [make_set(B, T, S, A, dev, gen) for _ in range(sets)]
        valid = statistics.mean(d[4] for d in data) * 4 * (1 + S + A)
        stat, stock = WORLDStat(S, A, device=dev), StockStat(S, A, dev)

        def run_update(i):
            stat.update(*data[i % sets][:4])

        def run_stock(i):
            stock.update(*data[i % sets][:4])
        runs = [run_update, run_stock]
        if 2 * nbytes > L3_BYTES:                                        # the bandwidth regime: the rotation passes the cache
            half = (int(valid) // 2 + 15) & ~15                          # the bytes update reads: the valid frames
            src = [torch.zeros(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
            dst = [torch.empty(half, dtype=torch.uint8, device=dev) for _ in range(sets)]
            runs.append(lambda i: N.call("v100_copy_probe", src[i % sets], dst[i % sets], half))
        for fn in runs:                                                  # warm-up: code objects, allocator, clocks
            window(fn, 2 * sets + 10)
        iters = [iters_for(fn, args.window) for fn in runs]
        times = [[] for _ in runs]
        for _ in range(args.rounds):
            for k, fn in enumerate(runs):
                times[k].append(window(fn, iters[k]))
        u, s = statistics.median(times[0]), statistics.median(times[1])
        copy = f"{statistics.median(times[2]):7.4f}  {u / statistics.median(times[2]):11.2f}" if len(runs) == 3 else "not measured (launch-latency regime)"
        parts = N.helper("v100_world_stat_parts", B, T, S)
        lines.append(f"{B:>4} {T:>4} {S:>4} {A:>4}  {nbytes / 1e6:8.2f}  {valid / 1e6:8.2f}  {parts:>5}  {u:9.4f}  {valid / u / 1e6:10.1f}  {s:8.4f}  {s / u:12.2f}  {copy}"
                     f"     (update rounds {min(times[0]):.4f}..{max(times[0]):.4f} ms, stock {min(times[1]):.4f}..{max(times[1]):.4f} ms, {iters[0]}/{iters[1]} calls per window)")
        ok = ok and u < s
        del data, stat, stock
        torch.cuda.empty_cache()
    lines.append("# update faster than the stock ops at every shape: " + ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
