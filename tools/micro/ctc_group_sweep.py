"""Where the grouped hand-over of the CTC wave pipeline (csrc/ctc.hip) beats the per-frame one: the whole v100_ctc_loss call (lse,
lattice, gradient; only the lattice differs between the forms) timed with both forms forced, over padded length T x waves.
B = 32, V = 29, full-length rows, labels of Lmax tokens where they fit the frames (else as many as fit): the benchmark's kind of batch.
Median of --reps calls after --warm, device events.  The host rule's threshold CTC_GROUP_MIN_T is read off this table
(profiles/ctc_group_ab.txt).

    python tools/micro/ctc_group_sweep.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from voice100_amd import _native as N  # noqa: E402

WAVES = {1: 31, 2: 63, 4: 100, 8: 255, 16: 511}          # waves -> Lmax
LENGTHS = (8, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 1024)


def time_call(dev, T, Lmax, form, warm, reps, B=32, V=29):
    g = torch.Generator().manual_seed(T * 7 + Lmax)
    logits = (torch.randn(B, T, V, generator=g) * 2).to(dev)
    labels = (torch.randint(1, V, (B, Lmax), generator=g)).to(dev)
    il = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl = torch.full((B,), min(Lmax, T // 2), dtype=torch.int32, device=dev)
    ws = torch.empty((int(N.helper("v100_ctc_workspace_floats", B, T, Lmax)),), device=dev)
    nll = torch.empty(B, device=dev)
    grad = torch.empty(B * T * V, device=dev)
    N.call("v100_ctc_lattice_form", form)
    try:
        times = []
        for i in range(warm + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            N.call("v100_ctc_loss", logits, labels, il, tl, ws, nll, grad, B, T, V, Lmax, 0)
            b.record()
            b.synchronize()
            if i >= warm:
                times.append(a.elapsed_time(b) * 1e3)
    finally:
        N.call("v100_ctc_lattice_form", -1)
    times.sort()
    return times[len(times) // 2], float(nll.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_group_sweep.py needs a GPU")
    dev = torch.device("cuda:0")
    group = int(N.helper("v100_ctc_lattice_plan", 1 << 20, 0))        # long enough for the rule to pick the grouped form
    rows = []
    print(f"group of {group} frames; call time in us, median of {args.reps}")
    print("waves      T   per-frame   grouped   grouped/per-frame   rule")
    for nw, Lmax in WAVES.items():
        for T in LENGTHS:
            t0, s0 = time_call(dev, T, Lmax, 0, args.warm, args.reps)
            t1, s1 = time_call(dev, T, Lmax, 1, args.warm, args.reps)
            if s0 != s1 and not (s0 != s0 and s1 != s1):
                raise SystemExit(f"the forms disagree at T {T}, Lmax {Lmax}: {s0} vs {s1}")
            rule = int(N.helper("v100_ctc_lattice_plan", T, Lmax))
            rows.append({"waves": nw, "T": T, "per_frame_us": t0, "grouped_us": t1, "rule_group": rule})
            print(f"{nw:5d} {T:6d} {t0:11.1f} {t1:9.1f} {t1 / t0:19.3f} {rule:6d}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"group": group, "B": 32, "V": 29, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
