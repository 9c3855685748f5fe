"""Cost of gradient clipping at the bench configuration (asr_en_base, B = 32 x 1024 frames, bf16, augmentation + dropout + FusedAdam):
TrainStep with clipping off, with norm clipping at 1.0 (the reference recipes' trainer.gradient_clip_val) and with value clipping at 1.0.

  python tools/bench_clip.py [--rounds R --steps K] --out time.json
      step time of the three settings, alternated round by round on one model (device-synchronised windows of K steps, the same seeds for the
      three settings of a round; median of R)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o clip -- python tools/bench_clip.py --trace --steps K
      K steps of each setting under the kernel tracer (a run of its own: tracing slows the host)
  python tools/bench_clip.py --report DIR/.../clip_kernel_stats.csv [--time time.json] --out summary.json
      per-kernel times of the Adam step with and without the clip and of the partials kernel, its bytes / time against 8 TB/s
"""
import argparse
import csv
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0
N_PARAMS = 11621661                    # asr_en_base (README.md:135-147): one fp32 gradient element each
SETTINGS = (("off", None, "norm"), ("norm", 1.0, "norm"), ("value", 1.0, "value"))


def setup():
    import numpy as np
    import torch
    from bench import B_PER_GPU, N_MEL, T_FRAMES, VOCAB, synth_batch
    from voice100_amd import functional as F_
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.trainer import TrainStep
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py needs a GPU")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    F_.set_matmul_precision("bf16")
    random.seed(1234); np.random.seed(1234); torch.manual_seed(1234)
    model = AudioToTextCTC(N_MEL, 512, VOCAB, 512, learning_rate=1e-3, weight_decay=4e-5).to(dev)
    assert sum(p.numel() for p in model.parameters()) == N_PARAMS
    step = TrainStep(model)
    # as bench.py: size the caching allocator for the longest time-stretched batch before anything is timed
    aug = model.batch_augment
    keep, aug.do_timestretch = aug.do_timestretch, False
    (a_long, _), tgt = synth_batch(dev, B_PER_GPU, 99, frames=T_FRAMES * 149 // 100)
    step(((a_long, torch.full((B_PER_GPU,), a_long.shape[1], dtype=torch.int32, device=dev)), tgt))
    aug.do_timestretch = keep
    return step, synth_batch(dev, B_PER_GPU, 1234)


def use(step, setting):
    _, val, algorithm = setting
    step.clip_val, step.clip_algorithm = val, algorithm        # the state TrainStep(gradient_clip_val=..., ...) sets up


def run_time(args):
    import torch
    step, batch = setup()
    for s in SETTINGS:
        use(step, s)
        for _ in range(args.warmup):
            step(batch)
    torch.cuda.synchronize()
    ms = {s[0]: [] for s in SETTINGS}
    norms = []
    for r in range(args.rounds):
        for s in SETTINGS:
            use(step, s)
            # the same augmentation draws (time-stretch lengths) and dropout masks for the three settings of a round
            random.seed(r); torch.manual_seed(r)
            step(batch); step(batch)                          # the switch's first steps stay out of the window
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(batch)
            torch.cuda.synchronize()
            ms[s[0]].append((time.perf_counter() - t0) / args.steps * 1e3)
            if s[0] == "norm":
                norms.append(float(step.last_grad_norm))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"config": "asr_en_base B=32 T=1024 bf16, augmentation + dropout + FusedAdam", "rounds": args.rounds, "steps": args.steps,
           "ms_per_step": ms, "median_ms": med,
           "overhead_pct": {k: 100.0 * (med[k] / med["off"] - 1.0) for k in ("norm", "value")},
           "overhead_us": {k: 1e3 * (med[k] - med["off"]) for k in ("norm", "value")},
           "grad_norm_at_window_end": norms, "norm_clip_engaged": [n > 1.0 for n in norms]}
    return out


def run_trace(args):
    import torch
    step, batch = setup()
    for s in SETTINGS:
        use(step, s)
        for _ in range(args.steps):
            step(batch)
        torch.cuda.synchronize()
    return {"traced_steps_per_setting": args.steps}


def report(args):
    rows = list(csv.DictReader(open(args.report)))
    grad_bytes = 4 * N_PARAMS

    def kern(name):
        r = [x for x in rows if name in x["Name"]]
        if not r:
            return None
        calls = sum(int(x["Calls"]) for x in r)
        return {"name": r[0]["Name"][:120], "calls": calls, "avg_us": sum(float(x["TotalDurationNs"]) for x in r) / calls / 1e3}

    out = {"adam_step_kernel": kern("adam_step_kernel("), "adam_step_clip_kernel<norm>": kern("adam_step_clip_kernel<1>"),
           "adam_step_clip_kernel<value>": kern("adam_step_clip_kernel<2>"), "grad_norm_partials_kernel": kern("grad_norm_partials_kernel<false>")}
    for k, v in out.items():
        if v is None:
            raise SystemExit(f"{k}: not in {args.report}")
    p = out["grad_norm_partials_kernel"]
    p["bytes"] = grad_bytes
    p["GBps"] = grad_bytes / (p["avg_us"] * 1e3)
    p["fraction_of_8TBps"] = p["GBps"] / HBM_PEAK_GBS
    # the Adam kernels: p, g, m, v read, p, m, v written (+ g written back when the clip changed it)
    out["adam_step_kernel"]["fraction_of_8TBps"] = 7 * grad_bytes / (out["adam_step_kernel"]["avg_us"] * 1e3) / HBM_PEAK_GBS
    out["norm_clip_kernel_us_per_step"] = p["avg_us"] + out["adam_step_clip_kernel<norm>"]["avg_us"] - out["adam_step_kernel"]["avg_us"]
    out["value_clip_kernel_us_per_step"] = out["adam_step_clip_kernel<value>"]["avg_us"] - out["adam_step_kernel"]["avg_us"]
    if args.time:
        t = out["step_time"] = json.load(open(args.time))
        ms = t["ms_per_step"]
        # the three settings of a round share seeds and weights: the per-round differences are the paired cost
        for k in ("norm", "value"):
            d = [1e3 * (a - b) for a, b in zip(ms[k], ms["off"])]
            out[f"step_overhead_{k}_paired"] = {"us_per_round": d, "median_us": statistics.median(d),
                                                "median_pct": 100.0 * statistics.median(d) / 1e3 / t["median_ms"]["off"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--report", metavar="KERNEL_STATS_CSV")
    ap.add_argument("--time", metavar="TIME_JSON", help="--report: include this step-time result")
    ap.add_argument("--out")
    args = ap.parse_args()
    out = report(args) if args.report is not None else run_trace(args) if args.trace else run_time(args)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
