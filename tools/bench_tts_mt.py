#!/usr/bin/env python3
"""Time K22 (functional.masked_cross_entropy, csrc/phone_loss.hip) beside the stock-op chain it replaces, then the whole training
step of AlignTextToAudioMultiTaskModel beside AlignTextToAudioModel's.

K22 shape: B = 32, V = 71, L = 512 fp32 logits [B, V, L], ragged target lengths (uniform in [L / 2, L], one full row), forward +
backward with a unit upstream gradient.  Arms, in one process, on the same logits:
  (a) fused: masked_cross_entropy -- two launches forward, one backward;
  (b) stock: cross_entropy(reduction='none'), the mask, two sums, a division, and autograd's backward (tts.py:328-331 as written).
Before anything is timed the two arms' loss and d loss / d logits are compared at the timed shape (rel_err < 1e-4, or the tool
stops).  Then, after a warm-up and one discarded window per arm, --rounds rounds alternate the arms; each timing is one window of
at least --window seconds of back-to-back calls between two device events, ended by a device synchronise.  Reported per arm: every
round, the median, the spread (max - min) / median -- the spread of repeating ONE arm is the yardstick a difference between the
arms is read against -- and the device kernels of one call (counted by torch.profiler in a pass of its own, after the timing; the library's own launches
from v100_launch_count()).  The bar: the fused arm is not slower than the stock arm by more than max(3 %, 3 x the larger spread).

Step shape: hidden 512, B = 16, L = 512 aligned-text positions (1023 WORLD frames, 257 log-spectrum bins), Vt = 71, precision
bf16, TrainStep (forward, loss, backward, FusedAdam) on one fixed batch; the two models alternate in the same way.
    python tools/bench_tts_mt.py [--window 0.5] [--rounds 7] [--out profiles/tts_mt_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice100_amd import _native as N  # noqa: E402
from voice100_amd import functional as F_  # noqa: E402

B, V, L = 32, 71, 512
SB, SH, SL = 16, 512, 512


def stock(logits, target, target_len):
    ce = torch.nn.functional.cross_entropy(logits, target, reduction="none")
    mask = (torch.arange(target.shape[1], device=target.device)[None, :] < target_len[:, None]).to(ce.dtype)
    return torch.sum(ce * mask) / torch.sum(mask)


def fwd_bwd(fn, logits, target, target_len):
    logits.grad = None
    fn(logits, target, target_len).backward()
    return logits.grad


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


def alternate(arms, seconds, rounds, warm):
    for fn in arms.values():
        window(fn, warm)
    iters = {k: iters_for(fn, seconds) for k, fn in arms.items()}
    for k, fn in arms.items():                                       # one whole window per arm, discarded: the first one runs on cold clocks
        window(fn, iters[k])
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            times[k].append(window(fn, iters[k]))
    return {k: dict(summary(v), calls_per_window=iters[k]) for k, v in times.items()}


def count_launches(fn):
    """(device kernels of one call as torch.profiler sees them, or None; the library's own launches of that call)."""
    torch.cuda.synchronize()
    n0 = N.launch_count()
    fn()
    lib = N.launch_count() - n0
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                      and "memset" not in e.name.lower())
    except Exception as exc:                                         # a profiler that cannot start leaves the count unmeasured
        print(f"bench_tts_mt.py: kernel count not measured ({exc})", file=sys.stderr)
        kernels = None
    return kernels, lib


def rel_err(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-5))


def step_batch(gen, dev, phone):
    Tw = 2 * SL - 1
    f0 = torch.rand(SB, Tw, generator=gen) * 200
    f0 = torch.where(f0 < 60, torch.zeros(()), f0)
    f0_len = torch.randint(Tw // 2, Tw + 1, (SB,), generator=gen, dtype=torch.int32)
    f0_len[0] = Tw
    world = (f0.to(dev), f0_len.to(dev), (torch.randn(SB, Tw, 257, generator=gen) - 5).to(dev), (torch.randn(SB, Tw, 1, generator=gen) - 2).to(dev))
    text = (torch.randint(0, 29, (SB, SL), generator=gen).to(dev), torch.full((SB,), SL, dtype=torch.int32, device=dev))
    if not phone:
        return world, text
    phone_len = torch.randint(SL // 2, SL + 1, (SB,), generator=gen, dtype=torch.int32)
    return world, text, (torch.randint(0, V, (SB, SL), generator=gen).to(dev), phone_len.to(dev))


def write(out, path):
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(text + "\n")
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5, help="least seconds per timed window")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tts_mt_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tts_mt.py needs a GPU (a timing taken anywhere else says nothing)")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    logits = (torch.randn(B, V, L, generator=gen) * 2).to(dev).requires_grad_(True)
    target = torch.randint(0, V, (B, L), generator=gen).to(dev)
    target_len = torch.randint(L // 2, L + 1, (B,), generator=gen, dtype=torch.int32)
    target_len[0] = L
    target_len = target_len.to(dev)

    arms = {"fused": lambda: fwd_bwd(F_.masked_cross_entropy, logits, target, target_len),
            "stock": lambda: fwd_bwd(stock, logits, target, target_len)}
    with torch.no_grad():
        losses = {"fused": F_.masked_cross_entropy(logits, target, target_len), "stock": stock(logits, target, target_len)}
    grads = {k: fn().clone() for k, fn in arms.items()}
    equal = {"loss_rel_err": rel_err(losses["fused"], losses["stock"]), "dlogits_rel_err": rel_err(grads["fused"], grads["stock"])}
    if not all(e < 1e-4 for e in equal.values()):
        raise SystemExit(f"bench_tts_mt.py: the arms disagree at the timed shape: {equal}")

    res = alternate(arms, args.window, args.rounds, 20)
    noise = max(res["fused"]["spread"], res["stock"]["spread"])
    allowed = max(0.03, 3 * noise)
    k22 = {"shape": {"B": B, "V": V, "L": L, "counted_columns": int(target_len.sum())}, "outputs_at_timed_shape": equal, "arms": res,
           "stock_over_fused": round(res["stock"]["median_ms"] / res["fused"]["median_ms"], 3), "largest_spread_of_one_arm": noise,
           "allowed_slowdown": round(allowed, 4),
           "fused_not_slower_beyond_bar": bool(res["fused"]["median_ms"] <= res["stock"]["median_ms"] * (1 + allowed))}
    out = {"tool": "tools/bench_tts_mt.py", "device": torch.cuda.get_device_name(0),
           "method": f"windows of >= {args.window} s of back-to-back calls between device events, {args.rounds} alternating rounds",
           "masked_cross_entropy": k22}
    write(out, args.out)

    from voice100_amd.trainer import TrainStep
    from voice100_amd.tts import AlignTextToAudioModel, AlignTextToAudioMultiTaskModel
    torch.manual_seed(0)
    models = {"multi_task": AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=V, hidden_size=SH).to(dev),
              "align_text_to_audio": AlignTextToAudioModel(vocab_size=29, hidden_size=SH).to(dev)}
    for m in models.values():
        with torch.no_grad():
            m.norm.f0_mean.fill_(120.0); m.norm.f0_std.fill_(35.0); m.norm.logspc_mean.fill_(-5.0); m.norm.codeap_mean.fill_(-2.0)
    steps = {k: TrainStep(m, precision="bf16") for k, m in models.items()}
    batches = {"multi_task": step_batch(gen, dev, True), "align_text_to_audio": step_batch(gen, dev, False)}
    step_arms = {k: (lambda k=k: steps[k](batches[k])) for k in steps}
    sres = alternate(step_arms, args.window, args.rounds, 5)
    out["training_step"] = {"shape": {"hidden_size": SH, "B": SB, "L": SL, "frames": 2 * SL - 1, "logspc": 257, "target_vocab": V},
                            "precision": "bf16", "arms": sres,
                            "multi_task_over_align_text_to_audio": round(sres["multi_task"]["median_ms"] / sres["align_text_to_audio"]["median_ms"], 3),
                            "parameters": {k: sum(p.numel() for p in m.parameters()) for k, m in models.items()}}
    write(out, args.out)

    # launches: a pass of its own, after every timing (the profiler slows the host)
    for k, fn in arms.items():
        kernels, lib = count_launches(fn)
        res[k]["device_kernels_per_call"], res[k]["library_launches_per_call"] = kernels, lib
    for k, fn in step_arms.items():
        kernels, lib = count_launches(fn)
        sres[k]["device_kernels_per_step"], sres[k]["library_launches_per_step"] = kernels, lib
    print(write(out, args.out))


if __name__ == "__main__":
    main()
