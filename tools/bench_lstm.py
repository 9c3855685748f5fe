#!/usr/bin/env python3
"""Time the HIP LSTM (K15) at the metric shape -- B = 32, T' = 512, H = 512, 2 layers, bidirectional -- against torch.nn.LSTM on the
same GPU, and the AudioToAlignText TrainStep (asr_en_base, B = 32 x 1024 frames, augmentation, Adam, gradient clipping 1.0).

Device-event timing after warm-up; one JSON object per line.  The HIP layer calls include their host work (weight layout, the give-up
word read after each recurrence).  us_per_step_layer = time / (layers x T').
    python tools/bench_lstm.py [--iters 10] [--warmup 3] [--train-steps 20]
"""
import argparse
import json
import os
import sys

import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice100_amd import functional as F_  # noqa: E402
from voice100_amd.lstm import LSTM  # noqa: E402

B, T, H, L = 32, 512, 512, 2


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train-steps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    ref = nn.LSTM(H, H, num_layers=L, bidirectional=True, dropout=0.2).to(dev)
    mine = LSTM(H, H, num_layers=L, bidirectional=True, dropout=0.2).to(dev)
    mine.load_state_dict(ref.state_dict())
    x_bct = torch.randn(B, H, T, device=dev)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    gy = torch.randn(B, 2 * H, T, device=dev)
    x_tbc = x_bct.permute(2, 0, 1).contiguous()
    gy_tbc = gy.permute(2, 0, 1).contiguous()
    from voice100_amd import _native as N
    for prec in ("fp32", "bf16"):
        F_.set_matmul_precision(prec)
        fmt = 1 if prec == "bf16" else 0
        for persistent in (True, False):
            F_.LSTM_PERSISTENT = persistent
            ran_persistent = persistent and all(N.helper("v100_lstm_persistent_ok", B, H, 2, fmt, bwd) for bwd in (0, 1))

            def fwd():
                with torch.no_grad():
                    mine.eval()
                    mine.forward_bct(x_bct, lens)

            def fwd_bwd():
                mine.train()
                x = x_bct.clone().requires_grad_(True)
                y, _, _ = mine.forward_bct(x, lens)
                y.backward(gy)
            for what, fn in (("eval_forward", fwd), ("forward_backward", fwd_bwd)):
                ms = timed(fn, args.iters, args.warmup)
                emit(impl="voice100_amd.LSTM", precision=prec, form="persistent" if ran_persistent else "step", what=what,
                     ms=round(ms, 3), us_per_step_layer=round(1000 * ms / (L * T), 2), B=B, T=T, H=H, layers=L)
    F_.set_matmul_precision("fp32")
    F_.LSTM_PERSISTENT = True
    for prec, ac in (("fp32", False), ("fp16-autocast", True)):
        def rfwd():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                ref.eval()
                ref(x_tbc)

        def rfwd_bwd():
            ref.train()
            x = x_tbc.clone().requires_grad_(True)
            with torch.autocast("cuda", dtype=torch.float16, enabled=ac):
                y, _ = ref(x)
            y.float().backward(gy_tbc)
        for what, fn in (("eval_forward", rfwd), ("forward_backward", rfwd_bwd)):
            ms = timed(fn, args.iters, args.warmup)
            emit(impl="torch.nn.LSTM", precision=prec, what=what, ms=round(ms, 3), us_per_step_layer=round(1000 * ms / (L * T), 2),
                 B=B, T=T, H=H, layers=L)

    from voice100_amd.asr import AudioToAlignText
    from voice100_amd.trainer import TrainStep
    torch.manual_seed(1)
    model = AudioToAlignText(64, [[512, False, 5, 2, 2, False], [512, False, 5, 1, 2, False]], 2, 512, 29).to(dev)
    audio = torch.randn(B, 1024, 64, device=dev) - 4
    audio_len = torch.full((B,), 1024, device=dev)
    text = torch.randint(1, 29, (B, 120), device=dev)
    text_len = torch.full((B,), 120, device=dev)
    step = TrainStep(model, precision="bf16", gradient_clip_val=1.0)
    batch = ((audio, audio_len), (text, text_len))
    ms = timed(lambda: step(batch), args.train_steps, args.warmup)
    emit(impl="AudioToAlignText TrainStep", precision="bf16", what="train_step", ms_per_step=round(ms, 3), B=B, frames=1024,
         gradient_clip_val=1.0, frames_per_s=round(B * 1024 / (ms / 1000)))
    F_.set_matmul_precision("fp32")


if __name__ == "__main__":
    main()
