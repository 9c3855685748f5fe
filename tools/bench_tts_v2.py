#!/usr/bin/env python3
"""Time the v2 TTS models' training steps at the recipes' batch of 128 and the new loss kernels, against a stock-PyTorch
restatement on the same GPU.

  align_en_base: TextToAlignText(29, 2, 256), text L <= 160 (ragged), TrainStep with Adam and gradient clipping 1.0
  tts_en_base:   AlignTextToAudio(29, 25, 1, 2, 512, base decoder), aligned text L <= 400 (ragged), Tt = 2 L, same step
  stock:         the same model as nn.Embedding -> nn.LSTM (MIOpen) on packed sequences -> nn.Conv1d / ConvTranspose1d + LayerNorm +
                 GELU -> nn.Linear, the loss in torch ops, torch.optim.Adam + clip_grad_norm_ (fp32, or bf16 autocast)
  kernels:       K16 (v2 WORLD loss + its backward) and K17 (align loss + backward) alone, with the bytes they must move and that
                 traffic's share of 8 TB/s

Device-event timing after warm-up; one JSON object per line, also appended to --out.
    python tools/bench_tts_v2.py [--steps 10] [--warmup 3] [--out profiles/tts_v2_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from voice100_amd import functional as F_  # noqa: E402
from voice100_amd.trainer import TrainStep  # noqa: E402
from voice100_amd.tts_v2 import AlignTextToAudio, TextToAlignText  # noqa: E402

BASE_DECODER = [[512, False, 5, 1, 2, False], [512, True, 5, 2, 2, False], [512, False, 5, 1, 2, False]]
OUT = []


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
    OUT.append(kw)
    print(json.dumps(kw), flush=True)


def align_batch(dev, B=128, L=160):
    g = torch.Generator().manual_seed(1)
    text_len = torch.randint(L // 4, L + 1, (B,), generator=g)
    text_len[0] = L
    text = torch.randint(1, 29, (B, L), generator=g) * (torch.arange(L)[None, :] < text_len[:, None])
    align = torch.randint(0, 12, (B, 2 * L + 1), generator=g) * (torch.arange(2 * L + 1)[None, :] < 2 * text_len[:, None] + 1)
    return ((text.to(dev), text_len.to(dev)), (align.to(dev), (2 * text_len + 1).to(dev)))


def tts_batch(dev, B=128, L=400, S=25):
    g = torch.Generator().manual_seed(2)
    at_len = torch.randint(L // 4, L + 1, (B,), generator=g)
    at_len[0] = L
    at = torch.randint(1, 29, (B, L), generator=g) * (torch.arange(L)[None, :] < at_len[:, None])
    Tt = 2 * L
    f0 = torch.where(torch.rand(B, Tt, generator=g) < 0.3, torch.zeros(B, Tt), 80 + torch.rand(B, Tt, generator=g) * 150)
    logspc = torch.randn(B, Tt, S, generator=g) * 2 - 3
    codeap = torch.randn(B, Tt, 1, generator=g) * 0.3 - 0.2
    return ((f0.to(dev), (2 * at_len).to(dev), logspc.to(dev), codeap.to(dev)), (at.to(dev), at_len.to(dev)))


# ---- the stock-PyTorch restatement (the yardstick) ----------------------------------------------------------------------------

class StockAlign(nn.Module):
    def __init__(self, H=256):
        super().__init__()
        self.embedding = nn.Embedding(29, H)
        self.lstm = nn.LSTM(H, H, num_layers=2, dropout=0.2, bidirectional=True, batch_first=True)
        self.dense = nn.Linear(2 * H, 2)

    def loss(self, batch):
        (text, text_len), (align, _) = batch
        packed = pack_padded_sequence(self.embedding(text), text_len.cpu(), batch_first=True, enforce_sorted=False)
        out, _ = pad_packed_sequence(self.lstm(packed)[0], batch_first=True)
        pred = self.dense(out)
        al = align[:, :-1].reshape(align.shape[0], -1, 2)
        per = torch.mean(torch.abs(torch.log((al + 1).to(pred.dtype)) - pred), dim=2)
        mask = (torch.arange(text.shape[1], device=text.device)[None, :] < text_len[:, None]).to(pred.dtype)
        return torch.sum(per * mask) / torch.sum(mask)


class StockBlock(nn.Module):
    def __init__(self, cin, cout, transpose):
        super().__init__()
        self.layer_norm = nn.LayerNorm(cout)
        self.conv = (nn.ConvTranspose1d if transpose else nn.Conv1d)(cin, cout, 5, stride=2 if transpose else 1, padding=2, bias=False)

    def forward(self, x):
        return F.gelu(self.layer_norm(self.conv(x).transpose(-2, -1)).transpose(-2, -1))


class StockTTS(nn.Module):
    def __init__(self, H=512, S=25):
        super().__init__()
        self.S = S
        self.embedding = nn.Embedding(29, H)
        self.lstm = nn.LSTM(H, H, num_layers=2, dropout=0.2, bidirectional=True)
        self.decoder = nn.Sequential(StockBlock(2 * H, 512, False), StockBlock(512, 512, True), StockBlock(512, 512, False))
        self.projection = nn.Linear(512, 2 + S + 2)

    def loss(self, batch):
        (f0, f0_len, logspc, codeap), (at, at_len) = batch
        hasf0, hascodeap = (f0 >= 30).float(), (codeap < -0.2).float()
        packed = pack_padded_sequence(self.embedding(at), at_len.cpu(), batch_first=True, enforce_sorted=False)
        out, _ = pad_packed_sequence(self.lstm(packed)[0], batch_first=True)
        x = self.projection(self.decoder(out.transpose(-2, -1)).transpose(-2, -1)).float()
        n = min(x.shape[1], f0.shape[1])
        x, hasf0, hascodeap, f0, logspc, codeap = x[:, :n], hasf0[:, :n], hascodeap[:, :n], f0[:, :n], logspc[:, :n], codeap[:, :n]
        mask = (torch.arange(n, device=x.device)[None, :] < f0_len[:, None]).float()
        S = self.S
        h = F.binary_cross_entropy_with_logits(x[:, :, 0], hasf0, reduction="none") * mask
        f = (x[:, :, 1] - f0) ** 2 * hasf0 * mask
        ls = torch.mean((x[:, :, 2:2 + S] - logspc) ** 2, dim=2) * mask
        hc = torch.mean(F.binary_cross_entropy_with_logits(x[:, :, 2 + S:3 + S], hascodeap, reduction="none"), dim=2) * mask
        c = torch.mean((x[:, :, 3 + S:] - codeap) ** 2 * hascodeap, dim=2) * mask
        ms = torch.sum(mask)
        return (h.sum() + f.sum() + 5 * ls.sum() + hc.sum() + c.sum()) / ms


def stock_step(model, batch, bf16):
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=bf16):
            loss = model.loss(batch)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "tts_v2_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gpu = torch.cuda.get_device_name(0)

    ab = align_batch(dev)
    tb = tts_batch(dev)
    for precision in ("fp32", "bf16"):
        torch.manual_seed(0)
        m = TextToAlignText(29, 2, 256, 2, 1e-3).to(dev)
        step = TrainStep(m, precision=32 if precision == "fp32" else "bf16", gradient_clip_val=1.0)
        ms = timed(lambda: step(ab), args.steps, args.warmup)
        emit(what="trainstep", model="align_en_base", impl="hip", precision=precision, B=128, L=160, ms_per_step=round(ms, 3), gpu=gpu)
        F_.set_matmul_precision("fp32")
        torch.manual_seed(0)
        s = StockAlign().to(dev)
        ms = timed(stock_step(s, ab, precision == "bf16"), args.steps, args.warmup)
        emit(what="trainstep", model="align_en_base", impl="stock", precision=precision, B=128, L=160, ms_per_step=round(ms, 3), gpu=gpu)
        del m, step, s
    for precision in ("fp32", "bf16"):
        torch.manual_seed(0)
        m = AlignTextToAudio(29, 25, 1, 2, 512, BASE_DECODER).to(dev)
        step = TrainStep(m, precision=32 if precision == "fp32" else "bf16", gradient_clip_val=1.0)
        ms = timed(lambda: step(tb), args.steps, args.warmup)
        emit(what="trainstep", model="tts_en_base", impl="hip", precision=precision, B=128, L=400, Tt=800, ms_per_step=round(ms, 3),
             gpu=gpu)
        F_.set_matmul_precision("fp32")
        torch.manual_seed(0)
        s = StockTTS().to(dev)
        ms = timed(stock_step(s, tb, precision == "bf16"), args.steps, args.warmup)
        emit(what="trainstep", model="tts_en_base", impl="stock", precision=precision, B=128, L=400, Tt=800, ms_per_step=round(ms, 3),
             gpu=gpu)
        del m, step, s
        torch.cuda.empty_cache()

    # the loss kernels alone, forward + backward, at the tts_en_base / align_en_base step shapes
    (f0, f0_len, logspc, codeap), (at, at_len) = tb
    B, Tt, S = logspc.shape
    Tp = 2 * 400 - 1
    pred = torch.randn(B, Tp, 2 + S + 2, device=dev, requires_grad=True)
    norm = [torch.zeros(1, device=dev), torch.ones(1, device=dev), torch.zeros(S, device=dev), torch.ones(S, device=dev),
            torch.zeros(1, device=dev), torch.ones(1, device=dev)]
    gout = torch.ones(5, device=dev)

    def k16():
        out = F_.world_loss_v2(pred, f0_len, f0, logspc, codeap, norm)
        torch.autograd.backward(out, gout)
    A = 2 + S + 2
    n = min(Tp, Tt)
    # pred read, unit written (fwd); unit read, dpred written (bwd); the targets read once
    nbytes = 4 * (B * Tp * A * 4 + B * n * (1 + S + 1))
    ms = timed(k16, 50, 5)
    emit(what="kernel", name="K16 world_loss_v2 fwd+bwd", B=B, Tp=Tp, Tt=Tt, S=S, ms=round(ms, 4), bytes=nbytes,
         frac_of_8TBps=round(nbytes / (ms * 1e-3) / 8e12, 4), gpu=gpu)
    (text, text_len), (align, _) = ab
    L = text.shape[1]
    ap_ = torch.randn(128, L, 2, device=dev, requires_grad=True)

    def k17():
        F_.align_loss(ap_, align, text_len).backward()
    nbytes = 128 * L * 2 * (4 * 4 + 8)
    ms = timed(k17, 50, 5)
    emit(what="kernel", name="K17 align_loss fwd+bwd", B=128, L=L, ms=round(ms, 4), bytes=nbytes,
         frac_of_8TBps=round(nbytes / (ms * 1e-3) / 8e12, 4), gpu=gpu)

    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "a") as f:
        for r in OUT:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
