#!/usr/bin/env python3
"""Generate tests/golden/tts_v2_tiny.npz and tts_v2_tiny_s257.npz by IMPORTING the reference's v2 TTS models
(voice100/models/_align_v2.py TextToAlignText, voice100/models/_tts_v2.py AlignTextToAudio).

Run in the build container only (needs the reference checkout; see make_golden.py for the stubs):

    python tests/golden/make_golden_tts_v2.py

TextToAlignText (align/*, in tts_v2_tiny.npz): H = 32, 2 layers, bidirectional, B = 3 with text_len (7, 1, 4), train mode with the
LSTM's dropout set to 0.  Written: parameters, text, forward output and lengths, predict, the loss and every parameter gradient, and
align() on crafted (gap, length) arrays (alignfn/*) with negative gaps and lengths below 1 that stay inside the row.

AlignTextToAudio (audio/*): H = 32, decoder width 32 with the tts_en_base settings, B = 3, aligntext_len (6, 1, 4) (2T - 1 = 11
frames), WORLDNorm set to random statistics, raw targets with f0 straddling 30 and codeap straddling -0.2, ragged f0_len.
logspc_size 25 with Tt = 14 > 11 in tts_v2_tiny.npz, logspc_size 257 with Tt = 9 < 11 in tts_v2_tiny_s257.npz.  Written:
parameters, inputs, the five forward outputs, the five loss terms, the total loss, every parameter gradient, and predict().

Parameters and inputs are rounded to bf16-representable float32 values (still float32) so the files compress below the size limit.
Only data is written -- no reference source.  Re-running reproduces the files bit for bit (fixed seeds, CPU float32).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _install_stubs  # noqa: E402

DECODER = [[32, False, 5, 1, 2, False], [32, True, 5, 2, 2, False], [32, False, 5, 1, 2, False]]

# (gap, length) rows for align(); the sum minus the first gap stays > 1e-3 away from an integer
ALIGN_CASES = [
    [[0.0, 1.5], [0.3, 0.2], [-0.5, 2.7], [1.25, 0.05]],
    [[2.2, 3.1], [0.0, 0.0], [0.4, 4.9], [-0.9, 0.6], [0.7, 1.1], [3.3, 2.05]],
    [[0.1, 0.4]],
    [[-0.6, 0.9], [-0.2, 0.3], [2.6, -0.4], [0.0, 5.55]],
    [[1.0, 2.0], [1.0, 2.0], [0.5, 0.5], [0.25, 0.75], [0.125, 0.3]],
]


def _bf16_round_(module):
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(p.to(torch.bfloat16).to(torch.float32))


def _r(x):
    return x.to(torch.bfloat16).to(torch.float32)


def gen_align(out):
    from voice100.models._align_v2 import TextToAlignText
    torch.manual_seed(20261016)
    model = TextToAlignText(vocab_size=29, num_layers=2, hidden_size=32, num_outputs=2, learning_rate=1e-3)
    _bf16_round_(model)
    model.lstm.dropout = 0.0
    model.train()
    B, L = 3, 7
    text_len = torch.tensor([7, 1, 4], dtype=torch.int64)
    text = torch.randint(1, 29, (B, L), dtype=torch.int64) * (torch.arange(L)[None, :] < text_len[:, None])
    align = torch.randint(0, 12, (B, 2 * L + 1), dtype=torch.int64) * (torch.arange(2 * L + 1)[None, :] < 2 * text_len[:, None] + 1)
    align_len = 2 * text_len + 1
    pred, pred_len = model(text, text_len)
    loss = model._calc_batch_loss(((text, text_len), (align, align_len)))
    loss.backward()
    with torch.no_grad():
        p_align, p_len = model.predict(text, text_len)
    out.update({"align/text": text.numpy(), "align/text_len": text_len.numpy(), "align/align": align.numpy(),
                "align/pred": pred.detach().numpy(), "align/pred_len": pred_len.numpy(), "align/loss": loss.detach().numpy(),
                "align/predict": p_align.numpy(), "align/predict_len": p_len.numpy()})
    for k, v in model.state_dict().items():
        out["align/param/" + k] = v.numpy()
    for k, p in model.named_parameters():
        out["align/grad/" + k] = p.grad.numpy()
    g = torch.Generator().manual_seed(5)
    for i, rows in enumerate(ALIGN_CASES):
        a = torch.tensor(rows, dtype=torch.float32)
        frac = float(torch.sum(a) - a[0, 0]) % 1.0
        assert 1e-3 < frac < 1 - 1e-3, (i, frac)
        t = torch.randint(1, 29, (a.shape[0],), generator=g, dtype=torch.int64)
        out[f"alignfn/{i}/text"] = t.numpy()
        out[f"alignfn/{i}/align"] = a.numpy()
        out[f"alignfn/{i}/out"] = model.align(t, a).numpy()


def gen_audio(out, S, Tt, seed):
    from voice100.models._tts_v2 import AlignTextToAudio
    torch.manual_seed(seed)
    model = AlignTextToAudio(vocab_size=29, logspc_size=S, codeap_size=1, encoder_num_layers=2, encoder_hidden_size=32,
                             decoder_settings=DECODER)
    n = model.norm
    with torch.no_grad():
        n.f0_mean.copy_(_r(torch.tensor([150.0]) + torch.randn(1) * 10))
        n.f0_std.copy_(_r(torch.tensor([60.0]) + torch.rand(1) * 20))
        n.logspc_mean.copy_(_r(torch.randn(S) * 2 - 3))
        n.logspc_std.copy_(_r(torch.rand(S) + 0.5))
        n.codeap_mean.copy_(_r(torch.randn(1) * 0.3 - 0.5))
        n.codeap_std.copy_(_r(torch.rand(1) * 0.5 + 0.5))
    _bf16_round_(model)
    model.lstm.dropout = 0.0
    model.train()
    B, L = 3, 6
    at_len = torch.tensor([6, 1, 4], dtype=torch.int64)
    aligntext = torch.randint(0, 29, (B, L), dtype=torch.int64) * (torch.arange(L)[None, :] < at_len[:, None])
    f0 = _r(torch.where(torch.rand(B, Tt) < 0.3, torch.zeros(B, Tt), torch.rand(B, Tt) * 260.0))
    f0[0, :4] = torch.tensor([29.5, 30.0, 30.5, 0.0])
    logspc = _r(torch.randn(B, Tt, S) * 2 - 3)
    codeap = _r(torch.randn(B, Tt, 1) * 0.3 - 0.2)
    f0_len = torch.tensor([Tt, 3, 2 * 4], dtype=torch.int64)
    outs = model(aligntext, at_len)
    terms = model._calc_batch_loss(((f0, f0_len, logspc, codeap), (aligntext, at_len)))
    loss = terms[0] + terms[1] + terms[2] * model.logspc_weight + terms[3] + terms[4]
    loss.backward()
    model.eval()
    with torch.no_grad():
        pf0, plog, pcap = model.predict(aligntext, at_len)
    p = f"audio{S}/"
    out.update({p + "aligntext": aligntext.numpy(), p + "aligntext_len": at_len.numpy(), p + "f0": f0.numpy(),
                p + "f0_len": f0_len.numpy(), p + "logspc": logspc.numpy(), p + "codeap": codeap.numpy(),
                p + "terms": torch.stack([t.detach() for t in terms]).numpy(), p + "loss": loss.detach().numpy(),
                p + "predict/f0": pf0.numpy(), p + "predict/logspc": plog.numpy(), p + "predict/codeap": pcap.numpy()})
    for name, v in zip(("hasf0_logits", "f0_hat", "logspc_hat", "hascodeap_logits", "codeap_hat"), outs):
        out[p + "out/" + name] = v.detach().numpy()
    for k, v in model.state_dict().items():
        out[p + "param/" + k] = v.numpy()
    for k, q in model.named_parameters():
        if q.grad is not None:
            out[p + "grad/" + k] = q.grad.numpy()


def main():
    sys.path.insert(0, REF)
    _install_stubs()
    torch.set_num_threads(1)
    out = {}
    gen_align(out)
    gen_audio(out, 25, 14, 20261017)
    np.savez_compressed(os.path.join(HERE, "tts_v2_tiny.npz"), **out)
    out = {}
    gen_audio(out, 257, 9, 20261018)
    np.savez_compressed(os.path.join(HERE, "tts_v2_tiny_s257.npz"), **out)
    for f in ("tts_v2_tiny.npz", "tts_v2_tiny_s257.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)))


if __name__ == "__main__":
    main()
