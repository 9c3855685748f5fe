#!/usr/bin/env python3
"""Generate tests/golden/asr_v2_tiny.npz by IMPORTING the reference's AudioToAlignText (voice100/models/_asr_v2.py).

Run in the build container only (needs the reference checkout; see make_golden.py for the stubs):

    python tests/golden/make_golden_lstm.py

Tiny widths (encoder 32 channels, LSTM H = 32, 2 layers, bidirectional), B = 3 with ragged lengths including 1, train mode with
the LSTM's dropout set to 0 and the augmentation bypassed.  Written: parameters (param/*), inputs, logits, lengths, the CTC loss and
every parameter gradient (grad/*) plus the input gradient, and ctc_best_path's (score, hist, path, logits_len) (best/*).  Only data is written -- no reference source.  Re-running reproduces the
file bit for bit (fixed seeds, CPU float32, zip entries without timestamps).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _install_stubs  # noqa: E402

SETTINGS = [[32, False, 5, 2, 2, False], [32, False, 5, 1, 2, False]]


def gen_asr_v2_tiny():
    from voice100.models._asr_v2 import AudioToAlignText
    torch.manual_seed(20261015)
    model = AudioToAlignText(audio_size=16, encoder_settings=SETTINGS, decoder_num_layers=2, decoder_hidden_size=32, vocab_size=29)
    model.lstm.dropout = 0.0
    model.train()
    B, T = 3, 23
    audio = (torch.randn(B, T, 16) * 1.5 - 2.0).requires_grad_(True)
    audio_len = torch.tensor([23, 1, 14], dtype=torch.int64)
    text = torch.randint(1, 29, (B, 5), dtype=torch.int64)
    text_len = torch.tensor([5, 1, 3], dtype=torch.int64)
    logits, logits_len = model(audio, audio_len)
    log_probs = torch.nn.functional.log_softmax(logits, dim=-1)
    loss = model.criterion(log_probs, text, logits_len, text_len)
    loss.backward()
    out = {"audio": audio.detach().numpy(), "audio_len": audio_len.numpy(), "text": text.numpy(), "text_len": text_len.numpy(),
           "logits": logits.detach().numpy(), "logits_len": logits_len.numpy(), "loss": loss.detach().numpy(),
           "grad_audio": audio.grad.numpy()}
    score, hist, path, best_len = model.ctc_best_path(audio.detach(), audio_len, text, text_len)
    out.update({"best/score": score.numpy(), "best/hist": hist.numpy(), "best/path": path.numpy(), "best/logits_len": best_len.numpy()})
    for k, v in model.state_dict().items():
        out["param/" + k] = v.numpy()
    for k, p in model.named_parameters():
        out["grad/" + k] = p.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "asr_v2_tiny.npz"), **out)


def main():
    sys.path.insert(0, REF)
    _install_stubs()
    torch.set_num_threads(1)
    gen_asr_v2_tiny()


if __name__ == "__main__":
    main()
