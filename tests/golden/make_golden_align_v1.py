#!/usr/bin/env python3
"""Generate tests/golden/align_v1_tiny.npz by IMPORTING the reference's AudioAlignCTC (voice100/models/align.py) and CharTokenizer.

Run in the build container only (needs the reference checkout; see make_golden.py for the stubs):

    python tests/golden/make_golden_align_v1.py

Model: AudioAlignCTC(16, 29, 32, 2, 1e-3) under seed 20261019, `dense.weight` overwritten with randn * 2.0 (the default initialisation
leaves the log-probabilities so flat that the best path hangs on the last bits), LSTM dropout 0.  Batch: B = 4, T = 41, audio = randn,
audio_len = [41, 3, 28, 40], a [4, 7] text with text_len = [7, 1, 5, 7].  Written: parameters (param/*); train-mode logits, lengths,
CTC loss, every parameter gradient (grad/*) and the input gradient, augmentation bypassed; eval-mode logits; ctc_best_path's four
returns (best/*); the per-utterance scores and the `align` rows of voice100/align_text.py:49-51; the CharTokenizer vocabulary and the
three-part lines align_text.py:52-56 writes for the batch.  Only data is written -- no reference source.

Decisiveness, asserted here: the reference's `hist` does not change under 200 seeded Gaussian perturbations of the log-probabilities
with sigma = 1e-3 * max|logit| (ten times the project's 1e-4 parity bar), so an implementation within the bar must reproduce the
integer outputs exactly.  If the assertion fails, change the seed; do not loosen it.

Re-running reproduces the file bit for bit (fixed seeds, one thread, CPU float32, zip entries with a fixed date).
"""
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _install_stubs  # noqa: E402

SEED = 20261019
TRIALS = 200


def _save(path, out):
    """np.savez_compressed with a fixed date on every entry: the bytes depend on the arrays alone."""
    from numpy.lib import format as npformat
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in out.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            with z.open(info, "w", force_zip64=True) as f:
                npformat.write_array(f, np.asanyarray(v), allow_pickle=False)


def gen_align_v1_tiny():
    from voice100.models.align import AudioAlignCTC, ctc_best_path
    from voice100.text import CharTokenizer
    torch.manual_seed(SEED)
    model = AudioAlignCTC(16, 29, 32, 2, 1e-3)
    with torch.no_grad():
        model.dense.weight.copy_(torch.randn(model.dense.weight.shape) * 2.0)
    model.lstm.dropout = 0.0
    B, T = 4, 41
    audio = torch.randn(B, T, 16).requires_grad_(True)
    audio_len = torch.tensor([41, 3, 28, 40], dtype=torch.int64)
    text = torch.randint(1, 29, (B, 7), dtype=torch.int64)
    text_len = torch.tensor([7, 1, 5, 7], dtype=torch.int64)

    model.train()                                        # the augmentation is bypassed: forward + criterion, as _calc_batch_loss
    logits, logits_len = model(audio, audio_len)
    loss = model.criterion(torch.nn.functional.log_softmax(logits, dim=-1), text, logits_len, text_len)
    loss.backward()
    out = {"audio": audio.detach().numpy(), "audio_len": audio_len.numpy(), "text": text.numpy(), "text_len": text_len.numpy(),
           "logits": logits.detach().numpy(), "logits_len": logits_len.numpy(), "loss": loss.detach().numpy(),
           "grad_audio": audio.grad.numpy()}
    for k, v in model.state_dict().items():
        out["param/" + k] = v.numpy()
    for k, p in model.named_parameters():
        out["grad/" + k] = p.grad.numpy()

    model.eval()
    with torch.no_grad():
        logits_eval, eval_len = model(audio.detach(), audio_len)
        score, hist, path, best_len = model.ctc_best_path(audio.detach(), audio_len, text, text_len)
    assert torch.equal(eval_len, logits_len)
    out["logits_eval"] = logits_eval.numpy()
    out.update({"best/score": score.numpy(), "best/hist": hist.numpy(), "best/path": path.numpy(), "best/logits_len": best_len.numpy()})

    # the loop body of align_text.py:48-56, with the per-utterance scores ctc_best_path drops
    tokenizer = CharTokenizer()
    log_probs = torch.log_softmax(logits_eval, dim=-1)                   # [T_out, B, V]
    eff_len = torch.minimum(best_len, text_len)
    scores, lines = [], []
    align = np.zeros((B, 2 * text.shape[1] + 1), dtype=np.int32)
    for i in range(B):
        one_score, one_hist, _ = ctc_best_path(log_probs[:int(best_len[i]), i].numpy(), text[i, :int(eff_len[i])].numpy())
        assert np.array_equal(one_hist, hist[i, :int(best_len[i])].numpy())
        scores.append(float(one_score))
        row = [0] * (2 * int(text_len[i]) + 1)
        for j in hist[i, :best_len[i]]:
            row[j] += 1
        align[i, :len(row)] = row
        lines.append(tokenizer.decode(text[i, :text_len[i]]) + "|" + tokenizer.decode(path[i, :best_len[i]]) + "|"
                     + " ".join(str(x) for x in row))
    assert np.all(np.isfinite(scores))
    out["scores"] = np.asarray(scores, dtype=np.float32)
    out["align"] = align
    out["vocab"] = np.asarray(list(tokenizer._vocab))
    out["lines"] = np.asarray(lines)

    # decisiveness: hist is the same under perturbations ten times the parity bar
    sigma = 1e-3 * float(logits_eval.abs().max())
    flips = 0
    for trial in range(TRIALS):
        noise = np.random.RandomState(SEED + trial).standard_normal(tuple(log_probs.shape)).astype(np.float32)
        _, h, _, _ = model.ctc_best_path(audio_len=best_len, text=text, text_len=text_len, logits=log_probs + sigma * torch.from_numpy(noise))
        flips += int(not torch.equal(h, hist))
    assert flips == 0, f"{flips} of {TRIALS} perturbed runs changed hist: change SEED"
    _save(os.path.join(HERE, "align_v1_tiny.npz"), out)


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    _install_stubs()
    torch.set_num_threads(1)
    gen_align_v1_tiny()


if __name__ == "__main__":
    main()
