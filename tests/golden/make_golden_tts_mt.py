#!/usr/bin/env python3
"""Generate tests/golden/tts_mt_tiny_logspc.npz and tts_mt_tiny_mcep.npz by IMPORTING the reference's multi-task TTS model
(voice100/models/tts.py AlignTextToAudioMultiTaskModel with its VoiceMultiTaskDecoder).

Run in the build container only (needs the reference checkout; see make_golden.py for the stubs):

    python tests/golden/make_golden_tts_mt.py

The reference's constructor passes `use_logspc_weights=` to a WORLDLoss whose argument is called `use_mel_weights` and so raises
TypeError.  At run time the name WORLDLoss in the imported module's namespace is replaced by a wrapper that maps the one keyword;
nothing else of the reference is touched and none of its text is copied.  Only data is written.

Model: vocab_size 29, target_vocab_size 71, hidden_size 32, BatchNorm randomised and WORLDNorm set as make_golden.gen_tts_tiny does
(with identity statistics the f0 term is ~1e4 and drowns the others).  Inputs: B = 2, L = 40; targets as in gen_tts_tiny (Tw = 2L + 3
frames, f0 below 60 zeroed, f0_len = (Tw, Tw - 11)); phonetext uniform in [0, 71) with phonetext_len = (L - 2, 3), so the phone mask
differs from the frame mask.  Written: state/*, the five eval-mode forward outputs, the four predict outputs, the five train-mode
loss terms and every parameter gradient of their sum.

Parameters and inputs are rounded to bf16-representable float32 values (still float32) so the files compress below the size limit.
Re-running reproduces the files bit for bit (fixed seeds, CPU float32, one thread).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _install_stubs, _randomize_bn  # noqa: E402


def _r(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _bf16_round_(module):
    with torch.no_grad():
        for t in list(module.parameters()) + [b for b in module.buffers() if b.dtype.is_floating_point]:
            t.copy_(_r(t))


def _patch_world_loss(tts):
    ref_loss = tts.WORLDLoss

    def world_loss(*args, use_logspc_weights=False, **kw):
        return ref_loss(*args, use_mel_weights=use_logspc_weights, **kw)
    tts.WORLDLoss = world_loss


def gen(use_mcep, gen):
    from voice100.models import tts
    torch.manual_seed(1234)
    m = tts.AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=71, hidden_size=32, learning_rate=1e-3, use_mcep=use_mcep)
    _randomize_bn(m, gen)
    with torch.no_grad():
        m.norm.f0_mean.fill_(120.0); m.norm.f0_std.fill_(35.0)
        m.norm.logspc_mean.copy_(torch.randn(m.norm.logspc_mean.shape, generator=gen) - 5)
        m.norm.logspc_std.copy_(torch.rand(m.norm.logspc_std.shape, generator=gen) + 0.5)
        m.norm.codeap_mean.fill_(-2.0); m.norm.codeap_std.fill_(1.5)
    _bf16_round_(m)
    B, L = 2, 40
    aligntext = torch.randint(0, 29, (B, L), generator=gen)
    out = {"aligntext": aligntext.numpy()}
    for k, v in m.state_dict().items():
        out["state/" + k] = v.numpy().copy()
    m.eval()
    with torch.no_grad():
        fwd = m(aligntext)
        pred = m.predict(aligntext)
    for name, v in zip(("hasf0_logits", "f0_hat", "logspc_hat", "codeap_hat", "target_logits"), fwd):
        out["fwd/" + name] = v.numpy()
    for name, v in zip(("f0", "logspc", "codeap", "logits"), pred):
        out["predict/" + name] = v.numpy()
    Tw = 2 * L + 3
    f0 = torch.rand(B, Tw, generator=gen) * 200
    f0 = _r(torch.where(f0 < 60, torch.zeros(()), f0))
    f0_len = torch.tensor([Tw, Tw - 11], dtype=torch.int32)
    logspc = _r(torch.randn(B, Tw, m.logspc_size, generator=gen) - 5)
    codeap = _r(torch.randn(B, Tw, 1, generator=gen) - 2)
    aligntext_len = torch.tensor([L, L - 5], dtype=torch.int32)
    phonetext = torch.randint(0, 71, (B, L), generator=gen)
    phonetext_len = torch.tensor([L - 2, 3], dtype=torch.int32)
    m.train()
    losses = m._calc_batch_loss(((f0, f0_len, logspc, codeap), (aligntext, aligntext_len), (phonetext, phonetext_len)))
    assert len(losses) == 5
    sum(losses).backward()
    out["target/f0"] = f0.numpy(); out["target/f0_len"] = f0_len.numpy()
    out["target/logspc"] = logspc.numpy(); out["target/codeap"] = codeap.numpy()
    out["target/aligntext_len"] = aligntext_len.numpy()
    out["target/phonetext"] = phonetext.numpy(); out["target/phonetext_len"] = phonetext_len.numpy()
    out["losses_train"] = np.array([float(v.detach()) for v in losses], dtype=np.float32)
    for key, p in m.named_parameters():
        if p.grad is not None:
            out["grad/" + key] = p.grad.numpy()
    return out


def main():
    sys.path.insert(0, REF)
    sys.dont_write_bytecode = True
    _install_stubs()
    torch.set_num_threads(1)
    from voice100.models import tts
    _patch_world_loss(tts)
    g = torch.Generator().manual_seed(22)
    for use_mcep in (False, True):
        name = f"tts_mt_tiny_{'mcep' if use_mcep else 'logspc'}.npz"
        np.savez_compressed(os.path.join(HERE, name), **gen(use_mcep, g))
        print(name, os.path.getsize(os.path.join(HERE, name)))


if __name__ == "__main__":
    main()
