"""The multi-task TTS model on the GPU: both reference fixtures through the HIP path, K22 (the phone head's masked cross-entropy,
csrc/phone_loss.hip) against float64 on the shapes where a lane-per-column kernel can go wrong, short training runs, one full-width
step, the TTS collate from waveforms and TTSPipeline's fourth value.  Tolerances are those of
tests/test_gpu_tts_features.py::test_align_text_to_audio_golden."""
import numpy as np
import pytest
import torch

from conftest import assert_grads_close, load_golden, rel_err, sub

pytestmark = pytest.mark.gpu


def _batch(g, dev):
    t = lambda k: torch.from_numpy(g[k]).to(dev)
    return ((t("target/f0"), t("target/f0_len"), t("target/logspc"), t("target/codeap")),
            (t("aligntext"), t("target/aligntext_len")), (t("target/phonetext"), t("target/phonetext_len")))


@pytest.mark.parametrize("name,use_mcep", [("tts_mt_tiny_logspc.npz", False), ("tts_mt_tiny_mcep.npz", True)])
def test_multi_task_golden(cuda, name, use_mcep):
    """Pins the branch gradient (two consumers of layer1's output), the k = 47 block and K22 together."""
    from voice100_amd.tts import AlignTextToAudioMultiTaskModel
    g = load_golden(name)
    m = AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=71, hidden_size=32, use_mcep=use_mcep)
    m.load_state_dict(sub(g, "state/"), strict=True)
    assert set(m.state_dict()) == {k[len("state/"):] for k in g if k.startswith("state/")}
    m = m.to(cuda).eval()
    at = torch.from_numpy(g["aligntext"]).to(cuda)
    with torch.no_grad():
        fwd = m(at)
    assert len(fwd) == 5
    for v, key in zip(fwd, ("hasf0_logits", "f0_hat", "logspc_hat", "codeap_hat", "target_logits")):
        assert v.shape == g["fwd/" + key].shape, key
        assert rel_err(v, g["fwd/" + key]) < 1e-4, key
    pred = m.predict(at)
    assert len(pred) == 4
    for v, key in zip(pred, ("f0", "logspc", "codeap", "logits")):
        assert v.shape == g["predict/" + key].shape, key
        assert rel_err(v, g["predict/" + key]) < 1e-4, key
    assert np.array_equal(pred[0].cpu().numpy() == 0, g["predict/f0"] == 0)          # F0 gate: exact
    m.train()
    losses = m._calc_batch_loss(_batch(g, cuda))
    assert len(losses) == 5
    assert np.allclose(np.array([float(v.detach()) for v in losses]), g["losses_train"], rtol=2e-4)
    sum(losses).backward()
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert set(grads) == {k[len("grad/"):] for k in g if k.startswith("grad/")}
    assert_grads_close(grads, {k: g["grad/" + k] for k in grads}, 2e-3)
    world, text, (phone, phone_len) = _batch(g, cuda)
    with pytest.raises(RuntimeError):
        m._calc_batch_loss((world, text, (phone[:, :-1].contiguous(), phone_len)))


# ---- K22 against float64 ---------------------------------------------------------------------------------------------------

def _k22_cases():
    """Every (V, L) pair once, B alternating, then the other B for the two vocabulary sizes the models use: 40 cases.  Each case
    carries its lengths (B = 3: one row of length 0, one of L, one of L + 5; B = 1: L, L + 5 or a length inside the row in turn),
    whether the logits are scaled by 1e4 and whether one row's targets are all -100."""
    Vs, Ls = (1, 2, 29, 64, 65, 71), (1, 63, 64, 65, 257)
    cases, n = [], 0
    for V in Vs:
        for L in Ls:
            cases.append((V, L, 1 + 2 * (n % 2), n))
            n += 1
    for V in (29, 71):
        for L in Ls:
            B = 3 if (cases[Vs.index(V) * len(Ls) + Ls.index(L)][2] == 1) else 1
            cases.append((V, L, B, n))
            n += 1
    return cases


def _k22_inputs(V, L, B, n):
    gen = torch.Generator().manual_seed(4000 + n)
    logits = torch.randn(B, V, L, generator=gen) * (1e4 if n % 3 == 0 else 2.0)
    target = torch.randint(0, V, (B, L), generator=gen)
    if B == 3:
        lens = [[0, L, L + 5], [L + 5, 0, L], [L, L + 5, 0]][n % 3]
    else:
        lens = [[L], [L + 5], [max(L - 3, 1)]][n % 3]
    full = max(range(B), key=lambda b: min(lens[b], L))
    if n % 2 == 0:
        target[full, 0] = -100                                        # one ignored target inside a counted row
    if n % 4 == 1 and B == 3:
        target[full] = -100                                           # a whole counted row of ignored targets
    return logits, target, torch.tensor(lens, dtype=torch.int32)


def _k22_reference(logits, target, lens, gout):
    x = logits.double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(x, target, reduction="none")
    mask = (torch.arange(target.shape[1])[None, :] < lens[:, None]).double()
    loss = (ce * mask).sum() / mask.sum()
    (loss * gout).backward()
    return loss.detach(), x.grad


@pytest.mark.parametrize("V,L,B,n", _k22_cases())
def test_masked_cross_entropy_vs_float64(cuda, V, L, B, n):
    from voice100_amd import functional as F_
    logits, target, lens = _k22_inputs(V, L, B, n)
    ref_loss, ref_grad = _k22_reference(logits, target, lens, 0.37)
    x = logits.to(cuda).requires_grad_(True)
    loss = F_.masked_cross_entropy(x, target.to(cuda), lens.to(cuda))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (loss * 0.37).backward()
    e_loss, e_grad = rel_err(loss, ref_loss), rel_err(x.grad, ref_grad)
    print(f"K22 V={V} L={L} B={B} lens={lens.tolist()} loss {float(loss.detach()):.6g} ref {float(ref_loss):.6g} rel_err {e_loss:.2e} grad {e_grad:.2e}")
    assert e_loss < 1e-4
    assert e_grad < 1e-4
    dead = torch.arange(L)[None, :] >= lens[:, None]                  # masked columns: exact zeros
    assert float(x.grad.cpu().transpose(1, 2)[dead].abs().sum()) == 0.0


def test_masked_cross_entropy_is_deterministic(cuda):
    from voice100_amd import _native as N
    logits, target, lens = _k22_inputs(71, 257, 3, 1)
    x, t, n = logits.to(cuda), target.to(cuda), lens.to(cuda)
    outs = []
    for _ in range(2):
        partial = torch.empty(N.helper("v100_masked_ce_parts", 3, 257), device=cuda)
        loss, unit = torch.empty(1, device=cuda), torch.empty_like(x)
        N.call("v100_masked_ce", x, t, n, partial, loss, unit, 3, 71, 257)
        outs.append((loss, unit))
    assert torch.equal(outs[0][0].view(torch.int32), outs[1][0].view(torch.int32))
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))


def test_masked_cross_entropy_checks_ids_before_launch(cuda, monkeypatch):
    from voice100_amd import _native as N
    from voice100_amd import functional as F_
    monkeypatch.setattr(F_, "CHECK_IDS", True)
    x = torch.randn(2, 29, 8, device=cuda)
    target = torch.randint(0, 29, (2, 8), device=cuda)
    lens = torch.tensor([8, 5], device=cuda)
    target[0, 1] = -100                                               # the ignore index is no out-of-range id
    assert torch.isfinite(F_.masked_cross_entropy(x, target, lens))
    target[1, 2] = 29
    before = N.launch_count()
    with pytest.raises(IndexError):
        F_.masked_cross_entropy(x, target, lens)
    assert N.launch_count() == before


# ---- the k = 47 block ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cin,B,T", [(64, 3, 133), (512, 16, 512), (256, 2, 640), (128, 2, 1023)])
def test_k47_block_act16_matches_fp32_storage(cuda, cin, B, T):
    """The decoder's second block is the one user of kernel size 47.  bf16 storage against fp32 storage (both with bf16 GEMM
    operands), as tests/test_gpu_act16.py::test_block_act16_wide_shapes compares the other sizes and with its bounds: an odd short
    row, the model's own shape (rows of 512: the kept-rows backward), rows of 513 ... 768 and rows past the streaming kernels."""
    from test_gpu_act16 import _wide_case
    from voice100_amd import _native as N
    assert N.helper("v100_dw_mfma_supported", 47, 1) == 1
    _wide_case(cuda, cin, 47, B, T)


def test_k47_block_fp32_vs_stock_ops(cuda):
    """One training-mode block with k = 47 at fp32 against the stock-op restatement on the CPU in float64: several time tiles
    (T = 300; the fixtures' rows are 40 long)."""
    from voice100_amd import _stock
    from voice100_amd.layers import InvertedResidual
    torch.manual_seed(47)
    blk = InvertedResidual(64, 64, kernel_size=47)
    gen = torch.Generator().manual_seed(48)
    x = torch.randn(2, 64, 300, generator=gen)
    gy = torch.randn(2, 64, 300, generator=gen)
    ref = InvertedResidual(64, 64, kernel_size=47).double()
    ref.load_state_dict(blk.state_dict())
    xr = x.double().requires_grad_(True)
    yr = _stock.inverted_residual(ref.train(), xr)
    (yr * gy.double()).sum().backward()
    blk = blk.to(cuda).train()
    xg = x.to(cuda).requires_grad_(True)
    y = blk(xg)
    (y * gy.to(cuda)).sum().backward()
    assert rel_err(y, yr) < 1e-4
    assert rel_err(xg.grad, xr.grad) < 2e-3
    assert_grads_close({k: p.grad for k, p in blk.named_parameters()}, {k: p.grad.numpy() for k, p in ref.named_parameters()}, 2e-3)


# ---- training --------------------------------------------------------------------------------------------------------------

def _random_batch(B, L, S, Vt, dev, gen):
    Tw = 2 * L - 1
    f0 = torch.rand(B, Tw, generator=gen) * 200
    f0 = torch.where(f0 < 60, torch.zeros(()), f0)
    f0_len = torch.randint(Tw // 2, Tw + 1, (B,), generator=gen, dtype=torch.int32)
    f0_len[0] = Tw
    at_len = torch.full((B,), L, dtype=torch.int32)
    phone_len = torch.randint(1, L + 1, (B,), generator=gen, dtype=torch.int32)
    return ((f0.to(dev), f0_len.to(dev), (torch.randn(B, Tw, S, generator=gen) - 5).to(dev), (torch.randn(B, Tw, 1, generator=gen) - 2).to(dev)),
            (torch.randint(0, 29, (B, L), generator=gen).to(dev), at_len.to(dev)),
            (torch.randint(0, Vt, (B, L), generator=gen).to(dev), phone_len.to(dev)))


def _set_norm(m):
    with torch.no_grad():
        m.norm.f0_mean.fill_(120.0); m.norm.f0_std.fill_(35.0)
        m.norm.logspc_mean.fill_(-5.0); m.norm.codeap_mean.fill_(-2.0); m.norm.codeap_std.fill_(1.5)


@pytest.mark.parametrize("precision", [32, "bf16"])
def test_training_reduces_loss(cuda, precision):
    """After test_gpu_models.py::test_training_loop_reduces_loss: 20 TrainStep steps on one fixed batch."""
    from voice100_amd import functional as F_
    from voice100_amd.trainer import TrainStep
    from voice100_amd.tts import AlignTextToAudioMultiTaskModel
    torch.manual_seed(0)
    try:
        m = AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=71, hidden_size=32, learning_rate=2e-3, use_mcep=True).to(cuda)
        _set_norm(m)
        step = TrainStep(m, precision=precision)
        batch = _random_batch(4, 48, 25, 71, cuda, torch.Generator().manual_seed(1))
        losses = [float(step(batch)) for _ in range(20)]
    finally:
        F_.set_matmul_precision("fp32")
    assert all(np.isfinite(l) for l in losses), losses
    assert losses[-1] < losses[0], losses
    if hasattr(m, "logged_metrics"):                                  # (the module shim keeps what was logged; Lightning sends it to its logger)
        assert {f"train_{n}loss" for n in ("", "hasf0_", "f0_", "logspc_", "codeap_", "phone_")} <= set(m.logged_metrics)


def test_full_width_step(cuda):
    """H = 512, B = 16, L = 512, Vt = 71 at bf16: one training step's loss and gradients, the five output shapes, and the batch
    independence of predict (as test_tts_config3_shape asserts for the v1 model)."""
    from voice100_amd import functional as F_
    from voice100_amd.tts import AlignTextToAudioMultiTaskModel
    torch.manual_seed(1234)
    B, L, Vt = 16, 512, 71
    m = AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=Vt, hidden_size=512).to(cuda)
    _set_norm(m)
    batch = _random_batch(B, L, 257, Vt, cuda, torch.Generator().manual_seed(2))
    F_.set_matmul_precision("bf16")
    try:
        m.train()
        losses = m._calc_batch_loss(batch)
        loss = sum(losses)
        loss.backward()
        assert len(losses) == 5 and all(bool(torch.isfinite(v)) for v in losses), [float(v.detach()) for v in losses]
        for k, p in m.named_parameters():
            if p.requires_grad:
                assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        m.eval()
        at = batch[1][0]
        with torch.no_grad():
            fwd = m(at)
        assert [tuple(v.shape) for v in fwd] == [(B, 2 * L - 1), (B, 2 * L - 1), (B, 2 * L - 1, 257), (B, 2 * L - 1, 1), (B, Vt, L)]
        f0, logspc, codeap, logits = m.predict(at)
        assert f0.shape == (B, 2 * L - 1) and logspc.shape == (B, 2 * L - 1, 257) and codeap.shape == (B, 2 * L - 1, 1) and logits.shape == (B, Vt, L)
        assert bool(torch.isfinite(logspc).all()) and bool(torch.isfinite(logits).all())
        _, logspc_b, _, logits_b = m.predict(at[3:5].contiguous())
        e1, e2 = rel_err(logspc_b, logspc[3:5]), rel_err(logits_b, logits[3:5])
        print(f"batch independence of predict: logspc {e1:.2e} phone logits {e2:.2e}")
        assert e1 < 1e-5 and e2 < 1e-5
    finally:
        F_.set_matmul_precision("fp32")


# ---- the collate from waveforms and the pipeline ---------------------------------------------------------------------------

def test_collate_from_waveforms(cuda):
    from voice100_amd.data import WorldAlignTextCollate
    from voice100_amd.tts import AlignTextToAudioMultiTaskModel
    from voice100_amd.vocoder import WORLDVocoder
    gen = torch.Generator().manual_seed(11)
    lens = (700, 2400, 4000)
    waves = [0.05 * torch.randn(n, generator=gen) + 0.4 * torch.sin(2 * np.pi * 140.0 * torch.arange(n) / 16000.0) for n in lens]
    L = 13                                                           # 2 L - 1 = 25 frames against frames(4000) = 26: adjust_size trims
    texts = [torch.randint(1, 29, (n,), generator=gen) for n in (4, 9, L)]
    phones = [torch.randint(1, 71, (n,), generator=gen) for n in (L, 6, 2)]
    v = WORLDVocoder()
    collate = WorldAlignTextCollate(v)
    two = collate(list(zip(waves, texts)))
    batch = collate(list(zip(waves, texts, phones)))
    assert len(two) == 2 and len(batch) == 3
    (f0, f0_len, spec, codeap), (text, text_len), (phone, phone_len) = batch
    T = v.frames(4000)
    assert f0.shape == (3, T) and spec.shape == (3, T, 257) and codeap.shape == (3, T, 1)
    assert (f0.dtype, spec.dtype, codeap.dtype, f0_len.dtype) == (torch.float32, torch.float32, torch.float32, torch.int32)
    assert f0_len.tolist() == [v.frames(n) for n in lens]
    assert text.shape == (3, L) and text.dtype == torch.int64 and text_len.tolist() == [4, 9, L] and text_len.dtype == torch.int32
    assert phone.shape == (3, L) and phone.dtype == torch.int64 and phone_len.tolist() == [L, 6, 2]
    assert all(t.is_cuda for t in (f0, f0_len, spec, codeap, text, text_len, phone, phone_len))
    block = torch.nn.utils.rnn.pad_sequence(waves, batch_first=True).to(cuda)
    rf0, rspec, rcodeap = v.encode_batch(block, torch.tensor(lens, dtype=torch.int32))
    for i, n in enumerate(f0_len.tolist()):
        assert torch.equal(f0[i, :n], rf0[i, :n]) and torch.equal(spec[i, :n], rspec[i, :n]) and torch.equal(codeap[i, :n], rcodeap[i, :n])
        assert not f0[i, n:].any() and not spec[i, n:].any() and not codeap[i, n:].any()
    for a, b in zip(two[0] + two[1], batch[0] + batch[1]):
        assert torch.equal(a, b)
    torch.manual_seed(3)
    m = AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=71, hidden_size=32).to(cuda).train()
    _set_norm(m)
    terms = m._calc_batch_loss(batch)
    assert len(terms) == 5 and all(bool(torch.isfinite(t)) for t in terms), [float(t.detach()) for t in terms]


def test_tts_pipeline_phone_logits(cuda):
    from voice100_amd.infer import TTSPipeline
    from voice100_amd.tts import AlignTextToAudioMultiTaskModel, TextToAlignTextModel
    from voice100_amd.vocoder import WORLDVocoder
    torch.manual_seed(4)
    al = TextToAlignTextModel(vocab_size=29, hidden_size=64).to(cuda).eval()
    with torch.no_grad():
        al.layers[4].bias.copy_(torch.tensor([0.6931, 1.3863], device=cuda))
    mt = AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=71, hidden_size=64, use_mcep=True).to(cuda).eval()
    with torch.no_grad():
        mt.norm.f0_mean.fill_(150.0); mt.norm.f0_std.fill_(30.0); mt.norm.codeap_mean.fill_(-12.0); mt.norm.codeap_std.fill_(3.0)
    v = WORLDVocoder(use_mcep=True).to(cuda)

    class ThreeValues:                                                # the same model behind the three-value interface
        def predict(self, aligntext):
            return mt.predict(aligntext)[:3]
    text = torch.randint(1, 29, (3, 20), device=cuda)
    text_len = torch.tensor([20, 11, 16], device=cuda)
    out = TTSPipeline(al, mt, v, synthesize=False)(text, text_len)
    ref = TTSPipeline(al, ThreeValues(), v, synthesize=False)(text, text_len)
    assert list(out) == list(ref) + ["phone_logits"]
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    B, La = out["aligntext"].shape
    f0, mcep, codeap, logits = mt.predict(out["aligntext"])
    assert out["phone_logits"].shape == (B, 71, La) and torch.equal(out["phone_logits"], logits)
    assert torch.equal(out["f0"], f0) and torch.equal(out["codeap"], codeap)
    assert torch.equal(out["logspc"], v.mcep_to_logspc(mcep.reshape(-1, 25)).reshape(B, -1, 257))
    full = TTSPipeline(al, mt, v)(text, text_len)                      # with the synthesis stage: the waveform keys beside the new one
    assert {"wave", "wave_len", "n_pulses", "phone_logits"} <= set(full) and bool(torch.isfinite(full["wave"]).all())
