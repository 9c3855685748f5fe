"""CPU-side checks of the multi-task TTS model (AlignTextToAudioMultiTaskModel, VoiceMultiTaskDecoder), the phone head's masked
cross-entropy, the TTS collate and TTSPipeline's fourth value.  The fixtures are made from the reference
(tests/golden/make_golden_tts_mt.py); on CPU tensors the model runs its stock-op restatement, so value parity is checked here too.
Tolerances are those of tests/test_gpu_tts_features.py::test_align_text_to_audio_golden."""
import argparse

import numpy as np
import pytest
import torch

from conftest import assert_grads_close, load_golden, rel_err, sub
from voice100_amd import functional as F_
from voice100_amd.tts import AlignTextToAudioMultiTaskModel, VoiceMultiTaskDecoder

FIXTURES = [("tts_mt_tiny_logspc.npz", False), ("tts_mt_tiny_mcep.npz", True)]


@pytest.fixture(scope="module", params=FIXTURES, ids=["logspc", "mcep"])
def golden(request):
    name, use_mcep = request.param
    return load_golden(name), use_mcep


def _model(g, use_mcep):
    m = AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=71, hidden_size=32, use_mcep=use_mcep)
    m.load_state_dict(sub(g, "state/"), strict=True)
    return m


def _batch(g, to=lambda t: t):
    t = lambda k: to(torch.from_numpy(g[k]))
    return ((t("target/f0"), t("target/f0_len"), t("target/logspc"), t("target/codeap")),
            (t("aligntext"), t("target/aligntext_len")), (t("target/phonetext"), t("target/phonetext_len")))


def test_state_dict_hparams_and_checkpoint(golden, tmp_path):
    g, use_mcep = golden
    ref = sub(g, "state/")
    m = AlignTextToAudioMultiTaskModel(vocab_size=29, target_vocab_size=71, hidden_size=32, use_mcep=use_mcep)
    sd = m.state_dict()
    assert len(ref) == 157 and set(sd) == set(ref)
    assert all(tuple(sd[k].shape) == g["state/" + k].shape for k in sd)
    assert "decoder.layer1.0.conv.0.0.weight" in sd and "decoder.layer3.bias" in sd
    assert sd["decoder.layer1.1.conv.1.0.weight"].shape == (128, 1, 47)
    m.load_state_dict(ref, strict=True)
    assert dict(m.hparams) == {"vocab_size": 29, "target_vocab_size": 71, "hidden_size": 32, "learning_rate": 1e-3, "use_mcep": use_mcep}
    assert (m.logspc_size, m.audio_size, m.target_vocab_size) == ((25, 28, 71) if use_mcep else (257, 260, 71))
    assert (m.criterion.logspc_weights is None) == use_mcep          # WORLDLoss(use_mel_weights=not use_mcep): the one departure
    from voice100_amd._base import checkpoint_dict
    path = tmp_path / "mt.ckpt"
    torch.save(checkpoint_dict(m), str(path))
    m2 = AlignTextToAudioMultiTaskModel.load_from_checkpoint(str(path))
    assert dict(m2.hparams) == dict(m.hparams)
    assert all(torch.equal(v, m2.state_dict()[k]) for k, v in m.state_dict().items())


def test_argparse_round_trip():
    p = AlignTextToAudioMultiTaskModel.add_model_specific_args(argparse.ArgumentParser())
    args = p.parse_args([])
    assert (args.hidden_size, args.audio_stat, args.learning_rate) == (512, None, 1e-3)
    args = p.parse_args(["--hidden_size", "32", "--learning_rate", "2e-3"])
    args.vocoder, args.resume_from_checkpoint = "world_mcep", True
    m = AlignTextToAudioMultiTaskModel.from_argparse_args(args, vocab_size=29, target_vocab_size=71)
    assert m.logspc_size == 25 and m.hparams.hidden_size == 32 and m.hparams.learning_rate == 2e-3 and m.hparams.use_mcep is True
    args.vocoder = "world"
    assert AlignTextToAudioMultiTaskModel.from_argparse_args(args, vocab_size=29, target_vocab_size=71).logspc_size == 257


def test_decoder_layout():
    d = VoiceMultiTaskDecoder(32, 28, 71)
    assert [b.kernel_size for b in d.layer1] == [65, 47, 33, 17, 11, 7]
    assert [b.kernel_size for b in (d.layer2[1], d.layer2[2])] == [11, 7]
    assert d.layer2[0].weight.shape == (32, 16, 5) and d.layer2[3].weight.shape == (28, 16, 1) and d.layer3.weight.shape == (71, 32, 1)
    x, y = d.eval()(torch.randn(2, 32, 9))
    assert x.shape == (2, 28, 17) and y.shape == (2, 71, 9)


def test_stock_path_matches_fixture(golden):
    g, use_mcep = golden
    m = _model(g, use_mcep).eval()
    at = torch.from_numpy(g["aligntext"])
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
    m.train()
    losses = m._calc_batch_loss(_batch(g))
    assert len(losses) == 5
    assert np.allclose(np.array([float(v.detach()) for v in losses]), g["losses_train"], rtol=2e-4)
    sum(losses).backward()
    grads = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
    assert set(grads) == {k[len("grad/"):] for k in g if k.startswith("grad/")}
    assert_grads_close(grads, {k: g["grad/" + k] for k in grads}, 2e-3)


def test_steps_log_phone_loss(golden):
    g, use_mcep = golden
    if not hasattr(AlignTextToAudioMultiTaskModel, "logged_metrics"):
        pytest.skip("logging goes to Lightning's logger")
    m = _model(g, use_mcep).train()
    for task, step in (("train", m.training_step), ("val", m.validation_step), ("test", m.test_step)):
        step(_batch(g), 0)
        names = {f"{task}_{n}loss" for n in ("", "hasf0_", "f0_", "logspc_", "codeap_", "phone_")}
        assert names <= set(m.logged_metrics)
        total = sum(float(m.logged_metrics[n]) for n in names if n != f"{task}_loss")
        assert abs(float(m.logged_metrics[f"{task}_loss"]) - total) < 1e-4 * total


def test_phonetext_width_mismatch_raises(golden):
    g, use_mcep = golden
    m = _model(g, use_mcep).train()
    world, text, (phone, phone_len) = _batch(g)
    with pytest.raises(RuntimeError):
        m._calc_batch_loss((world, text, (phone[:, :-1], phone_len)))
    with pytest.raises(RuntimeError):
        F_.masked_cross_entropy(torch.zeros(2, 5, 7), torch.zeros(2, 8, dtype=torch.int64), torch.tensor([7, 7]))


@pytest.mark.parametrize("B,V,L,lens", [(1, 1, 1, [1]), (2, 29, 40, [38, 3]), (3, 71, 65, [70, 0, 64]), (2, 2, 7, [7, 12])])
def test_masked_cross_entropy_cpu(B, V, L, lens):
    gen = torch.Generator().manual_seed(B * 1000 + V * 10 + L)
    logits = (torch.randn(B, V, L, generator=gen) * 3).requires_grad_(True)
    target = torch.randint(0, V, (B, L), generator=gen)
    target[0, 0] = -100                                             # ignored, but counted in the mask sum
    tl = torch.tensor(lens, dtype=torch.int32)
    loss = F_.masked_cross_entropy(logits, target, tl)
    assert loss.dim() == 0
    loss.backward()
    x64 = logits.detach().double().requires_grad_(True)
    ce = torch.nn.functional.cross_entropy(x64, target, reduction="none")
    mask = (torch.arange(L)[None, :] < tl[:, None]).double()
    ref = (ce * mask).sum() / mask.sum()
    ref.backward()
    assert float(mask.sum()) == sum(min(n, L) for n in lens)
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-5 * max(abs(float(ref.detach())), 1e-3)
    assert rel_err(logits.grad, x64.grad) < 1e-5
    assert float(logits.grad[0, :, 0].abs().max()) == 0.0


def test_masked_cross_entropy_all_lengths_zero_is_nan():
    loss = F_.masked_cross_entropy(torch.randn(2, 5, 4), torch.zeros(2, 4, dtype=torch.int64), torch.tensor([0, 0]))
    assert torch.isnan(loss)


def test_header_declares_masked_ce():
    import os
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = N.load()
    for name in ("v100_masked_ce_parts", "v100_masked_ce", "v100_masked_ce_bwd"):
        assert name in N.parse_header() and hasattr(lib, name)
    assert lib.v100_masked_ce_parts(32, 512) == 32 * 8 and lib.v100_masked_ce_parts(3, 65) == 6 and lib.v100_masked_ce_parts(0, 5) == -1
    assert lib.v100_masked_ce(*([None] * 6), 1, 1, 1, None) == 3
    one = 16
    assert lib.v100_masked_ce(one, one, one, one, one, one, 1, 0, 1, None) == 1
    assert lib.v100_masked_ce_bwd(None, None, None, 1, 1, 1, None) == 3
    assert lib.v100_masked_ce_bwd(one, one, one, 1, 1, -1, None) == 1


# ---- the collate ---------------------------------------------------------------------------------------------------------

def _triple(T, D, gen):
    return (torch.rand(T, generator=gen) * 200 + 1, torch.randn(T, D, generator=gen) - 5, torch.randn(T, 1, generator=gen) - 2)


def test_collate_triples():
    from voice100_amd.data import BLANK_IDX, WorldAlignTextCollate
    gen = torch.Generator().manual_seed(5)
    Ts, Ls, Lt = (7, 12, 3), (4, 6, 2), (5, 1, 9)
    feats = [_triple(T, 25, gen) for T in Ts]
    texts = [torch.randint(1, 29, (n,), generator=gen, dtype=torch.int32) for n in Ls]
    targets = [torch.randint(1, 71, (n,), generator=gen) for n in Lt]
    collate = WorldAlignTextCollate(None)                            # triples need neither a vocoder nor a GPU
    two = collate(list(zip(feats, texts)))
    three = collate(list(zip(feats, texts, targets)))
    assert len(two) == 2 and len(three) == 3
    for out in (two, three):
        (f0, f0_len, spec, codeap), (text, text_len) = out[0], out[1]
        assert f0.shape == (3, 12) and spec.shape == (3, 12, 25) and codeap.shape == (3, 12, 1) and text.shape == (3, 6)
        assert (f0.dtype, spec.dtype, codeap.dtype) == (torch.float32,) * 3
        assert f0_len.dtype == torch.int32 and f0_len.tolist() == list(Ts)
        assert text.dtype == torch.int64 and text_len.dtype == torch.int32 and text_len.tolist() == list(Ls)
        for i, T in enumerate(Ts):
            assert torch.equal(f0[i, :T], feats[i][0]) and torch.equal(spec[i, :T], feats[i][1]) and torch.equal(codeap[i, :T], feats[i][2])
            assert not f0[i, T:].any() and not spec[i, T:].any() and not codeap[i, T:].any()
            assert torch.equal(text[i, :Ls[i]], texts[i].long()) and bool((text[i, Ls[i]:] == BLANK_IDX).all())
    target, target_len = three[2]
    assert target.shape == (3, 9) and target.dtype == torch.int64 and target_len.dtype == torch.int32 and target_len.tolist() == list(Lt)
    for i, n in enumerate(Lt):
        assert torch.equal(target[i, :n], targets[i]) and bool((target[i, n:] == BLANK_IDX).all())


def test_collate_rejects_bad_items():
    from voice100_amd.data import WorldAlignTextCollate
    gen = torch.Generator().manual_seed(6)
    collate = WorldAlignTextCollate(None)
    a, b = _triple(5, 25, gen), _triple(4, 25, gen)
    t = torch.tensor([1, 2, 3])
    with pytest.raises(ValueError):
        collate([])
    with pytest.raises(ValueError):
        collate([(a, t), (b, t, t)])                                 # two- and three-part items mixed
    with pytest.raises(ValueError):
        collate([(a, t), (torch.zeros(800), t)])                     # triples and waveforms mixed
    with pytest.raises(ValueError):
        collate([(a, t.float())])


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the message raised without a GPU")
def test_collate_waveforms_need_a_gpu(tmp_path):
    from voice100_amd.data import WorldAlignTextCollate
    from voice100_amd.vocoder import WORLDVocoder
    collate = WorldAlignTextCollate(WORLDVocoder())
    t = torch.tensor([1, 2, 3])
    with pytest.raises(RuntimeError, match="GPU only"):
        collate([(torch.zeros(800), t)])
    with pytest.raises(RuntimeError, match="GPU only"):
        collate([(str(tmp_path / "missing.wav"), t, t)])


# ---- TTSPipeline with a four-value predict ---------------------------------------------------------------------------------

class _Align(torch.nn.Module):
    def forward(self, text):
        return torch.log(torch.ones(text.shape + (2,)) + 1.0)       # gap = len = 1 for every token


class _Audio3:
    def predict(self, aligntext):
        B, La = aligntext.shape
        T = 2 * La - 1
        return torch.full((B, T), 100.0), torch.zeros(B, T, 257) - 3, torch.zeros(B, T, 1) - 1


class _Audio4(_Audio3):
    def predict(self, aligntext):
        return super().predict(aligntext) + (torch.arange(aligntext.numel() * 71, dtype=torch.float32).reshape(aligntext.shape[0], 71, -1),)


class _Audio5(_Audio3):
    def predict(self, aligntext):
        return super().predict(aligntext) + (None, None)


def test_tts_pipeline_four_value_predict(monkeypatch):
    from voice100_amd import decode
    from voice100_amd.infer import TTSPipeline

    def expand(text, align, text_len, head, tail):                   # stands in for the device kernel: the widths are all that matter here
        B, L = text.shape
        La = head + 2 * L + tail
        return text.new_ones(B, La), torch.full((B,), La, dtype=torch.int32)
    monkeypatch.setattr(decode, "align_expand", expand)
    text, text_len = torch.randint(1, 29, (2, 6)), torch.tensor([6, 4])
    three = TTSPipeline(_Align(), _Audio3())(text, text_len)
    four = TTSPipeline(_Align(), _Audio4())(text, text_len)
    keys = ["align", "aligntext", "aligntext_len", "f0", "logspc", "spc", "codeap", "frames"]
    assert list(three) == keys                                       # the three-value models: unchanged, key for key
    assert list(four) == keys + ["phone_logits"]
    La = four["aligntext"].shape[1]
    assert four["phone_logits"].shape == (2, 71, La)
    assert torch.equal(four["phone_logits"], _Audio4().predict(four["aligntext"])[3])
    for k in keys:
        assert (three[k] is None and four[k] is None) or torch.equal(three[k], four[k]), k
    with pytest.raises(RuntimeError):
        TTSPipeline(_Align(), _Audio5())(text, text_len)
