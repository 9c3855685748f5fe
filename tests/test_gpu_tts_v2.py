"""GPU checks of the v2 TTS models and their kernels: fixture parity with the reference (TextToAlignText, AlignTextToAudio), the
v2 WORLD loss (K16) and the align loss (K17) against fp64 torch formulations, v100_align_expand_v2 against the fixture and a
spec oracle, TTSPipelineV2 end to end, full-width TrainSteps and fp16 inference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import assert_grads_close, load_golden, rel_err, rel_l2
from voice100_amd import _native as N
from voice100_amd import functional as F_
from voice100_amd.decode import align_expand_v2
from voice100_amd.tts_v2 import AlignTextToAudio, TextToAlignText

pytestmark = pytest.mark.gpu

DECODER = [[32, False, 5, 1, 2, False], [32, True, 5, 2, 2, False], [32, False, 5, 1, 2, False]]
BASE_DECODER = [[512, False, 5, 1, 2, False], [512, True, 5, 2, 2, False], [512, False, 5, 1, 2, False]]


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    F_.set_matmul_precision("fp32")


def _params(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(prefix)}


def _golden(S):
    return load_golden("tts_v2_tiny.npz" if S == 25 else "tts_v2_tiny_s257.npz")


def _align_model(cuda):
    g = load_golden("tts_v2_tiny.npz")
    m = TextToAlignText(29, 2, 32, 2, 1e-3)
    m.load_state_dict(_params(g, "align/param/"), strict=True)
    return m.to(cuda), g


def _audio_model(S, cuda):
    g = _golden(S)
    m = AlignTextToAudio(vocab_size=29, logspc_size=S, codeap_size=1, encoder_num_layers=2, encoder_hidden_size=32,
                         decoder_settings=DECODER)
    m.load_state_dict(_params(g, f"audio{S}/param/"), strict=True)
    return m.to(cuda), g


# ---- fixture parity ------------------------------------------------------------------------------------------------------------

def test_align_model_matches_reference_fixture(cuda):
    m, g = _align_model(cuda)
    m.train()
    m.lstm.dropout = 0.0
    text, text_len = torch.from_numpy(g["align/text"]).to(cuda), torch.from_numpy(g["align/text_len"]).to(cuda)
    pred, pred_len = m(text, text_len)
    assert pred.shape == g["align/pred"].shape
    assert rel_err(pred, g["align/pred"]) < 1e-4
    assert np.array_equal(pred_len.cpu().numpy(), g["align/pred_len"])
    align = torch.from_numpy(g["align/align"]).to(cuda)
    loss = m.training_step(((text, text_len), (align, 2 * text_len + 1)))
    assert abs(float(loss) - float(g["align/loss"])) < 1e-4 * abs(float(g["align/loss"]))
    loss.backward()
    got = {k: p.grad for k, p in m.named_parameters()}
    ref = _params(g, "align/grad/")
    assert set(got) == set(ref)
    assert_grads_close(got, ref, 1e-4)
    m.eval()
    with torch.no_grad():
        a, a_len = m.predict(text, text_len)
    assert rel_err(a, g["align/predict"]) < 1e-4
    assert np.array_equal(a_len.cpu().numpy(), g["align/predict_len"])


@pytest.mark.parametrize("S", [25, 257])
def test_audio_model_matches_reference_fixture(cuda, S):
    m, g = _audio_model(S, cuda)
    p = f"audio{S}/"
    m.train()
    m.lstm.dropout = 0.0
    at, at_len = torch.from_numpy(g[p + "aligntext"]).to(cuda), torch.from_numpy(g[p + "aligntext_len"]).to(cuda)
    outs = m(at, at_len)
    for got, name in zip(outs, ("hasf0_logits", "f0_hat", "logspc_hat", "hascodeap_logits", "codeap_hat")):
        ref = g[p + "out/" + name]
        assert got.shape == ref.shape, name
        assert rel_err(got, ref) < 1e-4, name
    batch = ((torch.from_numpy(g[p + "f0"]).to(cuda), torch.from_numpy(g[p + "f0_len"]).to(cuda),
              torch.from_numpy(g[p + "logspc"]).to(cuda), torch.from_numpy(g[p + "codeap"]).to(cuda)), (at, at_len))
    terms = torch.stack([t.detach() for t in m._calc_batch_loss(batch)])
    assert rel_err(terms, g[p + "terms"]) < 1e-4
    for a, b in zip(terms.cpu().numpy(), g[p + "terms"]):
        assert abs(a - b) <= 1e-4 * abs(b) + 1e-7
    loss = m.training_step(batch)
    assert abs(float(loss) - float(g[p + "loss"])) < 1e-4 * abs(float(g[p + "loss"]))
    loss.backward()
    got = {k: q.grad for k, q in m.named_parameters() if q.grad is not None}
    ref = _params(g, p + "grad/")
    assert set(got) == set(ref)
    assert_grads_close(got, ref, 1e-4)
    m.eval()
    with torch.no_grad():
        f0, logspc, codeap = m.predict(at, at_len)
    for got, name in ((f0, "f0"), (logspc, "logspc"), (codeap, "codeap")):
        ref = g[p + "predict/" + name]
        assert got.shape == ref.shape, name
        assert rel_err(got, ref) < 1e-4, name
    # the gates: exact zeros where the reference's logits are negative
    assert np.array_equal(f0.cpu().numpy() == 0, g[p + "predict/f0"] == 0)
    assert np.array_equal(codeap.cpu().numpy() == 0, g[p + "predict/codeap"] == 0)


# ---- K16: the v2 WORLD loss -----------------------------------------------------------------------------------------------------

def _norm(S, C, g):
    return (torch.tensor([140.0]) + torch.randn(1, generator=g) * 10, torch.tensor([55.0]) + torch.rand(1, generator=g) * 10,
            torch.randn(S, generator=g) * 2 - 3, torch.rand(S, generator=g) + 0.5,
            torch.randn(C, generator=g) * 0.3 - 0.5, torch.rand(C, generator=g) * 0.5 + 0.5)


def _world_loss_ref(pred, length, f0, logspc, codeap, norm, l1):
    """The v2 WORLDLoss with the target preparation, in float64 from torch.nn.functional ops."""
    d = torch.float64
    pred = pred.to(d)
    S, C = logspc.shape[2], codeap.shape[2]
    hasf0 = (f0 >= 30.0).to(d)
    hascodeap = (codeap < -0.2).to(d)
    f0m, f0s, lsm, lss, cam, cas = (t.to(d) for t in norm)
    f0n, lsn, can = (f0.to(d) - f0m) / f0s, (logspc.to(d) - lsm) / lss, (codeap.to(d) - cam) / cas
    n = min(pred.shape[1], f0.shape[1])
    pred, hasf0, hascodeap, f0n, lsn, can = pred[:, :n], hasf0[:, :n], hascodeap[:, :n], f0n[:, :n], lsn[:, :n], can[:, :n]
    mask = (torch.arange(n)[None, :] < length[:, None]).to(d)

    def el(a, b):
        return F.l1_loss(a, b, reduction="none") if l1 else F.mse_loss(a, b, reduction="none")
    h = F.binary_cross_entropy_with_logits(pred[:, :, 0], hasf0, reduction="none") * mask
    f = el(pred[:, :, 1], f0n) * hasf0 * mask
    ls = torch.mean(el(pred[:, :, 2:2 + S], lsn), dim=2) * mask
    hc = torch.mean(F.binary_cross_entropy_with_logits(pred[:, :, 2 + S:2 + S + C], hascodeap, reduction="none"), dim=2) * mask
    c = torch.mean(el(pred[:, :, 2 + S + C:], can) * hascodeap, dim=2) * mask
    ms = torch.sum(mask)
    return torch.stack([torch.sum(x) / ms for x in (h, f, ls, hc, c)])


@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("S", [25, 257])
@pytest.mark.parametrize("Tp,Tt", [(37, 50), (40, 40), (45, 31)])
def test_world_loss_v2_against_fp64(cuda, loss, S, Tp, Tt):
    g = torch.Generator().manual_seed(S * 100 + Tp + Tt)
    B, C = 4, 1
    pred = torch.randn(B, Tp, 2 + S + 2 * C, generator=g) * 1.5
    f0 = torch.where(torch.rand(B, Tt, generator=g) < 0.3, torch.zeros(B, Tt), torch.rand(B, Tt, generator=g) * 260)
    logspc = torch.randn(B, Tt, S, generator=g) * 2 - 3
    codeap = torch.randn(B, Tt, C, generator=g) * 0.3 - 0.2
    length = torch.tensor([Tt + 7, 1, Tt // 2, min(Tp, Tt) - 1])          # one past Tt, one of 1, ragged
    norm = _norm(S, C, g)
    gout = torch.rand(5, generator=g) + 0.5
    pref = pred.double().requires_grad_(True)
    ref = _world_loss_ref(pref, length, f0, logspc, codeap, norm, loss == "l1")
    (ref * gout.double()).sum().backward()

    results = []
    for _ in range(2):
        pg = pred.to(cuda).requires_grad_(True)
        out = F_.world_loss_v2(pg, length.to(cuda), f0.to(cuda), logspc.to(cuda), codeap.to(cuda), [t.to(cuda) for t in norm], loss)
        (out * gout.to(cuda)).sum().backward()
        results.append((out.detach().cpu(), pg.grad.cpu()))
    assert rel_err(results[0][0], ref.detach()) < 1e-5
    for a, b in zip(results[0][0].double(), ref.detach()):
        assert abs(float(a - b)) <= 1e-5 * abs(float(b)) + 1e-7
    assert rel_err(results[0][1], pref.grad) < 1e-5
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])     # deterministic


# ---- K17: the align loss ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,L", [(3, 7), (16, 160), (128, 40)])
def test_align_loss_against_fp64(cuda, B, L):
    g = torch.Generator().manual_seed(B * 1000 + L)
    text_len = torch.randint(1, L + 1, (B,), generator=g)
    text_len[0] = L
    pred = torch.randn(B, L, 2, generator=g)
    align = torch.randint(0, 15, (B, 2 * L + 1), generator=g)
    gout = 0.75
    pref = pred.double().requires_grad_(True)
    al = align[:, :-1].reshape(B, -1, 2)
    lg = torch.log((al + 1).to(torch.float64))
    per = torch.mean(torch.abs(lg - pref), dim=2)
    mask = (torch.arange(L)[None, :] < text_len[:, None]).double()
    ref = torch.sum(per * mask) / torch.sum(mask)
    (ref * gout).backward()
    results = []
    for _ in range(2):
        pg = pred.to(cuda).requires_grad_(True)
        out = F_.align_loss(pg, align.to(cuda), text_len.to(cuda))
        (out * gout).backward()
        results.append((out.detach().cpu(), pg.grad.cpu()))
    assert abs(float(results[0][0]) - float(ref)) <= 1e-5 * abs(float(ref))
    assert rel_err(results[0][1], pref.grad) < 1e-5
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


# ---- v100_align_expand_v2 -------------------------------------------------------------------------------------------------------

def _align_oracle(text, align, head, tail):
    """The v2 expansion from its specification: fp64 running position, trunc toward zero, >= 1 frame per token, the documented
    overflow rule.  text [L] list, align [L][2] list of floats -> list of ints."""
    total = 0.0
    for g, n in align:
        total += g
        total += n
    total -= align[0][0]
    length = head + int(total) + tail
    t, u, spans = float(head), 0, []
    for i, (g, n) in enumerate(align):
        if i:
            t += g
        s = max(int(t), u)
        t += n
        e = max(int(t), s + 1)
        u = e
        spans.append((s, e))
    row = [0] * max(length, u)
    for tok, (s, e) in zip(text, spans):
        for j in range(s, e):
            row[j] = tok
    return row


def test_align_expand_v2_matches_fixture(cuda):
    m, g = _align_model(cuda)
    i = 0
    while f"alignfn/{i}/text" in g:
        text = torch.from_numpy(g[f"alignfn/{i}/text"]).to(cuda)
        align = torch.from_numpy(g[f"alignfn/{i}/align"]).to(cuda)
        out = m.align(text, align)
        assert np.array_equal(out.cpu().numpy(), g[f"alignfn/{i}/out"]), i
        i += 1
    assert i >= 5


def test_align_expand_v2_against_spec_oracle(cuda):
    g = torch.Generator().manual_seed(99)
    for trial in range(300):
        B = int(torch.randint(1, 6, (1,), generator=g))
        L = int(torch.randint(1, 40, (1,), generator=g))
        text_len = torch.randint(1, L + 1, (B,), generator=g)
        text = torch.randint(1, 29, (B, L), generator=g)
        scale = [0.3, 1.0, 4.0][trial % 3]
        align = (torch.rand(B, L, 2, generator=g) * scale * 2 - 0.95).clamp_min(-0.99).to(torch.float32)
        head, tail = [(5, 5), (0, 0), (2, 7)][trial % 3]
        out, n = align_expand_v2(text.to(cuda), align.to(cuda), text_len.to(cuda), head, tail)
        out, n = out.cpu(), n.cpu()
        rows = []
        for b in range(B):
            lb = int(text_len[b])
            rows.append(_align_oracle(text[b, :lb].tolist(), align[b, :lb].double().tolist(), head, tail))
        assert out.shape == (B, max(len(r) for r in rows)), trial
        for b, r in enumerate(rows):
            assert int(n[b]) == len(r), (trial, b)
            assert out[b, :len(r)].tolist() == r, (trial, b)
            assert int(out[b, len(r):].abs().sum()) == 0


def test_align_expand_v2_overflow_length(cuda):
    text = torch.tensor([[3, 4, 5, 6, 7, 8]], device=cuda)
    align = torch.full((1, 6, 2), 0.01, device=cuda)
    out, n = align_expand_v2(text, align, None, 0, 0)              # 0 + int(0.11) + 0 = 0 frames: the spans need 6
    assert int(n[0]) == 6 and out[0].tolist() == [3, 4, 5, 6, 7, 8]
    out, n = align_expand_v2(text, align, None, 5, 5)              # 5 + 0 + 5 = 10 frames: the last span ends at 5 + 6 = 11
    assert int(n[0]) == 11 and out[0].tolist() == [0] * 5 + [3, 4, 5, 6, 7, 8]


# ---- the sample chain ------------------------------------------------------------------------------------------------------------

def test_tts_pipeline_v2_end_to_end(cuda):
    from voice100_amd.infer import TTSPipelineV2
    from voice100_amd.vocoder import WORLDVocoder
    am, g = _align_model(cuda)
    au, _ = _audio_model(25, cuda)
    gen = torch.Generator().manual_seed(12)
    with torch.no_grad():                    # plausible WORLD statistics, so the untrained model's f0 and spectra stay physical
        au.norm.f0_mean.fill_(120.0)
        au.norm.f0_std.fill_(10.0)
        au.norm.logspc_mean.copy_(torch.randn(25, generator=gen) * 0.3)
        au.norm.logspc_std.fill_(0.2)
        au.norm.codeap_mean.fill_(-1.0)
        au.norm.codeap_std.fill_(0.7)
    chain = TTSPipelineV2(am.eval(), au.eval(), WORLDVocoder(use_mcep=True).to(cuda))
    text, text_len = torch.from_numpy(g["align/text"]).to(cuda), torch.from_numpy(g["align/text_len"]).to(cuda)
    out = chain(text, text_len)
    B = text.shape[0]
    with torch.no_grad():
        align, _ = am.predict(text, text_len)
    ref_rows = [am.align(text[b, :int(text_len[b])].cpu(), align[b, :int(text_len[b])].cpu()) for b in range(B)]
    n = out["aligntext_len"].cpu()
    assert [int(x) for x in n] == [len(r) for r in ref_rows]
    assert out["aligntext"].shape == (B, max(len(r) for r in ref_rows))
    for b, r in enumerate(ref_rows):
        assert out["aligntext"][b, :len(r)].cpu().tolist() == r.tolist()
    T = 2 * int(n.max()) - 1
    assert out["f0"].shape == (B, T) and out["logspc"].shape == (B, T, 257) and out["codeap"].shape == (B, T, 1)
    with torch.no_grad():
        x = au._project(out["aligntext"], out["aligntext_len"])
    assert torch.all(out["f0"][x[:, :, 0] < 0] == 0)
    assert torch.all(out["codeap"][x[:, :, 27:28] < 0] == 0)
    assert out["frames"].cpu().tolist() == [min(2 * int(v), T) for v in n]
    assert "wave" in out and out["wave"].shape[0] == B
    assert torch.all(out["n_pulses"] >= 0) and torch.isfinite(out["wave"]).all()


# ---- full-width training steps and inference ------------------------------------------------------------------------------------

def _tts_batch(cuda, B=8, L=150, S=25):
    g = torch.Generator().manual_seed(41)
    at_len = torch.randint(L // 2, L + 1, (B,), generator=g)
    at_len[0] = L
    at = torch.randint(1, 29, (B, L), generator=g) * (torch.arange(L)[None, :] < at_len[:, None])
    table_f0 = torch.where(torch.rand(29, generator=g) < 0.3, torch.zeros(29), 80 + torch.rand(29, generator=g) * 150)
    table_ls = torch.randn(29, S, generator=g) * 2 - 3
    table_ca = torch.randn(29, 1, generator=g) * 0.3 - 0.2
    frames = at.repeat_interleave(2, dim=1)                                   # Tt = 2 L: two frames per aligned token
    f0, logspc, codeap = table_f0[frames], table_ls[frames], table_ca[frames]
    return ((f0.to(cuda), (2 * at_len).to(cuda), logspc.to(cuda), codeap.to(cuda)), (at.to(cuda), at_len.to(cuda)))


@pytest.mark.parametrize("precision", [32, "bf16"])
def test_tts_en_base_trainstep_lowers_loss(cuda, precision):
    from voice100_amd.trainer import TrainStep
    torch.manual_seed(5)
    m = AlignTextToAudio(29, 25, 1, 2, 512, BASE_DECODER).to(cuda)
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for t, v in zip((m.norm.f0_mean, m.norm.f0_std, m.norm.logspc_mean, m.norm.logspc_std, m.norm.codeap_mean, m.norm.codeap_std),
                        _norm(25, 1, g)):
            t.copy_(v)
    batch = _tts_batch(cuda)
    step = TrainStep(m, precision=precision, gradient_clip_val=1.0)
    losses = [float(step(batch)) for _ in range(50)]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), losses


@pytest.mark.parametrize("precision", [32, "bf16"])
def test_align_en_base_trainstep_lowers_loss(cuda, precision):
    from voice100_amd.trainer import TrainStep
    torch.manual_seed(7)
    m = TextToAlignText(29, 2, 256, 2, 1e-3).to(cuda)
    g = torch.Generator().manual_seed(8)
    B, L = 8, 120
    text_len = torch.randint(L // 3, L + 1, (B,), generator=g)
    text_len[0] = L
    text = torch.randint(1, 29, (B, L), generator=g) * (torch.arange(L)[None, :] < text_len[:, None])
    pairs = torch.stack([text % 3, text % 7 + 1], dim=2) * (text > 0)[:, :, None]
    align = torch.cat([pairs.reshape(B, 2 * L), torch.zeros(B, 1, dtype=torch.int64)], dim=1)
    batch = ((text.to(cuda), text_len.to(cuda)), (align.to(cuda), (2 * text_len + 1).to(cuda)))
    step = TrainStep(m, precision=precision, gradient_clip_val=1.0)
    losses = [float(step(batch)) for _ in range(50)]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), losses


def test_fp16_predict_saves_nothing(cuda, monkeypatch):
    am, g = _align_model(cuda)
    au, ga = _audio_model(25, cuda)
    am.eval()
    au.eval()
    text, text_len = torch.from_numpy(g["align/text"]).to(cuda), torch.from_numpy(g["align/text_len"]).to(cuda)
    at, at_len = torch.from_numpy(ga["audio25/aligntext"]).to(cuda), torch.from_numpy(ga["audio25/aligntext_len"]).to(cuda)
    seen = []
    real = N.call

    def spy(name, *args):
        if name == "v100_lstm_fwd":
            seen.append(tuple(a is None for a in args[8:11]))         # act, cs, hprev
        return real(name, *args)
    monkeypatch.setattr(N, "call", spy)
    F_.set_matmul_precision("fp16")
    with torch.no_grad():
        a, _ = am.predict(text, text_len)
        f0, logspc, codeap = au.predict(at, at_len)
    assert seen and all(s == (True, True, True) for s in seen)
    assert rel_l2(a, g["align/predict"]) < 5e-3
    assert rel_l2(logspc, ga["audio25/predict/logspc"]) < 5e-3
    assert torch.isfinite(f0).all() and torch.isfinite(codeap).all()
