"""K20 on the device: the one-launch alignment kernel against the numpy oracle and against the older best-path kernel (bit for
bit, also where the reference raises), AudioAlignCTC and AlignPipeline against the reference fixture, training and fp16 eval."""
import numpy as np
import pytest
import torch
from torch import nn

from conftest import assert_grads_close, load_golden, rel_err, rel_l2
from oracle import intops
from voice100_amd import _native as N
from voice100_amd import functional as F_

pytestmark = pytest.mark.gpu

V = 29


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    F_.set_matmul_precision("fp32")


def _logp(rng, B, T, v=V):
    return torch.log_softmax(torch.from_numpy(rng.randn(B, T, v).astype(np.float32)), -1)


def _case_ragged():
    """The ragged case of tests/test_gpu_decode.py."""
    rng = np.random.RandomState(5)
    lp = _logp(rng, 6, 90)
    labels = torch.from_numpy(rng.randint(1, V, size=(6, 17)))
    return lp, labels, [90, 77, 60, 90, 45, 88], [17, 9, 17, 1, 12, 5], 3


def _case_wide130():
    """2 L + 1 = 261 states: more than the 256 threads, the second state of a thread."""
    rng = np.random.RandomState(11)
    return _logp(rng, 2, 300), torch.from_numpy(rng.randint(1, V, size=(2, 130))), [300, 280], [130, 97], 3


def _case_wide300():
    """2 L + 1 = 601 states: the third state of a thread comes from the label row in LDS."""
    rng = np.random.RandomState(12)
    return _logp(rng, 2, 620), torch.from_numpy(rng.randint(1, V, size=(2, 300))), [620, 400], [300, 150], 3


def _case_seams():
    """Lengths of 2, blk-1, blk, blk+1, 2 blk and 2 blk + 1 frames in one batch padded beyond the longest."""
    blk = int(N.helper("v100_ctc_align_block"))
    lens = [2, blk - 1, blk, blk + 1, 2 * blk, 2 * blk + 1]
    rng = np.random.RandomState(13)
    return (_logp(rng, 6, 2 * blk + 8), torch.from_numpy(rng.randint(1, V, size=(6, 5))), lens, [min(5, t - 1) for t in lens], 3)


def _case_moves(max_move):
    rng = np.random.RandomState(14)
    return _logp(rng, 3, 60), torch.from_numpy(rng.randint(1, V, size=(3, 12))), [60, 41, 25], [12, 9, 12], max_move


def _case_ties():
    """Log-probabilities on multiples of 0.5: every sum is exact, so equal candidates are common and the first maximum decides."""
    rng = np.random.RandomState(15)
    lp = torch.round(_logp(rng, 3, 50) * 2) / 2
    labels = torch.from_numpy(rng.randint(1, V, size=(3, 8)))
    labels[1, 3] = labels[1, 2]
    return lp, labels, [50, 37, 9], [8, 8, 8], 3


def _case_neginf():
    """2 % of the entries are -inf; the seed keeps every best score finite."""
    rng = np.random.RandomState(16)
    lp = _logp(rng, 3, 60)
    lp[torch.from_numpy(rng.rand(3, 60, V) < 0.02)] = -np.inf
    return lp, torch.from_numpy(rng.randint(1, V, size=(3, 6))), [60, 44, 30], [6, 4, 6], 3


def _case_widevocab():
    """V = 150: rows too wide to be staged, the kernel gathers from global memory; T = L + 1 is the shortest aligned utterance."""
    rng = np.random.RandomState(17)
    return _logp(rng, 3, 40, 150), torch.from_numpy(rng.randint(1, 150, size=(3, 7))), [40, 8, 33], [7, 7, 3], 3


def _case_outside():
    """Where the reference raises: T_b <= L_b, T_b = 1, L_b = 0.  Only the older kernel defines these."""
    rng = np.random.RandomState(18)
    return _logp(rng, 6, 20), torch.from_numpy(rng.randint(1, V, size=(6, 9))), [5, 9, 1, 20, 1, 20], [9, 9, 4, 0, 0, 9], 3


CASES = {
    "ragged": _case_ragged, "wide130": _case_wide130, "wide300": _case_wide300, "seams": _case_seams,
    "move2": lambda: _case_moves(2), "move4": lambda: _case_moves(4), "move5": lambda: _case_moves(5),
    "ties": _case_ties, "neginf": _case_neginf, "widevocab": _case_widevocab,
}
_cache = {}


def _run(name, cuda):
    """(inputs, the new kernel's outputs on the host): computed once per case."""
    if name not in _cache:
        from voice100_amd.decode import ctc_align
        lp, labels, lens, llen, mm = (CASES.get(name) or _case_outside)()
        il, ll = torch.tensor(lens, dtype=torch.int32), torch.tensor(llen, dtype=torch.int32)
        out = ctc_align(lp.to(cuda), labels.to(cuda), il, ll, max_move=mm)
        _cache[name] = ((lp, labels, lens, llen, mm), tuple(o.cpu() for o in out))
    return _cache[name]


@pytest.mark.parametrize("name", list(CASES))
def test_ctc_align_against_oracle(cuda, name):
    (lp, labels, lens, llen, mm), (score, path, best, align) = _run(name, cuda)
    S = 2 * labels.shape[1] + 1
    assert path.dtype == torch.int32 and best.dtype == torch.int64 and align.dtype == torch.int32 and align.shape == (len(lens), S)
    for b, (t, l) in enumerate(zip(lens, llen)):
        assert l >= 1 and t >= l + 1 and (mm > 2 or t >= 2 * l + 1), "outside the reference's domain"
        s, p, bl = intops.ctc_best_path(lp[b, :t].numpy(), labels[b, :l].numpy(), max_move=mm)
        assert np.isfinite(s), (b, s)
        assert np.array_equal(path[b, :t].numpy(), p), b
        assert np.array_equal(best[b, :t].numpy(), bl), b
        assert np.array_equal(align[b].numpy(), np.bincount(p, minlength=S)), b
        assert int(align[b].sum()) == t
        assert not path[b, t:].any() and not best[b, t:].any() and not align[b, 2 * l + 1:].any()
        assert float(score[b]) == pytest.approx(float(s), rel=1e-6), b


@pytest.mark.parametrize("name", list(CASES) + ["outside"])
def test_ctc_align_bit_identical_to_best_path_kernel(cuda, name):
    from voice100_amd.decode import ctc_align, ctc_best_path
    (lp, labels, lens, llen, mm), (score, path, best, align) = _run(name, cuda)
    il, ll = torch.tensor(lens, dtype=torch.int32), torch.tensor(llen, dtype=torch.int32)
    old_score, old_path, old_best = ctc_best_path(lp.to(cuda), labels.to(cuda), il, ll, max_move=mm)
    assert torch.equal(path, old_path.cpu())
    assert torch.equal(score.view(torch.int32), old_score.cpu().view(torch.int32))       # the same bits, -inf and NaN included
    assert torch.equal(best, old_best.cpu())
    S = align.shape[1]
    for b, t in enumerate(lens):
        assert np.array_equal(align[b].numpy(), np.bincount(path[b, :t].numpy(), minlength=S)), b
    again = ctc_align(lp.to(cuda), labels.to(cuda), il, ll, max_move=mm)
    for a, o in zip(again, (score, path, best, align)):
        assert torch.equal(a.cpu().view(torch.int32) if a.dtype == torch.float32 else a.cpu(), o.view(torch.int32) if o.dtype == torch.float32 else o)


def test_ctc_align_without_lengths(cuda):
    from voice100_amd.decode import ctc_align
    rng = np.random.RandomState(19)
    lp, labels = _logp(rng, 2, 35), torch.from_numpy(rng.randint(1, V, size=(2, 6)))
    score, path, best, align = ctc_align(lp.to(cuda), labels.to(cuda))
    for b in range(2):
        s, p, bl = intops.ctc_best_path(lp[b].numpy(), labels[b].numpy())
        assert np.array_equal(path[b].cpu().numpy(), p) and np.array_equal(best[b].cpu().numpy(), bl)
        assert np.array_equal(align[b].cpu().numpy(), np.bincount(p, minlength=13))


def test_ctc_align_limits(cuda):
    from voice100_amd.decode import ctc_align
    lp = torch.zeros(1, 4, V, device=cuda)
    with pytest.raises(RuntimeError):
        ctc_align(lp, torch.ones(1, 2048, dtype=torch.int64, device=cuda))              # 2 L + 1 = 4097
    with pytest.raises(RuntimeError):
        ctc_align(lp, torch.ones(1, 2, dtype=torch.int64, device=cuda), max_move=9)
    with pytest.raises(RuntimeError):
        ctc_align(torch.zeros(1, 12001, 2, device=cuda), torch.ones(1, 2, dtype=torch.int64, device=cuda))


# ---- AudioAlignCTC and AlignPipeline against the reference fixture ----------------------------------------------------------------

def _model(cuda):
    from voice100_amd.align import AudioAlignCTC
    g = load_golden("align_v1_tiny.npz")
    model = AudioAlignCTC(16, 29, 32, 2, 1e-3)
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}, strict=True)
    return model.to(cuda), g


def _batch(g, cuda):
    return tuple(torch.from_numpy(g[k]).to(cuda) for k in ("audio", "audio_len", "text", "text_len"))


def test_audio_align_ctc_matches_reference_fixture(cuda):
    model, g = _model(cuda)
    audio, audio_len, text, text_len = _batch(g, cuda)
    model.eval()
    with torch.no_grad():
        logits, lens = model(audio, audio_len)
    assert logits.shape == g["logits_eval"].shape
    assert rel_err(logits, g["logits_eval"]) < 1e-4
    assert np.array_equal(lens.cpu().numpy(), g["logits_len"])

    model.train()
    model.lstm.dropout = 0.0
    audio.requires_grad_(True)
    logits, lens = model(audio, audio_len)
    assert rel_err(logits, g["logits"]) < 1e-4
    assert np.array_equal(lens.cpu().numpy(), g["logits_len"])

    class _NoAugment(nn.Module):                      # the fixture was made without the augmentation
        def forward(self, a, n):
            return a, n
    model.batch_augment = _NoAugment()
    loss = model.training_step(((audio, audio_len), (text, text_len)))
    assert abs(float(loss) - float(g["loss"])) < 1e-4 * abs(float(g["loss"]))
    loss.backward()
    got = {k: p.grad for k, p in model.named_parameters()}
    ref = {k[len("grad/"):]: v for k, v in g.items() if k.startswith("grad/")}
    assert set(got) == set(ref)
    assert_grads_close(got, ref, 1e-4)
    assert rel_err(audio.grad, g["grad_audio"]) < 1e-4


def test_audio_align_ctc_best_path_matches_reference(cuda):
    model, g = _model(cuda)
    audio, audio_len, text, text_len = _batch(g, cuda)
    model.eval()
    score, hist, path, lens = model.ctc_best_path(audio, audio_len, text, text_len)
    assert hist.dtype == torch.int32 and path.dtype == torch.int64
    assert np.array_equal(hist.cpu().numpy(), g["best/hist"])
    assert np.array_equal(path.cpu().numpy(), g["best/path"])
    assert np.array_equal(lens.cpu().numpy(), g["best/logits_len"])
    assert np.array_equal(score.cpu().numpy(), g["best/score"])             # the quirk: the last utterance's labels as float32
    amax = model.ctc_best_path(audio, audio_len)
    assert amax.shape == g["logits_eval"].shape[:2]
    assert torch.equal(amax, model(audio, audio_len)[0].argmax(-1))

def _assert_pipeline(out, hist, path, lens):
    assert out["hist"].dtype == torch.int32 and out["path"].dtype == torch.int64 and out["align"].dtype == torch.int32
    assert np.array_equal(out["hist"].cpu().numpy(), hist)
    assert np.array_equal(out["path"].cpu().numpy(), path)
    assert np.array_equal(out["path_len"].cpu().numpy(), lens)


def test_align_pipeline_matches_reference_fixture(cuda):
    from voice100_amd.infer import AlignPipeline, align_records
    model, g = _model(cuda)
    audio, audio_len, text, text_len = _batch(g, cuda)
    pipe = AlignPipeline(model)
    with pytest.raises(RuntimeError):
        pipe(audio, audio_len, text, text_len)                              # a fresh module is in training mode
    model.eval()
    out = pipe(audio, audio_len, text, text_len)
    _assert_pipeline(out, g["best/hist"], g["best/path"], g["best/logits_len"])
    assert np.array_equal(out["align"].cpu().numpy(), g["align"])
    assert rel_err(out["score"], g["scores"]) < 1e-4
    assert np.allclose(out["score"].cpu().numpy(), g["scores"], rtol=1e-4, atol=0)
    vocab = [str(c) for c in g["vocab"]]

    def decode(ids):
        return "".join(vocab[int(x)] for x in ids if 0 <= int(x) < len(vocab))
    assert align_records(out, text, text_len, decode) == [str(s) for s in g["lines"]]


def test_align_pipeline_with_the_v2_model(cuda):
    from voice100_amd.asr import AudioToAlignText
    from voice100_amd.infer import AlignPipeline
    g = load_golden("asr_v2_tiny.npz")
    model = AudioToAlignText(audio_size=16, encoder_settings=[[32, False, 5, 2, 2, False], [32, False, 5, 1, 2, False]],
                             decoder_num_layers=2, decoder_hidden_size=32, vocab_size=29)
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}, strict=True)
    model = model.to(cuda).eval()
    audio, audio_len, text, text_len = _batch(g, cuda)
    out = AlignPipeline(model)(audio, audio_len, text, text_len)
    _assert_pipeline(out, g["best/hist"], g["best/path"], g["best/logits_len"])
    S = 2 * text.shape[1] + 1
    for b, t in enumerate(g["best/logits_len"]):
        assert np.array_equal(out["align"][b].cpu().numpy(), np.bincount(g["best/hist"][b, :t], minlength=S))
    assert torch.isfinite(out["score"]).all()


# ---- training and precision -------------------------------------------------------------------------------------------------------

def test_trainstep_bf16_clip_lowers_ctc_loss(cuda):
    from voice100_amd.align import AudioAlignCTC
    from voice100_amd.trainer import TrainStep
    torch.manual_seed(3)
    model = AudioAlignCTC(64, 29, 64, 2, 3e-3).to(cuda)
    B, T = 4, 96
    audio = (torch.randn(B, T, 64) - 4).to(cuda)
    audio_len = torch.tensor([96, 80, 64, 90], device=cuda)
    text = torch.randint(1, 29, (B, 10), device=cuda)
    text_len = torch.tensor([10, 8, 6, 9], device=cuda)
    step = TrainStep(model, precision="bf16", gradient_clip_val=1.0)
    losses = [float(step(((audio, audio_len), (text, text_len)))) for _ in range(50)]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), losses


def test_audio_align_ctc_fp16_eval(cuda):
    model, g = _model(cuda)
    audio, audio_len, _, _ = _batch(g, cuda)
    model.eval()
    F_.set_matmul_precision("fp16")
    with torch.no_grad():
        logits, lens = model(audio, audio_len)
    assert torch.isfinite(logits).all()
    assert rel_l2(logits, g["logits_eval"]) < 5e-3
    assert np.array_equal(lens.cpu().numpy(), g["logits_len"])
