"""GPU checks of the HIP LSTM (K15) and AudioToAlignText against torch.nn.LSTM in float64 on the CPU and the reference fixture."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

from conftest import assert_grads_close, load_golden, rel_err, rel_l2
from voice100_amd import _native as N
from voice100_amd import functional as F_
from voice100_amd.lstm import LSTM

pytestmark = pytest.mark.gpu

SETTINGS = [[32, False, 5, 2, 2, False], [32, False, 5, 1, 2, False]]


@pytest.fixture(autouse=True)
def _fp32_after():
    yield
    F_.set_matmul_precision("fp32")
    F_.LSTM_PERSISTENT = True


def _lengths(B, T):
    g = torch.Generator().manual_seed(B * 1000 + T)
    lens = torch.randint(1, T + 1, (B,), generator=g)
    lens[0] = T
    if B > 1:
        lens[1] = 1
    return lens


def _case(C, H, B, T, layers, bidir, seed=0, bias=True, lens=None):
    torch.manual_seed(seed)
    ref = nn.LSTM(C, H, num_layers=layers, bias=bias, bidirectional=bidir)
    x = torch.randn(T, B, C)
    lens = _lengths(B, T) if lens is None else torch.tensor(lens)
    D = 2 if bidir else 1
    gy = torch.randn(T, B, D * H)
    gh = torch.randn(layers * D, B, H)
    gc = torch.randn(layers * D, B, H)
    return ref, x, lens, gy, gh, gc


def _oracle(ref, x, lens, gy, gh, gc, dtype=torch.float64, device="cpu", autocast=False):
    m = nn.LSTM(ref.input_size, ref.hidden_size, num_layers=ref.num_layers, bias=ref.bias, bidirectional=ref.bidirectional)
    m.load_state_dict(ref.state_dict())
    m = m.to(device=device, dtype=dtype)
    xx = x.to(device=device, dtype=dtype).requires_grad_(True)
    packed = pack_padded_sequence(xx, lens, enforce_sorted=False)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        out, (h, c) = m(packed)
    y, _ = pad_packed_sequence(out, total_length=x.shape[0])
    loss = (y.double() * gy.to(device, torch.float64)).sum() + (h.double() * gh.to(device, torch.float64)).sum() \
        + (c.double() * gc.to(device, torch.float64)).sum()
    loss.backward()
    grads = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    grads["x"] = xx.grad.detach().double().cpu()
    return y.detach().double().cpu(), h.detach().double().cpu(), c.detach().double().cpu(), grads


def _mine(ref, x, lens, gy, gh, gc, cuda, lens_on_device=False):
    m = LSTM(ref.input_size, ref.hidden_size, num_layers=ref.num_layers, bias=ref.bias, bidirectional=ref.bidirectional).to(cuda)
    m.load_state_dict(ref.state_dict())
    xx = x.to(cuda).requires_grad_(True)
    out, (h, c) = m(xx, lengths=lens.to(cuda) if lens_on_device else lens)
    loss = (out * gy.to(cuda)).sum() + (h * gh.to(cuda)).sum() + (c * gc.to(cuda)).sum()
    loss.backward()
    grads = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters()}
    grads["x"] = xx.grad.detach().double().cpu()
    return out.detach().double().cpu(), h.detach().double().cpu(), c.detach().double().cpu(), grads


CASES = [  # C, H, B, T, layers, bidirectional
    (24, 32, 3, 9, 2, True),
    (32, 64, 1, 7, 1, False),
    (48, 64, 32, 11, 1, True),
    (64, 32, 32, 6, 2, False),
    (40, 512, 3, 5, 1, True),
    (32, 512, 32, 4, 2, True),
]


@pytest.mark.parametrize("C,H,B,T,layers,bidir", CASES)
def test_fp32_against_fp64(cuda, C, H, B, T, layers, bidir):
    case = _case(C, H, B, T, layers, bidir)
    ry, rh, rc, rg = _oracle(*case)
    y, h, c, g = _mine(*case, cuda)
    assert rel_err(y, ry) < 1e-4
    assert rel_err(h, rh) < 1e-4
    assert rel_err(c, rc) < 1e-4
    assert_grads_close(g, rg, 1e-4)


@pytest.mark.parametrize("C,H,B,T,layers,bidir", [CASES[0], CASES[2], CASES[5]])
def test_bf16_against_fp16_autocast_nn_lstm(cuda, C, H, B, T, layers, bidir):
    case = _case(C, H, B, T, layers, bidir)
    ry, rh, rc, rg = _oracle(*case)
    ay, ah, ac, ag = _oracle(*case, dtype=torch.float32, device=cuda, autocast=True)
    F_.set_matmul_precision("bf16")
    y, h, c, g = _mine(*case, cuda)
    for what, mine, yard, exact in [("y", y, ay, ry), ("h_n", h, ah, rh), ("c_n", c, ac, rc)] + \
            [("grad " + k, g[k], ag[k], rg[k]) for k in rg]:
        e, e16 = rel_l2(mine, exact), rel_l2(yard, exact)
        print(f"{what}: bf16 {e:.2e}  fp16-autocast nn.LSTM {e16:.2e}")
        # bf16 keeps 3 mantissa bits fewer than fp16 (8x its unit round-off); measured up to 4.2x the fp16-autocast error here
        assert e < 2e-2 and e < 5 * e16 + 1e-4, what


def _run_layer(cuda, x_bct, lens, params, persistent, train=True, seed=3):
    x = x_bct.clone().requires_grad_(train)
    ps = [p.clone().requires_grad_(train) for p in params]
    y, h, c = F_.lstm_layer(x, lens, ps, persistent=persistent)
    if not train:
        return [y, h, c]
    g = torch.Generator(device=cuda).manual_seed(seed)
    gy, gh, gc = (torch.randn(t.shape, device=cuda, generator=g) for t in (y, h, c))
    torch.autograd.backward([y, h, c], [gy, gh, gc])
    return [y, h, c, x.grad] + [p.grad for p in ps]


def _layer_inputs(cuda, B=20, C=48, H=64, T=17, seed=5):
    torch.manual_seed(seed)
    ref = nn.LSTM(C, H, bidirectional=True)
    params = [t.detach().to(cuda) for t in ref.parameters()]
    x = torch.randn(B, C, T, device=cuda)
    lens = _lengths(B, T).to(cuda, torch.int32)
    return x, lens, params


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_persistent_bit_identical_to_step_form(cuda, precision):
    F_.set_matmul_precision(precision)
    fmt = 1 if precision == "bf16" else 0
    # B = 40 and 128: several slices, the last one ragged (40) or the grid at the persistent form's 128-workgroup cap (128)
    for B, H, T in ((20, 48, 17), (20, 64, 17), (20, 512, 9), (40, 256, 12), (128, 256, 9)):
        x, lens, params = _layer_inputs(cuda, B=B, H=H, T=T)
        assert all(N.helper("v100_lstm_persistent_ok", B, H, 2, fmt, bwd) for bwd in (0, 1)), (B, H)      # the two forms really differ
        a = _run_layer(cuda, x, lens, params, persistent=True)
        b = _run_layer(cuda, x, lens, params, persistent=False)
        for i, (u, v) in enumerate(zip(a, b)):
            assert torch.equal(u, v), (B, H, i)


def test_two_calls_bit_identical(cuda):
    x, lens, params = _layer_inputs(cuda)
    a = _run_layer(cuda, x, lens, params, persistent=True)
    b = _run_layer(cuda, x, lens, params, persistent=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_padding_is_zero_and_ignored(cuda):
    x, lens, params = _layer_inputs(cuda)
    T = x.shape[2]
    pad = torch.arange(T, device=cuda)[None, None, :] >= lens[:, None, None].long()
    a = _run_layer(cuda, x, lens, params, persistent=True)
    y = a[0]
    assert torch.all(y.masked_select(pad.expand_as(y)) == 0)
    x2 = torch.where(pad.expand_as(x), torch.full_like(x, 1e4), x)
    b = _run_layer(cuda, x2, lens, params, persistent=True)
    for i, (u, v) in enumerate(zip(a, b)):
        if i == 3:                                    # the input gradient: zero at padded positions in both
            assert torch.all(u.masked_select(pad.expand_as(u)) == 0)
        assert torch.equal(u, v), i


def test_packed_sequence_equals_padded(cuda):
    ref, x, lens, gy, gh, gc = _case(24, 32, 5, 8, 2, True, seed=11)
    m = LSTM(24, 32, num_layers=2, bidirectional=True).to(cuda)
    m.load_state_dict(ref.state_dict())
    xb = x.transpose(0, 1).contiguous().to(cuda)      # [B, T, C] as the reference packs it (batch_first=True)
    packed = pack_padded_sequence(xb, lens, batch_first=True, enforce_sorted=False)
    out, (h, c) = m(packed)
    r_out, (r_h, r_c) = ref.to(cuda)(packed)          # the structure nn.LSTM returns
    assert torch.equal(out.batch_sizes, r_out.batch_sizes)
    assert torch.equal(out.sorted_indices, r_out.sorted_indices)
    assert torch.equal(out.unsorted_indices, r_out.unsorted_indices)
    y_packed, y_len = pad_packed_sequence(out, batch_first=False)
    y_pad, (h2, c2) = m(x.to(cuda)[: int(lens.max())], lengths=lens)
    assert torch.equal(y_len, lens)
    assert torch.equal(y_packed, y_pad)
    assert torch.equal(h, h2) and torch.equal(c, c2)


def _tiny_model(cuda):
    from voice100_amd.asr import AudioToAlignText
    g = load_golden("asr_v2_tiny.npz")
    model = AudioToAlignText(audio_size=16, encoder_settings=SETTINGS, decoder_num_layers=2, decoder_hidden_size=32, vocab_size=29)
    model.load_state_dict({k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}, strict=True)
    return model.to(cuda), g


def test_asr_v2_matches_reference_fixture(cuda):
    model, g = _tiny_model(cuda)
    model.train()
    model.lstm.dropout = 0.0
    audio = torch.from_numpy(g["audio"]).to(cuda).requires_grad_(True)
    audio_len = torch.from_numpy(g["audio_len"]).to(cuda)
    logits, lens = model(audio, audio_len)
    assert logits.shape == g["logits"].shape
    assert rel_err(logits, g["logits"]) < 1e-4
    assert np.array_equal(lens.cpu().numpy(), g["logits_len"])
    text, text_len = torch.from_numpy(g["text"]).to(cuda), torch.from_numpy(g["text_len"]).to(cuda)

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


def test_full_size_training_step_fp32(cuda):
    C = H = 512
    B, T = 4, 512
    torch.manual_seed(17)
    ref = nn.LSTM(C, H, bidirectional=True)
    x = torch.randn(T, B, C)
    lens = torch.tensor([512, 300, 1, 77])
    gy, gh, gc = torch.randn(T, B, 2 * H), torch.randn(2, B, H), torch.randn(2, B, H)
    ry, rh, rc, rg = _oracle(ref, x, lens, gy, gh, gc)
    y, h, c, g = _mine(ref, x, lens, gy, gh, gc, cuda, lens_on_device=True)
    assert rel_err(y, ry) < 1e-4 and rel_err(h, rh) < 1e-4 and rel_err(c, rc) < 1e-4
    assert_grads_close(g, rg, 1e-4)


def test_trainstep_bf16_clip_lowers_ctc_loss(cuda):
    from voice100_amd.asr import AudioToAlignText
    from voice100_amd.trainer import TrainStep
    torch.manual_seed(3)
    model = AudioToAlignText(64, [[64, False, 5, 2, 2, False], [64, False, 5, 1, 2, False]], 2, 64, 29, learning_rate=3e-3).to(cuda)
    B, T = 4, 96
    audio = (torch.randn(B, T, 64) - 4).to(cuda)
    audio_len = torch.tensor([96, 80, 64, 90], device=cuda)
    text = torch.randint(1, 29, (B, 10), device=cuda)
    text_len = torch.tensor([10, 8, 6, 9], device=cuda)
    step = TrainStep(model, precision="bf16", gradient_clip_val=1.0)
    losses = [float(step(((audio, audio_len), (text, text_len)))) for _ in range(50)]
    assert all(np.isfinite(losses))
    assert np.mean(losses[-5:]) < 0.7 * np.mean(losses[:5]), losses


def test_fp32_wide_hidden_reads_w_hh_from_global(cuda):
    """fp32 at H = 1024: the W_hh slice does not fit the LDS, so only the step form runs, with A read from global memory."""
    assert not N.helper("v100_lstm_persistent_ok", 2, 1024, 1, 0, 0) and not N.helper("v100_lstm_persistent_ok", 2, 1024, 1, 0, 1)
    case = _case(32, 1024, 2, 4, 1, False, seed=21)
    ry, rh, rc, rg = _oracle(*case)
    y, h, c, g = _mine(*case, cuda)
    assert rel_err(y, ry) < 1e-4 and rel_err(h, rh) < 1e-4 and rel_err(c, rc) < 1e-4
    assert_grads_close(g, rg, 1e-4)


def test_bf16_k_tail(cuda):
    """bf16 at H = 48: the last 32-wide K chunk of the recurrent product is half padding."""
    case = _case(24, 48, 3, 7, 1, True, seed=23)
    ry, rh, rc, rg = _oracle(*case)
    ay, ah, ac, ag = _oracle(*case, dtype=torch.float32, device=cuda, autocast=True)
    F_.set_matmul_precision("bf16")
    y, h, c, g = _mine(*case, cuda)
    for what, mine, yard, exact in [("y", y, ay, ry), ("h_n", h, ah, rh), ("c_n", c, ac, rc)] + \
            [("grad " + k, g[k], ag[k], rg[k]) for k in rg]:
        assert rel_l2(mine, exact) < 5 * rel_l2(yard, exact) + 1e-4, what


def _spy_fwd(monkeypatch):
    seen = []
    real = N.call

    def spy(name, *args):
        if name == "v100_lstm_fwd":
            seen.append(tuple(a is None for a in args[8:11]))         # act, cs, hprev
        return real(name, *args)
    monkeypatch.setattr(N, "call", spy)
    return seen


def test_eval_saves_nothing(cuda, monkeypatch):
    seen = _spy_fwd(monkeypatch)
    m = LSTM(24, 32, num_layers=2, bidirectional=True).to(cuda).eval()
    x = torch.randn(6, 3, 24, device=cuda)
    lens = torch.tensor([6, 1, 4])
    with torch.no_grad():
        m(x, lengths=lens)
    for p in m.parameters():
        p.requires_grad_(False)
    m(x, lengths=lens)                                   # autograd on, but nothing can ask for a gradient
    assert seen == [(True, True, True)] * 4
    for p in m.parameters():
        p.requires_grad_(True)
    m(x, lengths=lens)
    assert seen[4:] == [(False, False, False)] * 2


def test_fp16_eval_under_no_grad(cuda):
    ref, x, lens, gy, gh, gc = _case(24, 64, 5, 9, 2, True, seed=29)
    ry, rh, rc, _ = _oracle(ref, x, lens, gy, gh, gc)
    m = LSTM(24, 64, num_layers=2, bidirectional=True).to(cuda).eval()
    m.load_state_dict(ref.state_dict())
    F_.set_matmul_precision("fp16")
    with torch.no_grad():
        y, (h, c) = m(x.to(cuda), lengths=lens)
    for mine, exact in ((y, ry), (h, rh), (c, rc)):
        assert rel_l2(mine, exact) < 2e-3
    with pytest.raises(RuntimeError):
        m(x.to(cuda), lengths=lens)                      # fp16 has no gradient kernels: a differentiable call refuses


def test_asr_v2_fp16_eval(cuda):
    model, g = _tiny_model(cuda)
    model.eval()
    F_.set_matmul_precision("fp16")
    with torch.no_grad():
        logits, lens = model(torch.from_numpy(g["audio"]).to(cuda), torch.from_numpy(g["audio_len"]).to(cuda))
    assert rel_l2(logits, g["logits"]) < 5e-3
    assert np.array_equal(lens.cpu().numpy(), g["logits_len"])


def test_asr_v2_ctc_best_path_matches_reference(cuda):
    model, g = _tiny_model(cuda)
    model.eval()
    score, hist, path, lens = model.ctc_best_path(torch.from_numpy(g["audio"]).to(cuda), torch.from_numpy(g["audio_len"]).to(cuda),
                                                  torch.from_numpy(g["text"]).to(cuda), torch.from_numpy(g["text_len"]).to(cuda))
    assert hist.dtype == torch.int32 and path.dtype == torch.int64
    assert np.array_equal(hist.cpu().numpy(), g["best/hist"])
    assert np.array_equal(path.cpu().numpy(), g["best/path"])
    assert np.array_equal(lens.cpu().numpy(), g["best/logits_len"])
    assert np.array_equal(score.cpu().numpy(), g["best/score"])


# ---- Regime sweep: every launch regime lstm.hip's ls_geometry / ls_launch choose, against fp64 nn.LSTM ----------------------------
# A regime is (U hidden units per workgroup, W_hh slice in LDS, grid = ndir * ceil(B / 16) * G, persistent form).  Each case asserts
# the regime it is meant for before it compares anything, so a later change of the geometry fails here instead of moving the case
# onto another code path.  The regime does not depend on T: T is short except where the length is the point.

def _geometry(H, fmt, backward):
    out = (ctypes.c_int * 4)()
    assert N.helper("v100_lstm_geometry", H, fmt, backward, out) == 0, (H, fmt, backward)
    return dict(zip(("U", "G", "wlds", "lds"), out))


def _assert_regime(B, H, ndir, fmt, regime, directions=(0, 1)):
    for bwd in directions:
        g = _geometry(H, fmt, bwd)
        got = (g["U"], bool(g["wlds"]), ndir * -(-B // 16) * g["G"], bool(N.helper("v100_lstm_persistent_ok", B, H, ndir, fmt, bwd)))
        assert got == regime, (f"the {('forward', 'backward')[bwd]} recurrence at B = {B}, H = {H}, fmt {fmt} runs as {got}; "
                               f"the case is meant for {regime} (U, W_hh in LDS, grid, persistent)")


def _spy_launches(monkeypatch):
    """[(entry point, kernel launches it issued)] of every recurrence call: 1 for the persistent form, T for the step form."""
    seen = []
    real = N.call

    def spy(name, *args):
        if name not in ("v100_lstm_fwd", "v100_lstm_bwd"):
            return real(name, *args)
        n0 = N.launch_count()
        real(name, *args)
        seen.append((name, N.launch_count() - n0))
    monkeypatch.setattr(N, "call", spy)
    return seen


_ORACLES = {}


def _cached_oracle(shape, bias=True, lens=None, seed=0):
    """The case and its fp64 oracle, computed once per module for the precisions that share it."""
    key = (shape, bias, lens, seed)
    if key not in _ORACLES:
        case = _case(*shape, seed=seed, bias=bias, lens=lens)
        _ORACLES[key] = case, _oracle(*case)
    return _ORACLES[key]


def _assert_bf16_close(mine, yard, exact):
    """bf16 against fp64, bounded as test_bf16_against_fp16_autocast_nn_lstm bounds it: < 2e-2 and < 5x the fp16-autocast error."""
    y, h, c, g = mine
    ay, ah, ac, ag = yard
    ry, rh, rc, rg = exact
    for what, m, a, r in [("y", y, ay, ry), ("h_n", h, ah, rh), ("c_n", c, ac, rc)] + [("grad " + k, g[k], ag[k], rg[k]) for k in rg]:
        e, e16 = rel_l2(m, r), rel_l2(a, r)
        print(f"{what}: bf16 {e:.2e}  fp16-autocast nn.LSTM {e16:.2e}")
        assert e < 2e-2 and e < 5 * e16 + 1e-4, what


P, S = True, False         # the persistent form / the step form
SWEEP = [  # id, (C, H, B, T, layers, bidirectional), bias, lengths (None: _lengths), precision, regime of forward and backward
    ("h80-U16", (40, 80, 5, 13, 2, True), True, None, "fp32", (16, True, 10, P)),                 # U = 16 as H % 32 != 0, one slice
    ("h48-U16-ragged", (48, 48, 20, 17, 1, True), True, None, "fp32", (16, True, 12, P)),         # 2nd slice holds 4 sequences
    ("b40-3slices", (64, 256, 40, 12, 1, True), True, None, "fp32", (32, True, 48, P)),           # last slice 8 wide
    ("unidir-b17", (64, 64, 17, 9, 2, False), True, None, "fp32", (32, True, 4, P)),              # 2nd slice holds 1 sequence
    ("align_en_base-fp32", (256, 256, 128, 20, 1, True), True, None, "fp32", (32, True, 128, P)),  # 8 slices, grid at the cap
    ("align_en_base-bf16", (256, 256, 128, 20, 1, True), True, None, "bf16", (32, True, 128, P)),
    ("step-lds-b33", (64, 512, 33, 12, 1, True), True, None, "fp32", (16, True, 192, S)),         # 3rd slice holds 1 sequence
    ("tts_en_base-fp32", (512, 512, 128, 16, 1, True), True, None, "fp32", (16, True, 512, S)),
    ("tts_en_base-bf16", (512, 512, 128, 16, 1, True), True, None, "bf16", (32, True, 256, S)),
    ("h1024-bf16", (32, 1024, 17, 6, 1, True), True, None, "bf16", (16, True, 256, S)),            # backward: K = 4096 slice in LDS
    ("long-bf16", (512, 512, 4, 512, 1, True), True, (512, 300, 1, 77), "bf16", (32, True, 32, P)),
    ("nobias-fp32", (24, 32, 20, 9, 2, True), False, None, "fp32", (32, True, 4, P)),
    ("nobias-bf16", (24, 32, 20, 9, 2, True), False, None, "bf16", (32, True, 4, P)),
]


@pytest.mark.parametrize("shape,bias,lens,precision,regime", [c[1:] for c in SWEEP], ids=[c[0] for c in SWEEP])
def test_regime_sweep_against_fp64(cuda, monkeypatch, shape, bias, lens, precision, regime):
    C, H, B, T, layers, bidir = shape
    fmt = {"fp32": 0, "bf16": 1}[precision]
    _assert_regime(B, H, 2 if bidir else 1, fmt, regime)
    case, exact = _cached_oracle(shape, bias, lens)
    yard = _oracle(*case, dtype=torch.float32, device=cuda, autocast=True) if fmt else None
    F_.LSTM_PERSISTENT = True
    F_.set_matmul_precision(precision)
    launches = _spy_launches(monkeypatch)
    mine = _mine(*case, cuda)
    per_call = 1 if regime[3] else T
    assert launches == [("v100_lstm_fwd", per_call)] * layers + [("v100_lstm_bwd", per_call)] * layers, launches
    if fmt:
        _assert_bf16_close(mine, yard, exact)
        return
    y, h, c, g = mine
    ry, rh, rc, rg = exact
    assert rel_err(y, ry) < 1e-4
    assert rel_err(h, rh) < 1e-4
    assert rel_err(c, rc) < 1e-4
    assert_grads_close(g, rg, 1e-4)


@pytest.mark.parametrize("shape,regime", [
    ((512, 512, 128, 16, 1, True), (32, True, 256, S)),            # tts_en_base width: step form
    ((256, 256, 128, 20, 1, True), (32, True, 128, P)),            # align_en_base width: persistent form at the cap
], ids=["step", "persistent-cap"])
def test_fp16_eval_regimes(cuda, monkeypatch, shape, regime):
    C, H, B, T, layers, bidir = shape
    _assert_regime(B, H, 2 if bidir else 1, 2, regime, directions=(0,))
    (ref, x, lens, _, _, _), (ry, rh, rc, _) = _cached_oracle(shape)
    m = LSTM(C, H, num_layers=layers, bidirectional=bidir).to(cuda).eval()
    m.load_state_dict(ref.state_dict())
    F_.LSTM_PERSISTENT = True
    F_.set_matmul_precision("fp16")
    launches = _spy_launches(monkeypatch)
    with torch.no_grad():
        y, (h, c) = m(x.to(cuda), lengths=lens)
    assert launches == [("v100_lstm_fwd", 1 if regime[3] else T)] * layers, launches
    for mine, exact in ((y, ry), (h, rh), (c, rc)):
        assert rel_l2(mine, exact) < 2e-3


def test_padded_beyond_longest_sequence(cuda, monkeypatch):
    """T = 15 with every length <= 11: y and the input gradient are exactly 0 beyond each length, and h_n / c_n are each sequence's
    own last step (direction 1 starts at len - 1, not at T - 1)."""
    shape = C, H, B, T, layers, bidir = (48, 64, 20, 15, 2, True)
    g = torch.Generator().manual_seed(31)
    lens = torch.randint(1, 12, (B,), generator=g)
    lens[0], lens[1] = 11, 1
    lens = tuple(int(v) for v in lens)
    _assert_regime(B, H, 2, 0, (32, True, 8, P))
    case, (ry, rh, rc, rg) = _cached_oracle(shape, lens=lens)
    F_.LSTM_PERSISTENT = True
    launches = _spy_launches(monkeypatch)
    y, h, c, gr = _mine(*case, cuda)
    assert launches == [("v100_lstm_fwd", 1)] * layers + [("v100_lstm_bwd", 1)] * layers, launches
    assert rel_err(y, ry) < 1e-4 and rel_err(h, rh) < 1e-4 and rel_err(c, rc) < 1e-4
    assert_grads_close(gr, rg, 1e-4)
    pad = torch.arange(T)[:, None] >= torch.tensor(lens)[None, :]           # [T, B]
    assert torch.all(y[pad] == 0)
    assert torch.all(gr["x"][pad] == 0)
    ref, x = case[0], case[1]
    m = nn.LSTM(C, H, num_layers=layers, bidirectional=bidir).double()
    m.load_state_dict(ref.state_dict())
    with torch.no_grad():
        for b, n in enumerate(lens):                  # each sequence alone, unpadded, in fp64
            _, (hb, cb) = m(x[:n, b:b + 1].double())
            assert rel_err(h[:, b], hb[:, 0]) < 1e-4 and rel_err(c[:, b], cb[:, 0]) < 1e-4, b
