"""CPU-side checks of the LSTM module and the v2 ASR model (K15): parameter names, shapes and initialisation are nn.LSTM's and
the reference's, unsupported options raise, nothing runs on the CPU, and the library exports the recurrence's entry points."""
import ctypes
import re

import pytest
import torch
from torch import nn

from conftest import load_golden
from voice100_amd.lstm import LSTM


@pytest.mark.parametrize("layers,bidir,bias", [(1, False, True), (2, True, True), (3, True, False)])
def test_state_dict_matches_nn_lstm(layers, bidir, bias):
    torch.manual_seed(7)
    ref = nn.LSTM(24, 32, num_layers=layers, bias=bias, bidirectional=bidir, dropout=0.1 if layers > 1 else 0.0)
    torch.manual_seed(7)
    mine = LSTM(24, 32, num_layers=layers, bias=bias, bidirectional=bidir, dropout=0.1 if layers > 1 else 0.0)
    a, b = ref.state_dict(), mine.state_dict()
    assert list(a) == list(b)
    for k in a:
        assert a[k].shape == b[k].shape, k
        assert torch.equal(a[k], b[k]), k          # same initialisation draws in the same order
    mine2 = LSTM(24, 32, num_layers=layers, bias=bias, bidirectional=bidir)
    mine2.load_state_dict(a, strict=True)
    assert all(torch.equal(mine2.state_dict()[k], a[k]) for k in a)


def test_model_state_dict_matches_fixture():
    from voice100_amd.asr import AudioToAlignText
    g = load_golden("asr_v2_tiny.npz")
    ref = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    model = AudioToAlignText(audio_size=16, encoder_settings=[[32, False, 5, 2, 2, False], [32, False, 5, 1, 2, False]],
                             decoder_num_layers=2, decoder_hidden_size=32, vocab_size=29)
    sd = model.state_dict()
    assert list(sd) == list(ref)
    assert all(sd[k].shape == ref[k].shape for k in sd)
    model.load_state_dict(ref, strict=True)


def test_unsupported_options_raise():
    with pytest.raises(NotImplementedError):
        LSTM(16, 32, proj_size=8)
    with pytest.raises(NotImplementedError):
        LSTM(16, 20)                                 # hidden size not a multiple of 16
    m = LSTM(16, 32)
    x = torch.zeros(4, 2, 16)
    with pytest.raises(NotImplementedError):
        m(x, (torch.zeros(1, 2, 32), torch.zeros(1, 2, 32)), lengths=torch.tensor([4, 4]))
    with pytest.raises(NotImplementedError):
        m(x)                                         # a padded tensor needs lengths=


def test_no_cpu_fallback():
    from voice100_amd.asr import AudioToAlignText
    m = LSTM(16, 32, bidirectional=True)
    with pytest.raises(RuntimeError):
        m(torch.zeros(4, 2, 16), lengths=torch.tensor([4, 3]))
    packed = nn.utils.rnn.pack_padded_sequence(torch.zeros(2, 4, 16), torch.tensor([4, 3]), batch_first=True, enforce_sorted=False)
    with pytest.raises(RuntimeError):
        m(packed)
    model = AudioToAlignText(16, [[32, False, 5, 2, 2, False]], 1, 32, 29)
    with pytest.raises(RuntimeError):
        model(torch.zeros(2, 10, 16), torch.tensor([10, 7]))


def test_header_exports_lstm_symbols():
    from voice100_amd import _native as N
    import __graft_entry__
    import os
    if not os.path.exists(N.LIB_PATH):
        __graft_entry__.build()
    lib = N.load()
    text = open(N.HEADER_PATH).read()
    names = ["v100_lstm_weight_bytes", "v100_lstm_ws_bytes", "v100_lstm_sync_words", "v100_lstm_persistent_ok",
             "v100_lstm_weight_prep", "v100_lstm_fwd", "v100_lstm_bwd", "v100_lstm_geometry"]
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
    # host helpers need no GPU; NULL pointers and bad shapes are reported, not dereferenced
    assert lib.v100_lstm_weight_bytes(512, 2, 1, 0) >= 2 * 4 * 512 * 512 * 2
    assert lib.v100_lstm_ws_bytes(32, 512, 2, 1) >= (2 * 2 * 32 * 2048 + 2 * 32 * 512) * 4
    assert lib.v100_lstm_sync_words(32, 2) % 4 == 0 and lib.v100_lstm_sync_words(32, 2) >= 4 + 4
    assert lib.v100_lstm_fwd(*([None] * 13), 1, 1, 32, 1, 0, 1, None) == 3
    assert lib.v100_lstm_bwd(*([None] * 10), 1, 1, 32, 1, 0, 1, None) == 3
    assert lib.v100_lstm_weight_prep(None, None, 32, 1, 0, 0, None, None) == 3
    assert lib.v100_lstm_weight_bytes(40, 1, 0, 0) == 0


def _geometry(lib, H, fmt, backward):
    out = (ctypes.c_int * 4)()
    assert lib.v100_lstm_geometry(H, fmt, backward, out) == 0, (H, fmt, backward)
    return dict(zip(("U", "G", "wlds", "lds"), out))


# (fmts, directions, H, U, W_hh in LDS or None for either): the regimes tests/test_gpu_lstm.py's sweep relies on
LSTM_REGIMES = [
    ((0,), (0,), 512, 16, 1),         # fp32 forward at the tts_en_base width: the U = 32 slice does not fit the LDS
    ((0,), (1,), 512, 16, 1),
    ((1,), (0,), 512, 32, 1),
    ((0,), (0, 1), 1024, 16, 0),      # fp32 at H = 1024: W_hh read from global memory, step form only
    ((1,), (0, 1), 1024, 16, 1),      # bf16 at H = 1024: the backward keeps a K = 4096 slice in LDS
    ((0, 1, 2), (0, 1), 48, 16, None),
    ((0, 1, 2), (0, 1), 80, 16, None),
    ((0,), (0,), 256, 32, 1),         # align_en_base
    ((1,), (0,), 256, 32, 1),
]


def test_lstm_geometry_regimes_and_invariants():
    from voice100_amd import _native as N
    import __graft_entry__
    import os
    if not os.path.exists(N.LIB_PATH):
        __graft_entry__.build()
    lib = N.load()
    for fmts, dirs, H, U, wlds in LSTM_REGIMES:
        for fmt in fmts:
            for bwd in dirs:
                if bwd and fmt == 2:
                    continue                          # fp16 is an inference precision
                g = _geometry(lib, H, fmt, bwd)
                assert g["U"] == U, (fmt, bwd, H, g)
                assert wlds is None or g["wlds"] == wlds, (fmt, bwd, H, g)
    for fmt, bwd in [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1)]:
        for H in range(16, 1025, 16):
            g = _geometry(lib, H, fmt, bwd)
            assert g["U"] in (16, 32) and H % g["U"] == 0 and g["G"] * g["U"] == H, (fmt, bwd, H, g)
            assert g["lds"] > 0 and (not g["wlds"] or g["lds"] <= 160 * 1024), (fmt, bwd, H, g)
            for ndir in (1, 2):
                wb = lib.v100_lstm_weight_bytes(H, ndir, fmt, bwd)
                assert wb > 0 and wb % (ndir * g["G"]) == 0, (fmt, bwd, H, ndir, wb, g)
    out = (ctypes.c_int * 4)()
    for H, fmt, bwd in [(0, 0, 0), (8, 0, 0), (40, 0, 0), (1040, 0, 0), (2048, 1, 1), (64, -1, 0), (64, 3, 0), (64, 2, 1)]:
        assert lib.v100_lstm_geometry(H, fmt, bwd, out) == 1, (H, fmt, bwd)
    assert lib.v100_lstm_geometry(64, 0, 0, None) == 3


def test_traced_forward_is_stock_lstm():
    """While a graph is recorded (torch.jit.trace / torch.onnx.export) the module is the aten LSTM nn.LSTM records."""
    torch.manual_seed(3)
    ref = nn.LSTM(16, 32, num_layers=2, bidirectional=True)
    mine = LSTM(16, 32, num_layers=2, bidirectional=True)
    mine.load_state_dict(ref.state_dict())
    ref.eval()
    mine.eval()
    x = torch.randn(5, 2, 16)
    class Wrap(nn.Module):
        def __init__(self):
            super().__init__()
            self.lstm = mine

        def forward(self, t):
            return self.lstm(t, lengths=torch.tensor([5, 5]))[0]
    traced = torch.jit.trace(Wrap(), (x,), check_trace=False)
    assert "lstm" in str(traced.graph)
    assert torch.allclose(traced(x), ref(x)[0], atol=1e-6)



def test_traced_padded_input_honours_lengths():
    """Traced with lengths shorter than the padding: the packed round trip, as the eager path computes it."""
    torch.manual_seed(4)
    ref = nn.LSTM(16, 32, bidirectional=True)
    mine = LSTM(16, 32, bidirectional=True)
    mine.load_state_dict(ref.state_dict())
    x = torch.randn(6, 3, 16)
    lens = torch.tensor([6, 2, 4])

    class Wrap(nn.Module):
        def __init__(self):
            super().__init__()
            self.lstm = mine

        def forward(self, t):
            y, (h, c) = self.lstm(t, lengths=lens)
            return y, h, c
    with torch.no_grad():
        y, h, c = torch.jit.trace(Wrap(), (x,), check_trace=False)(x)
        out, (rh, rc) = ref(nn.utils.rnn.pack_padded_sequence(x, lens, enforce_sorted=False))
        ry, _ = nn.utils.rnn.pad_packed_sequence(out, total_length=6)
    assert torch.allclose(y, ry, atol=1e-6) and torch.allclose(h, rh, atol=1e-6) and torch.allclose(c, rc, atol=1e-6)
    assert torch.all(y[4:, 2] == 0) and torch.all(y[2:, 1] == 0)
