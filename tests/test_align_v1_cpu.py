"""CPU-side checks of the v1 aligner (K20): AudioAlignCTC's parameter names and count are the reference's, the traced forward is
the stock-op restatement, nothing runs on the CPU, the library exports the alignment entry points and their host-side argument
checks work without a device, and align_records formats the alignment file's lines."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden
from voice100_amd.align import AudioAlignCTC


def _fixture_model():
    g = load_golden("align_v1_tiny.npz")
    ref = {k[len("param/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")}
    return AudioAlignCTC(16, 29, 32, 2, 1e-3), ref, g


def test_state_dict_matches_fixture():
    model, ref, _ = _fixture_model()
    sd = model.state_dict()
    assert list(sd) == list(ref)
    assert all(k.split(".")[0] in ("conv", "lstm", "dense") for k in sd)
    assert all(sd[k].shape == ref[k].shape for k in sd)
    model.load_state_dict(ref, strict=True)
    assert dict(model.hparams) == {"audio_size": 16, "vocab_size": 29, "hidden_size": 32, "num_layers": 2, "learning_rate": 1e-3}


def test_default_size_parameter_count():
    import argparse
    args = AudioAlignCTC.add_model_specific_args(argparse.ArgumentParser()).parse_args([])
    model = AudioAlignCTC.from_argparse_args(args, audio_size=64, vocab_size=29)
    assert sum(p.numel() for p in model.parameters()) == 691613
    assert isinstance(model.criterion, torch.nn.CTCLoss) and model.criterion.zero_infinity
    assert isinstance(model.configure_optimizers(), torch.optim.Adam)


def test_traced_forward_matches_fixture():
    """While a graph is recorded the module is stock ops: pack_padded_sequence -> aten LSTM -> pad_packed_sequence."""
    model, ref, g = _fixture_model()
    model.load_state_dict(ref, strict=True)
    model.eval()
    audio, audio_len = torch.from_numpy(g["audio"]), torch.from_numpy(g["audio_len"])
    with torch.no_grad():
        traced = torch.jit.trace(model, (audio, audio_len), check_trace=False)
        logits, lens = traced(audio, audio_len)
    assert "lstm" in str(traced.graph)
    assert logits.shape == g["logits_eval"].shape
    assert torch.allclose(logits, torch.from_numpy(g["logits_eval"]), atol=1e-5)
    assert np.array_equal(lens.numpy(), g["logits_len"])


def test_no_cpu_fallback():
    from voice100_amd.decode import ctc_align
    from voice100_amd.infer import AlignPipeline
    model, _, g = _fixture_model()
    audio, audio_len = torch.from_numpy(g["audio"]), torch.from_numpy(g["audio_len"])
    text, text_len = torch.from_numpy(g["text"]), torch.from_numpy(g["text_len"])
    with pytest.raises(RuntimeError):
        model(audio, audio_len)
    with pytest.raises(RuntimeError):
        ctc_align(torch.zeros(1, 8, 29), torch.ones(1, 3, dtype=torch.int64))
    model.eval()
    with pytest.raises(RuntimeError, match="GPU"):
        AlignPipeline(model)(audio, audio_len, text, text_len)
    model.train()
    with pytest.raises(RuntimeError, match="training"):
        AlignPipeline(model)(audio, audio_len, text, text_len)


def _lib():
    from voice100_amd import _native as N
    import __graft_entry__
    if not os.path.exists(N.LIB_PATH):
        __graft_entry__.build()
    return N, N.load()


def test_header_exports_align_symbols():
    N, lib = _lib()
    text = open(N.HEADER_PATH).read()
    for n in ("v100_ctc_align", "v100_ctc_align_workspace_bytes", "v100_ctc_align_block"):
        assert re.search(r"\b%s\s*\(" % n, text), n
        assert hasattr(lib, n), n
    assert set(N.parse_header()) >= {"v100_ctc_align", "v100_ctc_align_workspace_bytes", "v100_ctc_align_block"}


def test_align_host_abi_without_a_device():
    _, lib = _lib()
    blk = lib.v100_ctc_align_block()
    assert 1 <= blk <= 4096
    ws = lib.v100_ctc_align_workspace_bytes
    assert ws(1, 1, 0) > 0
    base = ws(4, 100, 20)
    assert base >= 4 * 100 * 41                                          # one byte per frame and state at least
    assert ws(5, 100, 20) > base and ws(4, 101, 20) > base and ws(4, 100, 40) > base
    for B, T, L in [(1, 1, 1), (3, 50, 7), (32, 800, 200), (2, 12000, 2047)]:
        assert 0 < ws(B, T, L) <= ws(B + 1, T, L) and ws(B, T, L) <= ws(B, T + 1 if T < 12000 else T, L)
        assert ws(B, T, L) <= ws(B, T, min(L + 1, 2047))
    assert ws(0, 10, 5) == 0 and ws(1, 0, 5) == 0 and ws(1, 10, 2048) == 0 and ws(1, 12001, 5) == 0
    # the entry point checks its arguments before anything touches a device: host buffers stand in for the pointers
    bufs = [ctypes.create_string_buffer(64) for _ in range(9)]
    ptrs = [ctypes.addressof(b) for b in bufs]

    def call(p, B=1, T=4, V=29, Lmax=2, max_move=3):
        return lib.v100_ctc_align(*p, B, T, V, Lmax, max_move, None)
    for k in (0, 1, 4, 5, 6, 7, 8):                                      # every required pointer; in_len / lab_len may be NULL
        assert call(ptrs[:k] + [None] + ptrs[k + 1:]) == 3, k
    assert call([None] * 9) == 3
    assert call(ptrs, Lmax=2048) == 1                                    # 2 Lmax + 1 = 4097
    assert call(ptrs, max_move=0) == 1 and call(ptrs, max_move=9) == 1
    assert call(ptrs, T=12001) == 1 and call(ptrs, B=0) == 1 and call(ptrs, V=0) == 1


def test_align_records_on_hand_made_tensors():
    from voice100_amd.infer import align_records
    vocab = ["_", " ", "a", "b", "c"]

    def decode(ids):
        return "".join(vocab[int(x)] for x in ids if 0 <= int(x) < len(vocab))
    text = torch.tensor([[2, 3, 4], [4, 1, 0]])
    text_len = torch.tensor([3, 2])
    out = {"path": torch.tensor([[0, 2, 2, 3, 0, 4], [4, 4, 1, 0, 0, 0]]), "path_len": torch.tensor([6, 3]),
           "hist": torch.tensor([[0, 1, 1, 3, 4, 5], [1, 1, 3, 0, 0, 0]], dtype=torch.int32),
           "align": torch.tensor([[1, 2, 0, 1, 1, 1, 0], [0, 2, 0, 1, 0, 0, 0]], dtype=torch.int32)}
    assert align_records(out, text, text_len, decode) == ["abc|_aab_c|1 2 0 1 1 1 0", "c |cc |0 2 0 1 0"]
