"""The ragged log-mel launch (v100_log_mel_fused_len, csrc/mel.hip): a padded batch of utterances of different lengths gives what
the reference's collate builds (generate_audio_text_batch, data_modules.py:446-455) -- every utterance transformed ALONE, then
pad_sequence with log(1e-6).

Bars.  The frames of an utterance are compared with transform(x[b, :n]), the dense entry point on the utterance alone: the same
instruction sequence on the same samples, so bit equality (torch.equal).  Against oracle/mel.py (float64 FFT) the project's fp32
bar, conftest.rel_err < 1e-4.  The padding is compared exactly with the float32 value of math.log(1e-6), what pad_sequence writes.
Samples beyond each row's length are NaN: a NaN anywhere in the output would show that one was read.
"""
import math

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import mel as oracle_mel
from voice100_amd.mel import MelSpectrogramAudioTransform

pytestmark = pytest.mark.gpu

HOP = 160
FILL = torch.tensor(math.log(1e-6), dtype=torch.float32)
EDGES = [257, 319, 320, 321, 479, 480, 511, 512, 513, 799, 800, 1599, 1600]


@pytest.fixture(scope="module")
def tr(cuda):
    return MelSpectrogramAudioTransform().to(cuda)


def batch(cuda, lengths, N, seed):
    """[B, N] seeded randn * 0.1 on the device, NaN beyond each row's length."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(len(lengths), N, generator=gen) * 0.1
    for b, n in enumerate(lengths):
        x[b, n:] = float("nan")
    return x.to(cuda)


def check_rows(tr, x, lengths, out, out_len, rows, oracle=True):
    T = out.shape[1]
    fill = FILL.to(out.device)
    for b in rows:
        n = int(lengths[b])
        Tb = 1 + n // HOP
        assert int(out_len[b]) == Tb, (b, n)
        alone = tr.transform(x[b, :n])
        assert alone.shape == (Tb, out.shape[2])
        assert torch.equal(out[b, :Tb], alone), (b, n, float((out[b, :Tb] - alone).abs().max()))
        if oracle:
            ref = oracle_mel.log_mel(x[b, :n].cpu().numpy(), n_mels=out.shape[2])
            assert ref.shape[0] == Tb
            e = rel_err(out[b, :Tb], ref)
            print(f"row {b} n {n}: rel_err vs float64 oracle {e:.3e}")
            assert e < 1e-4, (b, n, e)
        assert torch.equal(out[b, Tb:], fill.expand(T - Tb, out.shape[2])), (b, n)


def test_every_edge_of_the_length_rule(tr, cuda):
    N = 1600
    x = batch(cuda, EDGES, N, 0)
    out, out_len = tr.transform(x, torch.tensor(EDGES))
    assert out.shape == (len(EDGES), 1 + N // HOP, 64) and out.dtype == torch.float32
    assert out_len.dtype == torch.int32 and out_len.device == out.device and out_len.shape == (len(EDGES),)
    assert out_len.tolist() == [1 + n // HOP for n in EDGES]
    assert not torch.isnan(out).any()
    check_rows(tr, x, EDGES, out, out_len, range(len(EDGES)))


def test_width_follows_the_longest_utterance_for_host_lengths(tr, cuda):
    lengths = [800, 400]
    x = batch(cuda, lengths, 2000, 1)
    host, host_len = tr.transform(x, lengths)
    assert host.shape == (2, 6, 64)
    dev, dev_len = tr.transform(x, torch.tensor(lengths, device=cuda))
    assert dev.shape == (2, 13, 64)
    assert torch.equal(host_len, dev_len) and host_len.tolist() == [6, 3]
    assert torch.equal(dev[:, :6], host)
    assert torch.equal(dev[:, 6:], FILL.to(cuda).expand(2, 7, 64))
    check_rows(tr, x, lengths, host, host_len, range(2), oracle=False)
    # int32 / int64, list or tensor: the same call
    again, again_len = tr.transform(x, torch.tensor(lengths, dtype=torch.int32))
    assert torch.equal(again, host) and torch.equal(again_len, host_len)


def test_grid_stride_second_trip(tr, cuda):
    B, N = 64, 48000
    gen = torch.Generator().manual_seed(2)
    lengths = torch.randint(257, N + 1, (B,), generator=gen).tolist()
    lengths[5], lengths[40] = N, 257
    assert B * (1 + N // HOP) == 19264 > 4 * 4096                # more frames than one pass of the grid's waves
    x = batch(cuda, lengths, N, 3)
    out, out_len = tr.transform(x, lengths)
    assert out.shape == (B, 301, 64)
    assert out_len.tolist() == [1 + n // HOP for n in lengths]
    assert not torch.isnan(out).any()
    check_rows(tr, x, lengths, out, out_len, [0, 5, 17, 31, 40, 47, 62, 63])


def test_full_rows_equal_the_dense_transform(tr, cuda):
    gen = torch.Generator().manual_seed(4)
    x = (torch.randn(5, 16000, generator=gen) * 0.1).to(cuda)
    out, out_len = tr.transform(x, [16000] * 5)
    assert torch.equal(out, tr.transform(x))
    assert out_len.tolist() == [101] * 5
    dev, dev_len = tr.transform(x, torch.full((5,), 16000, dtype=torch.int64, device=cuda))
    assert torch.equal(dev, out) and torch.equal(dev_len, out_len)


def test_forty_filters(cuda):
    tr40 = MelSpectrogramAudioTransform(n_mels=40).to(cuda)
    assert tr40.fused
    lengths = [1000, 257, 1600, 640]
    x = batch(cuda, lengths, 1600, 5)
    out, out_len = tr40.transform(x, lengths)
    assert out.shape == (4, 11, 40)
    assert not torch.isnan(out).any()
    check_rows(tr40, x, lengths, out, out_len, range(4))


def test_errors_and_the_degenerate_row(tr, cuda):
    x = batch(cuda, [1600, 1600], 1600, 6)
    with pytest.raises(ValueError, match=r"lengths\[1\] = 256"):
        tr.transform(x, [1600, 256])
    with pytest.raises(ValueError, match=r"lengths\[0\] = 1601"):
        tr.transform(x, [1601, 300])
    with pytest.raises(ValueError, match="lengths must be"):
        tr.transform(x, [300, 300, 300])
    with pytest.raises(ValueError, match="lengths must be"):
        tr.transform(x, torch.tensor([[300, 300]]))
    with pytest.raises(NotImplementedError):
        tr.transform(x, [300, 300], fused=False)
    odd = MelSpectrogramAudioTransform(n_fft=400).to(cuda)            # a configuration without the one-launch kernel
    assert not odd.fused
    with pytest.raises(NotImplementedError):
        odd.transform(x, [300, 300])
    # device lengths are not read back: a row too short for the reflect padding is all padding, length 0 (nothing of it is loaded)
    y = batch(cuda, [100, 700], 1600, 7)
    out, out_len = tr.transform(y, torch.tensor([100, 700], device=cuda))
    assert out_len.tolist() == [0, 5]
    assert torch.equal(out[0], FILL.to(cuda).expand(11, 64))
    assert torch.equal(out[1, :5], tr.transform(y[1, :700])) and not torch.isnan(out).any()
