"""Host side of the ragged front-end: frame counts, the length checks of transform(waveform, lengths) (raised before any device
work, so they hold on a machine without a GPU too), the constants of the collate, and the refusal to run without a device."""
import math

import pytest
import torch

from voice100_amd import data
from voice100_amd.audio_io import load_batch
from voice100_amd.mel import MelSpectrogramAudioTransform


def test_num_frames_on_ints_and_tensors():
    tr = MelSpectrogramAudioTransform()
    assert [tr.num_frames(n) for n in (0, 159, 160, 257, 1600, 16000)] == [1, 1, 2, 2, 11, 101]
    for dtype in (torch.int32, torch.int64):
        n = torch.tensor([159, 160, 257, 319, 320, 1600], dtype=dtype)
        got = tr.num_frames(n)
        assert got.dtype == dtype and got.tolist() == [1, 2, 2, 2, 3, 11]
    assert MelSpectrogramAudioTransform(hop_length=128).num_frames(torch.tensor([1024])).tolist() == [9]


def test_blank_constants_are_the_reference_s():
    assert data.BLANK_IDX == 0
    assert data.BLANK_AUDIO == math.log(1e-6)
    # what pad_sequence writes into a float32 batch, and what the kernel is handed as `fill`
    assert torch.tensor(data.BLANK_AUDIO, dtype=torch.float32).item() == torch.full((1,), math.log(1e-6)).item()


def test_host_lengths_are_checked_before_any_device_work():
    tr = MelSpectrogramAudioTransform()
    x = torch.zeros(3, 1600)                        # a CPU tensor: a call that got past the checks would raise RuntimeError
    with pytest.raises(ValueError, match=r"lengths\[2\] = 256 is outside \[257, 1600\]"):
        tr.transform(x, [1600, 257, 256])
    with pytest.raises(ValueError, match=r"lengths\[1\] = 1601 is outside \[257, 1600\]"):
        tr.transform(x, torch.tensor([300, 1601, 300]))
    with pytest.raises(ValueError, match=r"lengths\[0\] = -1 is outside"):
        tr.transform(x, [-1, 300, 300])
    with pytest.raises(ValueError, match=r"lengths must be \[3\], got \(2,\)"):
        tr.transform(x, [300, 300])
    with pytest.raises(ValueError, match="lengths must be integers"):
        tr.transform(x, torch.tensor([300.0, 300.0, 300.0]))
    with pytest.raises(ValueError, match=r"\[B, N\] waveform"):
        tr.transform(torch.zeros(1600), [1600])
    with pytest.raises(NotImplementedError):
        tr.transform(x, [300, 300, 300], fused=False)
    with pytest.raises(NotImplementedError):
        MelSpectrogramAudioTransform(n_fft=400).transform(x, [300, 300, 300])
    with pytest.raises(RuntimeError, match="GPU only"):            # valid lengths: the tensor itself is refused, as without lengths
        tr.transform(x, [300, 1600, 257])
    with pytest.raises(RuntimeError, match="GPU only"):
        tr.transform(x)


def test_loader_and_collate_are_gpu_only(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)       # the same answer on a machine that has a device
    tr = MelSpectrogramAudioTransform()
    with pytest.raises(RuntimeError, match="GPU only"):
        load_batch([str(tmp_path / "missing.wav")], 16000)
    with pytest.raises(RuntimeError, match="GPU only"):
        data.AudioTextCollate(tr)([(torch.zeros(1600), torch.tensor([1, 2]))])
    with pytest.raises(RuntimeError, match="GPU only"):
        tr([str(tmp_path / "missing.wav")])


def test_ragged_entry_reports_null_and_shape_before_any_launch():
    import ctypes
    from voice100_amd import _native as N
    lib = N.load()
    one = ctypes.c_void_p(16)
    tables = (one,) * 6
    ok = (2, 1600, 11, 160, 512, 64, 1e-6, math.log(1e-6), None)
    assert lib.v100_log_mel_fused_len(one, None, one, one, *tables, *ok) == 3             # lengths
    assert lib.v100_log_mel_fused_len(one, one, one, None, *tables, *ok) == 3             # out_len
    assert lib.v100_log_mel_fused_len(None, one, one, one, *tables, *ok) == 3
    for bad in ((0, 1600, 11, 160, 512, 64), (2, 256, 1, 160, 512, 64), (2, 1600, 12, 160, 512, 64), (2, 1600, 11, 160, 400, 64),
                (2, 1600, 11, 160, 512, 65), (2, 1600, 0, 160, 512, 64)):
        assert lib.v100_log_mel_fused_len(one, one, one, one, *tables, *bad, 1e-6, math.log(1e-6), None) == 1, bad
