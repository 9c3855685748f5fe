"""The ASR collate on the device: a list of (audio, text) items -> the batch AudioToTextCTC, AudioAlignCTC, AudioToAlignText
and AlignPipeline consume.

The reference's dataset runs MelSpectrogramAudioTransform on every utterance alone and its collate pads the results
(generate_audio_text_batch, voice100/data_modules.py:446-455: audio with BLANK_AUDIO, text with BLANK_IDX, lengths int32).  Here the
waveforms of a batch are padded first and ONE launch (transform(wave, wave_len), csrc/mel.hip) gives the same padded log-mel batch:
each utterance's frames are those of the utterance alone, the rest is BLANK_AUDIO.  The text side is the stock pad_sequence.
"""
import math
import os

import torch
from torch.nn.utils.rnn import pad_sequence

BLANK_IDX = 0
BLANK_AUDIO = math.log(1e-6)

__all__ = ["BLANK_IDX", "BLANK_AUDIO", "AudioTextCollate"]


class AudioTextCollate:
    """collate_fn for (audio, text ids) items.  `audio` is a path to a WAV file (loaded and brought to the transform's rate by
    audio_io.load_batch) or a waveform tensor [samples] already at that rate (CPU or device); `text ids` is a 1-D integer tensor.

        AudioTextCollate(mel)(items) -> ((audio [B, T, n_mels] fp32, audio_len [B] int32), (text [B, L] int64, text_len [B] int32))

    all on the transform's device, T = 1 + (longest utterance) // hop and L the longest text: layout, dtypes and padding values of
    data_modules.py:446-455, a batch TrainStep(AudioToTextCTC(...)) takes as it is.  `mel` is a MelSpectrogramAudioTransform on the
    GPU whose log_offset gives the audio padding (BLANK_AUDIO for the reference's 1e-6)."""

    def __init__(self, mel):
        self.mel = mel

    def _waveforms(self, audios, device):
        """(wave [B, N] fp32 on the device, zero beyond each utterance, lengths [B]): lengths on the host for tensors (known without
        a read-back), on the device for files (the resampler wrote them)."""
        from .audio_io import load_batch
        is_path = [isinstance(a, (str, os.PathLike)) for a in audios]
        if all(is_path):
            return load_batch(audios, self.mel.sample_rate, device)
        for a in audios:
            if not isinstance(a, (str, os.PathLike)) and not (isinstance(a, torch.Tensor) and a.dim() == 1):
                raise ValueError("AudioTextCollate: audio must be a path or a waveform tensor [samples]")
        tensors = [(i, a) for i, a in enumerate(audios) if not is_path[i]]
        lens = torch.tensor([a.shape[0] for _, a in tensors], dtype=torch.int32)
        if all(not a.is_cuda for _, a in tensors):                                # one padded block, one host-to-device copy
            block = pad_sequence([a.to(torch.float32) for _, a in tensors], batch_first=True).to(device)
        else:
            block = pad_sequence([a.to(device, torch.float32) for _, a in tensors], batch_first=True)
        if len(tensors) == len(audios):
            return block, lens
        rows = [i for i, p in enumerate(is_path) if p]
        wave_p, len_p = load_batch([audios[i] for i in rows], self.mel.sample_rate, device)
        wave = torch.zeros((len(audios), max(block.shape[1], wave_p.shape[1])), dtype=torch.float32, device=device)
        wave_len = torch.empty((len(audios),), dtype=torch.int32, device=device)
        for idx, w, n in ((rows, wave_p, len_p), ([i for i, _ in tensors], block, lens.to(device))):
            idx = torch.tensor(idx, dtype=torch.int64, device=device)
            wave[:, :w.shape[1]].index_copy_(0, idx, w)
            wave_len.index_copy_(0, idx, n)
        return wave, wave_len

    def __call__(self, items):
        if not torch.cuda.is_available():
            raise RuntimeError("AudioTextCollate: voice100_amd runs on the GPU only (no CPU fallback): the log-mel kernel runs on the device")
        items = list(items)
        if not items:
            raise ValueError("AudioTextCollate: no items")
        device = self.mel.dft_basis.device
        if device.type != "cuda":
            raise RuntimeError(f"AudioTextCollate: the transform is on {device}; voice100_amd runs on the GPU only (mel.to('cuda'))")
        texts = [torch.as_tensor(t) for _, t in items]
        if any(t.dim() != 1 or t.dtype.is_floating_point for t in texts):
            raise ValueError("AudioTextCollate: text ids must be 1-D integer tensors")
        wave, wave_len = self._waveforms([a for a, _ in items], device)
        audio, audio_len = self.mel.transform(wave, wave_len)
        text_len = torch.tensor([t.shape[0] for t in texts], dtype=torch.int32)
        text = pad_sequence([t.to(torch.int64) for t in texts], batch_first=True, padding_value=BLANK_IDX)
        return (audio, audio_len), (text.to(device), text_len.to(device))
