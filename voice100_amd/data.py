"""The collates on the device.  AudioTextCollate: a list of (audio, text) items -> the batch AudioToTextCTC, AudioAlignCTC,
AudioToAlignText and AlignPipeline consume.  WorldAlignTextCollate: (audio, aligntext[, targettext]) items -> the WORLD-feature batch of
the TTS models.

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

__all__ = ["BLANK_IDX", "BLANK_AUDIO", "AudioTextCollate", "WorldAlignTextCollate"]


def _waveforms(audios, sample_rate, device, who):
    """(wave [B, N] fp32 on the device, zero beyond each utterance, lengths [B]): lengths on the host for tensors (known without
    a read-back), on the device for files (the resampler wrote them)."""
    from .audio_io import load_batch
    is_path = [isinstance(a, (str, os.PathLike)) for a in audios]
    if all(is_path):
        return load_batch(audios, sample_rate, device)
    for a in audios:
        if not isinstance(a, (str, os.PathLike)) and not (isinstance(a, torch.Tensor) and a.dim() == 1):
            raise ValueError(f"{who}: audio must be a path or a waveform tensor [samples]")
    tensors = [(i, a) for i, a in enumerate(audios) if not is_path[i]]
    lens = torch.tensor([a.shape[0] for _, a in tensors], dtype=torch.int32)
    if all(not a.is_cuda for _, a in tensors):                                # one padded block, one host-to-device copy
        block = pad_sequence([a.to(torch.float32) for _, a in tensors], batch_first=True).to(device)
    else:
        block = pad_sequence([a.to(device, torch.float32) for _, a in tensors], batch_first=True)
    if len(tensors) == len(audios):
        return block, lens
    rows = [i for i, p in enumerate(is_path) if p]
    wave_p, len_p = load_batch([audios[i] for i in rows], sample_rate, device)
    wave = torch.zeros((len(audios), max(block.shape[1], wave_p.shape[1])), dtype=torch.float32, device=device)
    wave_len = torch.empty((len(audios),), dtype=torch.int32, device=device)
    for idx, w, n in ((rows, wave_p, len_p), ([i for i, _ in tensors], block, lens.to(device))):
        idx = torch.tensor(idx, dtype=torch.int64, device=device)
        wave[:, :w.shape[1]].index_copy_(0, idx, w)
        wave_len.index_copy_(0, idx, n)
    return wave, wave_len


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
        return _waveforms(audios, self.mel.sample_rate, device, "AudioTextCollate")

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


def _is_triple(a) -> bool:
    return isinstance(a, (tuple, list)) and len(a) == 3 and all(isinstance(t, torch.Tensor) for t in a)


class WorldAlignTextCollate:
    """collate_fn of the TTS models: the device counterpart of generate_audio_text_align_batch and
    generate_audio_text_align_target_batch (data_modules.py:458-496).

        WorldAlignTextCollate(vocoder)(items)

    items are all `(audio, aligntext)` or all `(audio, aligntext, targettext)` (a mix raises ValueError) and give

        ((f0 [B, T] fp32, f0_len [B] int32, spec [B, T, D] fp32, codeap [B, T, nb] fp32), (text [B, L] int64, text_len [B] int32))

    plus `(target [B, Lt] int64, target_len [B] int32)` for three-part items: the batches AlignTextToAudioModel and
    AlignTextToAudioMultiTaskModel train on.  Features are padded with 0, ids with BLANK_IDX; dtypes are the reference's.
    `audio` is, the same for every item of a batch, one of

    * a path to a WAV or FLAC file: audio_io.load_batch, then ONE WORLDVocoder.encode_batch(wave, wave_len) over the whole batch;
    * a 1-D waveform tensor at the vocoder's sample rate: padded to one block, then the same call;
    * an already computed `(f0 [T], spec [T, D], codeap [T, nb])` triple -- what the reference's feature cache hands its collate.
      This path is pure pad_sequence, needs no GPU and leaves the batch where the tensors are.

    For waveforms f0_len is vocoder.frames(samples) per utterance and T the longest utterance's frame count (the lengths are read
    back once, as align_expand does); the batch is on the current GPU.  Without a GPU the waveform paths raise RuntimeError.

    Out of scope: the reference cache's lossy mel-cepstrum round trip for the `world` vocoder (data_modules.py:221-232: the stored
    features are mcep, expanded back to a log spectrum on load).  It is two existing GEMMs a caller can apply to `spec`
    (WORLDVocoder.logspc_to_mcep, then mcep_to_logspc)."""

    def __init__(self, processor):
        self.processor = processor

    def _features(self, audios):
        """(f0, f0_len, spec, codeap) from waveforms or files, on the device."""
        if not torch.cuda.is_available():
            raise RuntimeError("WorldAlignTextCollate: voice100_amd runs on the GPU only (no CPU fallback): the WORLD analysis kernels run "
                               "on the device (only already computed (f0, spec, codeap) triples collate without one)")
        v = self.processor
        device = torch.device("cuda", torch.cuda.current_device())
        wave, wave_len = _waveforms(audios, v.sample_rate, device, "WorldAlignTextCollate")
        lens = [int(n) for n in wave_len.tolist()]                 # the one read-back (none for tensors: those lengths are on the host)
        wave = wave[:, :max(lens)].contiguous()                    # T = frames(longest utterance), whatever the block was padded to
        f0, spec, codeap = v.encode_batch(wave, wave_len)
        f0_len = torch.tensor([v.frames(n) for n in lens], dtype=torch.int32, device=device)
        return f0, f0_len, spec, codeap

    def __call__(self, items):
        items = [tuple(it) for it in items]
        if not items:
            raise ValueError("WorldAlignTextCollate: no items")
        width = len(items[0])
        if width not in (2, 3) or any(len(it) != width for it in items):
            raise ValueError("WorldAlignTextCollate: items must be all (audio, aligntext) or all (audio, aligntext, targettext)")
        audios = [it[0] for it in items]
        triples = [_is_triple(a) for a in audios]
        if any(triples) and not all(triples):
            raise ValueError("WorldAlignTextCollate: (f0, spec, codeap) triples and waveforms / paths cannot be mixed in one batch")
        texts = [[torch.as_tensor(it[k]) for it in items] for k in range(1, width)]
        if any(t.dim() != 1 or t.dtype.is_floating_point for ts in texts for t in ts):
            raise ValueError("WorldAlignTextCollate: text ids must be 1-D integer tensors")
        if all(triples):
            if any(a[0].dim() != 1 or a[1].dim() != 2 or a[2].dim() != 2 or not a[0].shape[0] == a[1].shape[0] == a[2].shape[0]
                   for a in audios):
                raise ValueError("WorldAlignTextCollate: a feature triple is (f0 [T], spec [T, D], codeap [T, nb]) with one T")
            device = audios[0][0].device
            f0_len = torch.tensor([a[0].shape[0] for a in audios], dtype=torch.int32, device=device)
            f0, spec, codeap = (pad_sequence([a[k] for a in audios], batch_first=True, padding_value=0) for k in range(3))
        else:
            f0, f0_len, spec, codeap = self._features(audios)
            device = f0.device
        out = [(f0, f0_len, spec, codeap)]
        for ts in texts:
            n = torch.tensor([t.shape[0] for t in ts], dtype=torch.int32)
            ids = pad_sequence([t.to(torch.int64) for t in ts], batch_first=True, padding_value=BLANK_IDX)
            out.append((ids.to(device), n.to(device)))
        return tuple(out)
