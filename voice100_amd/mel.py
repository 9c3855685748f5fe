"""Log-mel front-end on the GPU (K7).  Drop-in arithmetic for MelSpectrogramAudioTransform
(voice100/data_modules.py:262-292): torchaudio-0.13.1 `MelSpectrogram(sample_rate=16000, n_fft=512,
win_length=400, hop_length=160, n_mels=64)` defaults (center, reflect pad, periodic Hann zero-padded to
n_fft, power 2, HTK mel scale, no norm) followed by log(mel.T + 1e-6).

The framed real DFT is a dense [2*257 x 400] x [400 x T] product (window folded into the basis) and the
filterbank a [64 x 257] x [257 x T] one; both run on the exact-fp32 MFMA GEMM kernel, with three small
HBM-bound kernels around them (framing, power, log+transpose).  A file path is decoded on the host by
audio_io.load_audio (WAV on the host, FLAC on the GPU) and brought to the module's rate on the GPU by audio_io.resample: no torchaudio.
PARITY UNPINNED against torchaudio itself (absent here): checked against oracle/mel.py and torch.stft.
"""
import math

import numpy as np
import torch
from torch import nn

from . import _native as N
from . import functional as F_

LOG_OFFSET = 1e-6
MELSPEC_DIM = 64


def _melscale_fbanks(n_freqs, f_min, f_max, n_mels, sample_rate):
    all_freqs = np.linspace(0, sample_rate // 2, n_freqs, dtype=np.float32)
    m_min = 2595.0 * math.log10(1.0 + f_min / 700.0)
    m_max = 2595.0 * math.log10(1.0 + f_max / 700.0)
    m_pts = np.linspace(np.float32(m_min), np.float32(m_max), n_mels + 2, dtype=np.float32)
    f_pts = (700.0 * (10.0 ** (m_pts / np.float32(2595.0)) - 1.0)).astype(np.float32)
    f_diff = f_pts[1:] - f_pts[:-1]
    slopes = f_pts[None, :] - all_freqs[:, None]
    down = -slopes[:, :-2] / f_diff[:-1]
    up = slopes[:, 2:] / f_diff[1:]
    return np.maximum(0.0, np.minimum(down, up)).astype(np.float32)        # [n_freqs, n_mels]


class MelSpectrogramAudioTransform(nn.Module):
    def __init__(self, sample_rate: int = 16000, n_fft: int = 512, win_length: int = 400, hop_length: int = 160,
                 n_mels: int = MELSPEC_DIM, log_offset: float = LOG_OFFSET) -> None:
        super().__init__()
        self.log_offset = log_offset
        self.sample_rate = sample_rate
        self.n_mels = n_mels
        self.n_fft, self.win_length, self.hop_length = n_fft, win_length, hop_length
        nf = n_fft // 2 + 1
        n = np.arange(win_length, dtype=np.float64)
        window = 0.5 - 0.5 * np.cos(2.0 * np.pi * n / win_length)              # periodic Hann
        left = (n_fft - win_length) // 2
        ang = 2.0 * np.pi * np.arange(nf, dtype=np.float64)[:, None] * (n[None, :] + left) / n_fft
        basis = np.concatenate([np.cos(ang) * window[None, :], -np.sin(ang) * window[None, :]], axis=0)
        self.register_buffer("dft_basis", torch.from_numpy(basis.astype(np.float32)), persistent=False)      # [2*nf, win]
        fb = _melscale_fbanks(nf, 0.0, sample_rate / 2.0, n_mels, sample_rate)
        self.register_buffer("mel_fb_t", torch.from_numpy(np.ascontiguousarray(fb.T)), persistent=False)      # [n_mels, nf]
        # tables of the one-launch kernel (csrc/mel.hip): n_fft = 512, <= 64 filters, each a contiguous run of <= 32 bins
        self.fused = False
        if n_fft == 512 and n_mels <= 64:
            starts, counts, wts, ok = np.zeros(n_mels, np.int32), np.zeros(n_mels, np.int32), np.zeros((n_mels, 32), np.float32), True
            for m in range(n_mels):
                nz = np.nonzero(fb[:, m])[0]
                if nz.size == 0:
                    continue
                lo, hi = int(nz[0]), int(nz[-1]) + 1
                if hi - lo > 32:
                    ok = False
                    break
                starts[m], counts[m] = lo, hi - lo
                wts[m, :hi - lo] = fb[lo:hi, m]                     # zeros inside the run (none for triangles) stay zero weights
            if ok:
                win512 = np.zeros(n_fft, dtype=np.float64)
                win512[left:left + win_length] = window
                k256, k512 = np.arange(256, dtype=np.float64), np.arange(257, dtype=np.float64)
                tw = lambda k, n_: np.stack([np.cos(2.0 * np.pi * k / n_), -np.sin(2.0 * np.pi * k / n_)], axis=1).astype(np.float32)
                self.register_buffer("_win512", torch.from_numpy(win512.astype(np.float32)), persistent=False)
                self.register_buffer("_tw256", torch.from_numpy(tw(k256, 256.0)), persistent=False)
                self.register_buffer("_tw512", torch.from_numpy(tw(k512, 512.0)), persistent=False)
                self.register_buffer("_mel_start", torch.from_numpy(starts), persistent=False)
                self.register_buffer("_mel_count", torch.from_numpy(counts), persistent=False)
                self.register_buffer("_mel_w", torch.from_numpy(wts), persistent=False)
                self.fused = True

    @property
    def audio_size(self) -> int:
        return self.n_mels

    def num_frames(self, n_samples):
        """Frames of an utterance of n_samples samples (an int, or a tensor of them: the result has its dtype and device)."""
        if isinstance(n_samples, torch.Tensor):
            return 1 + torch.div(n_samples, self.hop_length, rounding_mode="floor")
        return 1 + n_samples // self.hop_length

    def _host_lengths(self, lengths, B: int, n: int):
        """`lengths` as a tensor, its shape checked against the batch and, when it lives on the host, every entry against
        [n_fft / 2 + 1, n] (device lengths are not read back).  Returns (tensor, the longest entry or None)."""
        lens = torch.as_tensor(lengths)
        if lens.shape != (B,):
            raise ValueError(f"MelSpectrogramAudioTransform: lengths must be [{B}], got {tuple(lens.shape)}")
        if lens.dtype.is_floating_point or lens.dtype == torch.bool:
            raise ValueError(f"MelSpectrogramAudioTransform: lengths must be integers, got {lens.dtype}")
        if lens.is_cuda:
            return lens, None
        lo = self.n_fft // 2 + 1
        host = lens.tolist()
        for b, v in enumerate(host):
            if not lo <= v <= n:
                raise ValueError(f"MelSpectrogramAudioTransform: lengths[{b}] = {v} is outside [{lo}, {n}] (the reflect padding "
                                 f"needs more than n_fft / 2 = {self.n_fft // 2} samples, and the row holds {n})")
        return lens, max(host)

    @torch.no_grad()
    def transform(self, waveform: torch.Tensor, lengths=None, fused: bool = None):
        """waveform [N] or [B, N] fp32 on the GPU -> log-mel [T, n_mels] or [B, T, n_mels].  One launch (csrc/mel.hip: FFT per wave)
        for the reference's configuration; `fused=False` (or any other n_fft / filter count) takes the framing + DFT-GEMM +
        filterbank-GEMM kernels.

        With `lengths` ([B] integers, CPU or device) every row of waveform [B, N] is an utterance of its own length and the result is
        (audio [B, T, n_mels] fp32, audio_len [B] int32 on the device), the batch the reference's collate builds
        (generate_audio_text_batch, data_modules.py:446-455): row b's first audio_len[b] = 1 + lengths[b] // hop frames are those of
        transform(waveform[b, :lengths[b]]), bit for bit (the reflection is taken at the utterance's own end), the rest is
        log(log_offset), and what the waveform holds beyond lengths[b] is never read.  One launch; fused kernel only
        (NotImplementedError with fused=False or a configuration without it).
          * CPU lengths are checked (each in [n_fft / 2 + 1, N], ValueError naming the row otherwise -- torch's reflect pad raises
            there too) and the batch is as wide as its longest utterance, T = 1 + max(lengths) // hop (pad_sequence's width).
          * Device lengths are not read back: T = 1 + N // hop, entries are clamped to [0, N], and a row with
            lengths[b] <= n_fft / 2 comes back all log(log_offset) with audio_len[b] = 0."""
        if lengths is not None:
            return self._transform_ragged(waveform, lengths, fused)
        squeeze = waveform.dim() == 1
        x = waveform[None] if squeeze else waveform
        F_._check(x, "MelSpectrogramAudioTransform")
        x = x.contiguous()
        B, n = x.shape
        T = self.num_frames(n)
        nf = self.n_fft // 2 + 1
        if self.fused if fused is None else (fused and self.fused):
            out = torch.empty((B, T, self.n_mels), dtype=torch.float32, device=x.device)
            N.call("v100_log_mel_fused", x, out, self._win512, self._tw256, self._tw512, self._mel_start, self._mel_count, self._mel_w,
                   B, n, T, self.hop_length, self.n_fft, self.n_mels, float(self.log_offset))
            return out[0] if squeeze else out
        frames = torch.empty((B, self.win_length, T), dtype=torch.float32, device=x.device)
        N.call("v100_stft_frames", x, frames, B, n, T, self.hop_length, self.win_length, self.n_fft)
        spec = torch.empty((B, 2 * nf, T), dtype=torch.float32, device=x.device)
        F_._pw_gemm(self.dft_basis, None, frames, spec, 2 * nf, self.win_length, T, B, False)     # exact-fp32 MFMA
        power = torch.empty((B, nf, T), dtype=torch.float32, device=x.device)
        N.call("v100_power_spectrum", spec, power, B, nf, T)
        mel = torch.empty((B, self.n_mels, T), dtype=torch.float32, device=x.device)
        F_._pw_gemm(self.mel_fb_t, None, power, mel, self.n_mels, nf, T, B, False)
        out = torch.empty((B, T, self.n_mels), dtype=torch.float32, device=x.device)
        N.call("v100_log_transpose", mel, out, B, self.n_mels, T, float(self.log_offset))
        return out[0] if squeeze else out

    def _transform_ragged(self, waveform, lengths, fused):
        if waveform.dim() != 2 or waveform.shape[0] < 1:
            raise ValueError(f"MelSpectrogramAudioTransform: lengths need a [B, N] waveform, B >= 1, got {tuple(waveform.shape)}")
        B, n = waveform.shape
        lens, longest = self._host_lengths(lengths, B, n)               # before any device work
        if fused is False or not self.fused:
            raise NotImplementedError("MelSpectrogramAudioTransform: lengths are served by the one-launch kernel only "
                                      "(n_fft = 512, <= 64 filters of <= 32 bins; not with fused=False)")
        F_._check(waveform, "MelSpectrogramAudioTransform")
        x = waveform.contiguous()
        T = self.num_frames(n if longest is None else longest)
        lens = lens.to(x.device, torch.int32).contiguous()
        out = torch.empty((B, T, self.n_mels), dtype=torch.float32, device=x.device)
        out_len = torch.empty((B,), dtype=torch.int32, device=x.device)
        with torch.cuda.device(x.device):
            N.call("v100_log_mel_fused_len", x, lens, out, out_len, self._win512, self._tw256, self._tw512, self._mel_start,
                   self._mel_count, self._mel_w, B, n, T, self.hop_length, self.n_fft, self.n_mels, float(self.log_offset),
                   float(math.log(self.log_offset)))
        return out, out_len

    def forward(self, audio):
        """A path to a WAV or FLAC file (as in the reference: load, first channel, resample to the module's rate, transform) or an
        already-loaded waveform tensor.  A list or tuple of paths gives the padded batch and its lengths,
        transform(*audio_io.load_batch(paths, sample_rate)).  The module must be on the GPU: the resampling runs there too."""
        if isinstance(audio, torch.Tensor):
            return self.transform(audio)
        from .audio_io import load_audio, load_batch, resample
        if isinstance(audio, (list, tuple)):
            return self.transform(*load_batch(audio, self.sample_rate, self.dft_basis.device))
        waveform, sr = load_audio(audio)
        return self.transform(resample(waveform[0].to(self.dft_basis.device), sr, self.sample_rate))
