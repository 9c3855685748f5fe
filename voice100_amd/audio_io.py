"""From an audio file to a waveform at the model's rate, without torchaudio: a RIFF/WAVE reader on the host and
`torchaudio.functional.resample`'s default method on the GPU (csrc/resample.hip).

The reference opens files with `torchaudio.load` + `torchaudio.functional.resample` (data_modules.py:287-292) or with sox effects
(`remix 1`, `rate`: data_modules.py:295-316).  `load_wav` returns what `torchaudio.load` returns for a WAV file with its defaults;
`resample` follows the published definition of `sinc_interpolation` with a Hann window, its filter bank built in float64 and
rounded to float32 once (torchaudio builds it in float32: a few ulps per tap apart).  PARITY UNPINNED against torchaudio itself
(absent here): checked against a float64 restatement of that definition.  FLAC (LibriSpeech) and every compressed format are out
of scope -- decode those with a decoder of your own and pass the tensor.
"""
import math
import struct
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch
from torch import nn

from . import _native as N
from . import functional as F_

_PCM, _FLOAT, _EXTENSIBLE = 0x0001, 0x0003, 0xFFFE
_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")      # KSDATAFORMAT_SUBTYPE_*: the format tag, then these 14 bytes


def _decode(raw: np.ndarray, tag: int, bits: int, what: str) -> np.ndarray:
    """Interleaved little-endian samples (a uint8 array holding whole samples) -> float32, torchaudio's normalisation."""
    if tag == _PCM and bits == 8:
        return (raw.astype(np.float32) - 128.0) / 128.0
    if tag == _PCM and bits == 16:
        return raw.view("<i2").astype(np.float32) / 32768.0
    if tag == _PCM and bits == 24:
        b = raw.reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = (v ^ 0x800000) - 0x800000                                 # sign extension
        return v.astype(np.float32) / 8388608.0
    if tag == _PCM and bits == 32:
        return (raw.view("<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
    if tag == _FLOAT and bits == 32:
        return raw.view("<f4").astype(np.float32)
    if tag == _FLOAT and bits == 64:
        return raw.view("<f8").astype(np.float32)
    raise ValueError(f"{what}: unsupported WAV sample format (format tag 0x{tag:04x}, {bits} bits per sample); "
                     "supported: PCM 8/16/24/32-bit and IEEE float 32/64-bit")


def load_wav(path):
    """(waveform [channels, frames] float32 CPU tensor, sample_rate): `torchaudio.load(path)` with its defaults, for a WAV file.

    PCM unsigned 8-bit ((v - 128) / 128), PCM 16 / 24 / 32-bit (v / 2^15, 2^23, 2^31), IEEE float 32 / 64-bit, plain or inside
    WAVE_FORMAT_EXTENSIBLE.  Chunks other than `fmt ` and `data` are skipped (odd sizes padded to even, as RIFF says); a `data`
    chunk that claims more bytes than the file holds (a streaming writer that never went back to the header) gives the frames
    that are there.  Anything else -- a compressed format, FLAC, a file that is not RIFF/WAVE -- is a ValueError naming what was
    found."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file (it begins {data[:4]!r} ... {data[8:12]!r}); "
                         "only WAV is read here (FLAC and other containers need a decoder of yours)")
    pos, fmt = 12, None
    while pos + 8 <= len(data):
        cid, size = data[pos:pos + 4], struct.unpack_from("<I", data, pos + 4)[0]
        body = pos + 8
        if cid == b"fmt ":
            if size < 16 or body + size > len(data):
                raise ValueError(f"{path}: truncated or short `fmt ` chunk ({size} bytes declared, {len(data) - body} in the file)")
            tag, channels, rate, _, _, bits = struct.unpack_from("<HHIIHH", data, body)
            if tag == _EXTENSIBLE:
                if size < 40:
                    raise ValueError(f"{path}: WAVE_FORMAT_EXTENSIBLE with a {size}-byte `fmt ` chunk (40 needed)")
                guid = data[body + 24:body + 40]
                if guid[2:] != _GUID_TAIL:
                    raise ValueError(f"{path}: WAVE_FORMAT_EXTENSIBLE with an unknown sub-format {guid.hex()}")
                tag = struct.unpack_from("<H", guid)[0]
            if channels < 1 or rate < 1:
                raise ValueError(f"{path}: `fmt ` chunk with {channels} channels at {rate} Hz")
            fmt = (tag, channels, rate, bits)
        elif cid == b"data":
            if fmt is None:
                raise ValueError(f"{path}: `data` chunk before any `fmt ` chunk")
            tag, channels, rate, bits = fmt
            if bits < 8 or bits % 8:
                raise ValueError(f"{path}: unsupported WAV sample format (format tag 0x{tag:04x}, {bits} bits per sample)")
            frame = channels * (bits // 8)
            frames = min(size, len(data) - body) // frame
            raw = np.frombuffer(data, dtype=np.uint8, count=frames * frame, offset=body)
            samples = _decode(raw, tag, bits, str(path))
            return torch.from_numpy(np.ascontiguousarray(samples.reshape(frames, channels).T)), int(rate)
        pos = body + size + (size & 1)
    raise ValueError(f"{path}: RIFF/WAVE file without a `data` chunk" + ("" if fmt else " or a `fmt ` chunk") + " (truncated?)")


# ---- the filter bank --------------------------------------------------------------------------------------------------------
ResampleKernel = namedtuple("ResampleKernel", "o n width L dense starts taps")
ResampleKernel.__doc__ = """The polyphase bank of one rate pair, reduced to o / n: `dense` [n, 2 width + o] float32 (the table
torchaudio convolves with), and the compact form the kernel takes -- `starts` [n] int32, `taps` [n, L] float32 with
taps[p] = dense[p, starts[p]:starts[p] + L] (zero where that passes the end of the dense row), L = 2 width + 2."""


def _rates(orig_freq, new_freq):
    for f in (orig_freq, new_freq):
        if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)) or f != int(f) or f <= 0:
            raise ValueError(f"resample: sample rates must be positive integers (got {orig_freq!r} -> {new_freq!r})")
    o, n = int(orig_freq), int(new_freq)
    g = math.gcd(o, n)
    return o // g, n // g


@lru_cache(maxsize=None)
def _bank(o: int, n: int, lpw: int, rolloff: float) -> ResampleKernel:
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    j = np.arange(2 * width + o, dtype=np.float64)
    p = np.arange(n, dtype=np.float64)
    t = np.clip((-p[:, None] / n + (j[None, :] - width) / o) * base, -lpw, lpw)
    window = np.cos(t * np.pi / lpw / 2.0) ** 2
    t = t * np.pi
    safe = np.where(t == 0.0, 1.0, t)
    dense = (np.where(t == 0.0, 1.0, np.sin(safe) / safe) * window * (base / o)).astype(np.float32)
    # |t| < lpw only where |j - width - p o / n| < lpw o / base <= width: at most 2 width + 1 taps, from floor(p o / n) on
    L = 2 * width + 2
    starts = (np.arange(n, dtype=np.int64) * o // n).astype(np.int32)
    padded = np.concatenate([dense, np.zeros((n, L), np.float32)], axis=1)
    taps = np.stack([padded[q, s:s + L] for q, s in enumerate(starts)])
    for a in (dense, starts, taps):
        a.setflags(write=False)
    return ResampleKernel(o, n, width, L, dense, starts, taps)


def resample_kernel(orig_freq, new_freq, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> ResampleKernel:
    """The filter bank of `torchaudio.functional.resample(..., resampling_method="sinc_interpolation")` (Hann window), computed in
    float64 and rounded to float32 once.  With o, n = the rates over their gcd, base = min(o, n) rolloff and
    width = ceil(lowpass_filter_width o / base):  t = clip((-p / n + (j - width) / o) base, +-lowpass_filter_width),
    K[p][j] = sinc(pi t) cos^2(pi t / (2 lowpass_filter_width)) base / o  for phase p < n and tap j < 2 width + o."""
    o, n = _rates(orig_freq, new_freq)
    if int(lowpass_filter_width) != lowpass_filter_width or lowpass_filter_width < 1:
        raise ValueError(f"resample: lowpass_filter_width must be a positive integer (got {lowpass_filter_width!r})")
    if not 0.0 < rolloff <= 1.0:
        raise ValueError(f"resample: rolloff must be in (0, 1] (got {rolloff!r})")
    return _bank(o, n, int(lowpass_filter_width), float(rolloff))


_device_banks = {}


def _device_bank(k: ResampleKernel, lpw: int, rolloff: float, device):
    key = (k.o, k.n, lpw, rolloff, device)
    ent = _device_banks.get(key)
    if ent is None:
        ent = _device_banks[key] = (torch.tensor(k.taps, device=device), torch.tensor(k.starts, device=device))
    return ent


def resample_tile() -> int:
    """Outputs one workgroup of the resampling kernel serves (the tests put utterance ends on both sides of its edges)."""
    return int(N.helper("v100_resample_tile"))


def resample_out_len(length: int, orig_freq, new_freq) -> int:
    """ceil(new length / orig): the samples `resample` returns for `length` of them."""
    o, n = _rates(orig_freq, new_freq)
    return int(N.helper("v100_resample_out_len", int(length), o, n))


@torch.no_grad()
def resample(waveform: torch.Tensor, orig_freq, new_freq, lengths=None, lowpass_filter_width: int = 6, rolloff: float = 0.99):
    """`torchaudio.functional.resample` (default method) on the GPU, one launch.  waveform [N] or [B, Nmax] float32 -> [M] or
    [B, Mmax], M = ceil(new N / orig).  With `lengths` ([B], CPU or device) every row is an utterance of its own length: returns
    (y, out_lengths [B] int32 on the device); row b holds ceil(new lengths[b] / orig) samples and exact zeros from there on, and
    what the input holds beyond lengths[b] is never read.  Equal rates return the argument itself.  No CPU fallback."""
    o, n = _rates(orig_freq, new_freq)
    if o == n:
        if lengths is None:
            return waveform
        return waveform, torch.as_tensor(lengths).to(waveform.device, torch.int32)
    F_._check(waveform, "resample")
    if waveform.dim() not in (1, 2) or waveform.shape[-1] < 1 or waveform.shape[0] < 1:
        raise ValueError("resample: waveform must be [samples] or [B, samples], not empty")
    k = resample_kernel(o, n, lowpass_filter_width, rolloff)
    x = waveform[None] if waveform.dim() == 1 else waveform
    x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    B, Nmax = x.shape
    Mmax = N.helper("v100_resample_out_len", Nmax, o, n)
    if Mmax >= 2 ** 31:
        raise ValueError(f"resample: {Nmax} samples at {o}:{n} give {Mmax} outputs, more than one launch indexes")
    lens = None
    if lengths is not None:
        lens = torch.as_tensor(lengths)
        if lens.shape != (B,):
            raise ValueError(f"resample: lengths must be [{B}], got {tuple(lens.shape)}")
        if not lens.is_cuda and lens.numel() and (int(lens.min()) < 0 or int(lens.max()) > Nmax):
            raise ValueError(f"resample: lengths must lie in [0, {Nmax}]")
        lens = lens.to(x.device, torch.int32).contiguous()
    taps, starts = _device_bank(k, int(lowpass_filter_width), float(rolloff), x.device)
    y = torch.empty((B, Mmax), dtype=torch.float32, device=x.device)
    out_lens = torch.empty((B,), dtype=torch.int32, device=x.device) if lens is not None else None
    with torch.cuda.device(x.device):
        N.call("v100_resample_sinc", x, lens, taps, starts, y, out_lens, B, Nmax, Mmax, k.o, k.n, k.width, k.L)
    if lens is not None:
        return y, out_lens
    return y[0] if waveform.dim() == 1 else y


def load_batch(paths, sample_rate, device=None):
    """A list of WAV files -> (wave [B, Mmax] float32, zero beyond each utterance, wave_len [B] int32), both on the device, in
    the order of `paths`: per file what the reference's transforms do (load, first channel, resample to `sample_rate`:
    data_modules.py:287-292), row b equal to resample(load_wav(paths[b])[0][0], its rate, sample_rate).  The files are grouped by
    their own rate; a group is one padded block, one host-to-device copy and one resample(..., lengths=) launch, and its rows
    are scattered to their places by one indexed copy.  Files already at `sample_rate` are copied through."""
    if not torch.cuda.is_available():
        raise RuntimeError("load_batch: voice100_amd runs on the GPU only (no CPU fallback): the resampling runs on the device")
    paths = list(paths)
    if not paths:
        raise ValueError("load_batch: no paths")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"load_batch: voice100_amd runs on the GPU only (got device {device})")
    _rates(sample_rate, sample_rate)                                  # a positive integer, or ValueError
    target = int(sample_rate)
    groups = {}                                                       # source rate -> [(row, first channel)]
    for row, path in enumerate(paths):
        waveform, sr = load_wav(path)
        if waveform.shape[1] < 1:
            raise ValueError(f"{path}: no samples")
        groups.setdefault(sr, []).append((row, waveform[0]))
    done = []                                                         # (rows, y [G, M], y_len [G])
    for sr, items in groups.items():
        rows = torch.tensor([r for r, _ in items], dtype=torch.int64)
        lens = torch.tensor([w.shape[0] for _, w in items], dtype=torch.int32)
        block = torch.zeros((len(items), int(lens.max())), dtype=torch.float32)
        for g, (_, w) in enumerate(items):
            block[g, :w.shape[0]] = w
        y, y_len = resample(block.to(device), sr, target, lengths=lens)
        done.append((rows.to(device), y, y_len))
    B, width = len(paths), max(y.shape[1] for _, y, _ in done)
    wave = torch.zeros((B, width), dtype=torch.float32, device=device)
    wave_len = torch.empty((B,), dtype=torch.int32, device=device)
    for rows, y, y_len in done:
        wave[:, :y.shape[1]].index_copy_(0, rows, y)
        wave_len.index_copy_(0, rows, y_len)
    return wave, wave_len


class WORLDAudioProcessor(nn.Module):
    """voice100's WORLDAudioProcessor (data_modules.py:295-316): a file path -> (f0, logspc or mcep, codeap), float32 CPU tensors
    as `WORLDVocoder.encode` returns them.  The reference reads the file through sox (`remix 1`: the first channel; `rate`: to
    `sample_rate`); here `load_wav` reads it and `resample` converts the rate.  sox's `rate` effect is a different low-pass filter
    from torchaudio's windowed sinc, so the features are those of this library's resampler, not sample-equal to a sox run --
    unpinned, like the rest of the WORLD analysis."""

    def __init__(self, sample_rate: int, use_mcep: bool) -> None:
        from .vocoder import WORLDVocoder
        super().__init__()
        self.sample_rate = sample_rate
        self.vocoder = WORLDVocoder(sample_rate=sample_rate, use_mcep=use_mcep)

    @property
    def audio_size(self) -> int:
        return sum(self.vocoder.output_dims)

    def forward(self, audiopath):
        if not torch.cuda.is_available():
            raise RuntimeError("WORLDAudioProcessor runs on the GPU only (no CPU fallback)")
        waveform, sr = load_wav(audiopath)
        x = resample(waveform[0].to(torch.device("cuda", torch.cuda.current_device())), sr, self.sample_rate)
        return self.vocoder.encode(x)
