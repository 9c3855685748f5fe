"""From an audio file to a waveform at the model's rate, without torchaudio: a RIFF/WAVE reader on the host, a FLAC decoder on the
GPU (csrc/flac.hip: the container is parsed on the host, the frames are found, decoded, chained and committed on the device) and
`torchaudio.functional.resample`'s default method on the GPU (csrc/resample.hip).

The reference opens files with `torchaudio.load` + `torchaudio.functional.resample` (data_modules.py:287-292) or with sox effects
(`remix 1`, `rate`: data_modules.py:295-316).  `load_wav` returns what `torchaudio.load` returns for a WAV file with its defaults;
`resample` follows the published definition of `sinc_interpolation` with a Hann window, its filter bank built in float64 and
rounded to float32 once (torchaudio builds it in float32: a few ulps per tap apart).  PARITY UNPINNED against torchaudio itself
(absent here): checked against a float64 restatement of that definition.  `load_flac` returns what `torchaudio.load` returns for a
native FLAC file (LibriSpeech's format; 8 to 24 bits, 1 to 8 channels), `load_audio` picks between the two by the file's first bytes,
and `load_batch` takes either.  FLAC parity with libFLAC rests on the three worked examples of the format's RFC until real files
exist under tests/golden/flac.  Out of scope: Ogg-FLAC, files with a leading ID3 tag, FLAC of unknown length, 32-bit FLAC and every
lossy format.

Writing: `save_wav` (PCM 8 / 16 / 24 bits, on the host, no GPU needed), `encode_flac` / `save_flac` (csrc/flac_enc.hip: the frames are
searched, costed exactly and packed on the device, the host adds b'fLaC' and STREAMINFO), `save_audio` by extension and `save_batch` for
a batch on the device.  Floats become integers as clamp(rint(x 2^(bits-1))), ties to even, in every writer.  Out of scope when writing:
Ogg-FLAC, variable blocking, escape-coded partitions, more than two channels, 32-bit samples, metadata blocks other than STREAMINFO,
dither and every lossy format.
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


# ---- FLAC: the container on the host, the frames on the device (csrc/flac.hip) ---------------------------------------------------
FlacInfo = namedtuple("FlacInfo", "sample_rate channels bits_per_sample total_samples min_blocksize max_blocksize md5 first_frame_offset")
FlacInfo.__doc__ = """STREAMINFO of a FLAC file, and the byte at which its first frame begins.  md5: 16 bytes, all zero = unknown."""

_FLAC_STATUS = {
    1: "more frame headers than its STREAMINFO allows for (near byte {w} of the frames)",
    2: "no valid frame header where frame {w} must begin (missing, cut off, or damaged)",
    3: "frame {w} holds a reserved code",
    4: "frame {w} runs past the end of the file (truncated?)",
    5: "frame {w} fails its CRC-16 (damaged data)",
    6: "frame {w} is not at the sample position that follows the frame before it (a frame is missing)",
    7: "frame {w} passes the total_samples of STREAMINFO",
    8: "the file ends after {w} frames, short of the total_samples of STREAMINFO",
}


def _flac_bytes(src):
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src), "<bytes>"
    with open(src, "rb") as f:
        return f.read(), str(src)


def _flac_info(data: bytes, what: str) -> FlacInfo:
    if data[:4] == b"OggS":
        raise ValueError(f"{what}: an Ogg container (Ogg-FLAC is not read; native FLAC begins b'fLaC')")
    if data[:3] == b"ID3":
        raise ValueError(f"{what}: a leading ID3 tag (strip it; native FLAC begins b'fLaC')")
    if data[:4] != b"fLaC":
        raise ValueError(f"{what}: not a FLAC file (it begins {data[:4]!r})")
    pos, info = 4, None
    while True:
        if pos + 4 > len(data):
            raise ValueError(f"{what}: truncated FLAC metadata (a block header at byte {pos}, the file has {len(data)})")
        last, typ, size = data[pos] >> 7, data[pos] & 0x7F, int.from_bytes(data[pos + 1:pos + 4], "big")
        if pos + 4 + size > len(data):
            raise ValueError(f"{what}: truncated FLAC metadata (block type {typ} at byte {pos} declares {size} bytes, "
                             f"{len(data) - pos - 4} in the file)")
        if pos == 4 and (typ != 0 or size != 34):
            raise ValueError(f"{what}: the first metadata block is type {typ} with {size} bytes, not STREAMINFO (type 0, 34 bytes)")
        if typ == 0 and info is None:
            b = data[pos + 4:pos + 38]
            x = int.from_bytes(b[10:18], "big")
            info = (x >> 44, ((x >> 41) & 7) + 1, ((x >> 36) & 31) + 1, x & ((1 << 36) - 1),
                    int.from_bytes(b[0:2], "big"), int.from_bytes(b[2:4], "big"), bytes(b[18:34]))
        pos += 4 + size
        if last:
            break
    rate, channels, bits, total, lo, hi, md5 = info
    if total == 0:
        raise ValueError(f"{what}: STREAMINFO gives total_samples 0 (length unknown): not decoded")
    if bits == 32:
        raise ValueError(f"{what}: 32 bits per sample (a side channel would need 33): not decoded")
    if bits < 4 or channels > 8:
        raise ValueError(f"{what}: {channels} channels of {bits} bits per sample: not decoded")
    if total >= 2 ** 31:
        raise ValueError(f"{what}: {total} samples: sample positions pass 2^31, not decoded")
    if lo < 1 or hi < lo:
        raise ValueError(f"{what}: STREAMINFO gives block sizes {lo} to {hi}")
    if rate < 1:
        raise ValueError(f"{what}: STREAMINFO gives a sample rate of {rate} Hz")
    return FlacInfo(rate, channels, bits, total, lo, hi, md5, pos)


def flac_info(path_or_bytes) -> FlacInfo:
    """The STREAMINFO block of a native FLAC file (a path, or its bytes) and where its frames begin; needs no GPU.  ValueError naming
    what was found for: a file that is not FLAC, Ogg-FLAC, a leading ID3 tag, a truncated metadata chain, total_samples 0 (length
    unknown), 32 bits per sample, and a file so long that sample positions pass 2^31."""
    return _flac_info(*_flac_bytes(path_or_bytes))


_FLAC_WS_LIMIT = 2 ** 31 - 1                                           # staging ints one call indexes


def _flac_plan(datas, infos, names):
    """The byte buffer and the per-file table v100_flac_decode takes (numpy, host only): (buffer uint8, table [B][16] int32, S, H,
    stage_ints, max_file_bytes)."""
    B = len(datas)
    table = np.zeros((B, 16), np.int32)
    chunks, at, slot, entry, stage, longest = [], 0, 0, 0, 0, 1
    for b, (data, fi) in enumerate(zip(datas, infos)):
        region = data[fi.first_frame_offset:]
        frames = -(-fi.total_samples // fi.min_blocksize)
        slots = frames + 8 + frames // 8                              # every true frame, and slack for payload bytes that spell a header
        entries = 1 << max(4, (2 * slots - 1).bit_length())
        table[b, :13] = (at, at + len(region), fi.channels, fi.bits_per_sample, fi.min_blocksize, fi.max_blocksize, fi.total_samples, b,
                         slot, slots, entry, entries, stage)
        padded = -(-len(region) // 16) * 16 + 16
        chunks.append(np.frombuffer(region, np.uint8))
        chunks.append(np.zeros(padded - len(region), np.uint8))
        at, slot, entry, longest = at + padded, slot + slots, entry + entries, max(longest, len(region))
        stage += slots * fi.channels * fi.max_blocksize
        if stage > _FLAC_WS_LIMIT or at > _FLAC_WS_LIMIT or slot >= 2 ** 26 or entry >= 2 ** 27:
            raise ValueError(f"decode_flac: the batch needs more workspace than one call indexes (at {names[b]}: {fi.total_samples} samples "
                             f"in blocks of {fi.min_blocksize} to {fi.max_blocksize}); decode fewer files per call")
    return np.concatenate(chunks), table, slot, entry, stage, longest


@torch.no_grad()
def _flac_decode_device(files, device, channels, want_pcm):
    """decode_flac up to and including the read-back of the status: (wave, lengths, pcm or None, status [B][2] numpy, names, infos)."""
    if channels not in ("first", "all"):
        raise ValueError(f"decode_flac: channels must be 'first' or 'all' (got {channels!r})")
    files = list(files)
    if not files:
        raise ValueError("decode_flac: no files")
    datas, names, infos = [], [], []
    for k, src in enumerate(files):
        data, name = _flac_bytes(src)
        name = f"<bytes #{k}>" if name == "<bytes>" else name
        datas.append(data)
        names.append(name)
        infos.append(_flac_info(data, name))
    if not torch.cuda.is_available():
        raise RuntimeError("decode_flac: voice100_amd runs on the GPU only (no CPU fallback): FLAC frames are decoded on the device")
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"decode_flac: voice100_amd runs on the GPU only (got device {device})")
    buf, table, S, H, stage_ints, longest = _flac_plan(datas, infos, names)
    B = len(files)
    Nmax = max(fi.total_samples for fi in infos)
    Cmax = max(fi.channels for fi in infos)
    Cw = 1 if channels == "first" else Cmax
    with torch.cuda.device(device):
        ws_bytes = int(N.helper("v100_flac_workspace_bytes", B, S, H, stage_ints))
        if ws_bytes < 0:
            raise ValueError(f"decode_flac: unsupported batch ({B} files, {S} frame slots)")
        d_buf = torch.from_numpy(buf).to(device)
        d_table = torch.from_numpy(table).to(device)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
        wave = torch.zeros((B, Nmax) if channels == "first" else (B, Cw, Nmax), dtype=torch.float32, device=device)
        pcm = torch.zeros((B, Cmax, Nmax), dtype=torch.int32, device=device) if want_pcm else None
        lengths = torch.empty((B,), dtype=torch.int32, device=device)
        status = torch.empty((B, 2), dtype=torch.int32, device=device)
        N.call("v100_flac_decode", d_buf, int(buf.size), d_table, ws, wave, pcm, lengths, status, B, S, H, stage_ints, longest, Cw, Cmax,
               Nmax)
        st = status.cpu().numpy()
    return wave, lengths, pcm, st, names, infos


@torch.no_grad()
def decode_flac(files, device=None, channels="first", verify_md5=False, return_pcm=False):
    """A list of FLAC files (paths, or their bytes) -> (wave, lengths, rates), decoded on the GPU in one pass (csrc/flac.hip).

    wave [B, Nmax] float32 on the device = channel 0 of each file (`channels="first"`), or [B, Cmax, Nmax] with every channel
    (`channels="all"`; rows of files with fewer channels stay zero); the sample value is int / 2^(bits - 1), as `torchaudio.load`
    normalises; exact zeros beyond each file's length.  lengths [B] int32 on the device, rates a list of ints.  With `return_pcm`
    a fourth value: the integer samples [B, Cmax, Nmax] int32 on the device.

    The container is parsed on the host (`flac_info`), the frame regions go to the device in one copy, four launches find, decode,
    chain and commit the frames, and ONE read-back brings the per-file status: a file that does not decode cleanly -- a damaged,
    truncated or missing frame, a sample count that disagrees with STREAMINFO -- is a ValueError naming the file, the frame and the
    reason.  `verify_md5` also reads the integer PCM back and compares the MD5 of the interleaved little-endian samples (whole
    bytes per sample) with STREAMINFO's; an all-zero MD5 is skipped.  Files of different rates, widths, channel counts and lengths
    mix freely.  No CPU fallback."""
    wave, lengths, pcm, st, names, infos = _flac_decode_device(files, device, channels, bool(return_pcm or verify_md5))
    B = len(names)
    for b in range(B):
        code, where = int(st[b, 0]), int(st[b, 1])
        if code:
            raise ValueError(f"{names[b]}: FLAC " + _FLAC_STATUS.get(code, f"status {code} at {{w}}").format(w=where))
    if verify_md5:
        import hashlib
        host = pcm.cpu().numpy()
        for b, fi in enumerate(infos):
            if fi.md5 == bytes(16):
                continue
            nb = (fi.bits_per_sample + 7) // 8
            inter = np.ascontiguousarray(host[b, :fi.channels, :fi.total_samples].T).reshape(-1)
            raw = inter.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nb]
            got = hashlib.md5(np.ascontiguousarray(raw).tobytes()).digest()
            if got != fi.md5:
                raise ValueError(f"{names[b]}: FLAC MD5 mismatch (decoded {got.hex()}, STREAMINFO says {fi.md5.hex()})")
    rates = [fi.sample_rate for fi in infos]
    return (wave, lengths, rates, pcm) if return_pcm else (wave, lengths, rates)


def load_flac(path, verify_md5=False):
    """(waveform [channels, frames] float32 CPU tensor, sample_rate): `torchaudio.load(path)` with its defaults, for a FLAC file.
    The frames are decoded on the GPU (`decode_flac`): without one this is a RuntimeError; `flac_info` works without."""
    if not torch.cuda.is_available():
        raise RuntimeError("load_flac: voice100_amd runs on the GPU only (no CPU fallback): FLAC frames are decoded on the device")
    wave, _, rates = decode_flac([path], channels="all", verify_md5=verify_md5)
    return wave[0].cpu(), int(rates[0])


def load_audio(path):
    """`load_wav` or `load_flac`, by the file's first four bytes (b'RIFF' / b'fLaC'); anything else is a ValueError naming them."""
    with open(path, "rb") as f:
        magic = f.read(4)
    if magic == b"RIFF":
        return load_wav(path)
    if magic == b"fLaC":
        return load_flac(path)
    raise ValueError(f"{path}: neither WAV nor FLAC (it begins {magic!r}; b'RIFF' and b'fLaC' are read)")


# ---- writing: WAV on the host, FLAC frames on the device (csrc/flac_enc.hip) -----------------------------------------------------
_FLAC_ENC_STATUS = {
    1: "a non-finite sample (NaN or infinity) at sample {w}",
    2: "an integer sample outside the {bits}-bit range at sample {w}",
    3: "an internal inconsistency between the encoder's plan and its bit stream (a bug: please report the input)",
    4: "a segment outside the input (near sample {w})",
}
_FLAC_RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
_FLAC_ENC_MAX_FRAMES = 1 << 24
_FLAC_ENC_MAX_BYTES = 1 << 36


def _check_format(who, sample_rate, bits_per_sample, channels):
    if bits_per_sample not in (8, 16, 24):
        raise ValueError(f"{who}: bits_per_sample must be 8, 16 or 24 (got {bits_per_sample!r})")
    if channels not in (1, 2):
        raise ValueError(f"{who}: 1 or 2 channels are written (got {channels})")
    if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or not 1 <= int(sample_rate) <= 655350:
        raise ValueError(f"{who}: sample_rate must be an integer in 1 .. 655350 (got {sample_rate!r})")


def _flac_rate_code(rate):
    """(frame-header code, 16-bit trailer): a table entry, else Hz, else tens of Hz, else 0 = "as STREAMINFO says"."""
    if rate in _FLAC_RATE_CODES:
        return _FLAC_RATE_CODES[rate], 0
    if rate < 65536:
        return 13, rate
    if rate % 10 == 0 and rate // 10 < 65536:
        return 14, rate // 10
    return 0, 0


def _flac_enc_plan(lengths, rows, starts, R, Nrow, C, bits_per_sample, block_size):
    """The frame table v100_flac_encode takes (numpy, host only): (ftab [F][8] int32, first frame of every item [B + 1], out_bytes).
    ValueError naming the item for a length of 0, of 2^31 or more, or past the end of its row, and for a batch beyond one call."""
    B = len(lengths)
    frames_total, bytes_total = 0, 0
    for b in range(B):
        n, r, s = int(lengths[b]), int(rows[b]), int(starts[b])
        if n == 0:
            raise ValueError(f"encode_flac: item {b} has length 0 (a FLAC total of 0 means 'unknown', which flac_info refuses)")
        if n < 0 or n >= 2 ** 31:
            raise ValueError(f"encode_flac: item {b} has {n} samples; 1 .. 2^31 - 1 are encoded")
        if not 0 <= r < R or s < 0 or s + n > Nrow:
            raise ValueError(f"encode_flac: item {b} (row {r}, samples {s} .. {s + n}) lies outside the input [{R}, {Nrow}]")
        f = -(-n // block_size)
        frames_total += f
        bytes_total += 18 * f + (16 * f + (C * bits_per_sample + (C == 2)) * n + 7 * f) // 8
        if frames_total > _FLAC_ENC_MAX_FRAMES or bytes_total > _FLAC_ENC_MAX_BYTES:
            raise ValueError(f"encode_flac: the batch needs more frames or bytes than one call indexes (at item {b}: {frames_total} frames, "
                             f"{bytes_total} bytes); encode fewer items per call")
    lens = np.asarray(lengths, np.int64)
    nf = -(-lens // block_size)
    first = np.concatenate([[0], np.cumsum(nf)])
    item = np.repeat(np.arange(B, dtype=np.int64), nf)
    num = np.arange(int(first[-1]), dtype=np.int64) - first[item]
    ftab = np.zeros((int(first[-1]), 8), np.int32)
    ftab[:, 0] = np.asarray(rows, np.int64)[item]
    ftab[:, 1] = np.asarray(starts, np.int64)[item] + num * block_size
    ftab[:, 2] = np.minimum(block_size, lens[item] - num * block_size)
    ftab[:, 3] = num
    ftab[:, 4] = item
    return ftab, first, -(-bytes_total // 16) * 16


def _flac_streaminfo(rate, channels, bits, total, block_size, min_frame, max_frame, md5):
    x = (rate << 44) | ((channels - 1) << 41) | ((bits - 1) << 36) | total
    body = (block_size.to_bytes(2, "big") * 2 + min_frame.to_bytes(3, "big") + max_frame.to_bytes(3, "big") + x.to_bytes(8, "big") + md5)
    return b"fLaC" + bytes([0x80]) + len(body).to_bytes(3, "big") + body


def _quantise(x: torch.Tensor, bits: int) -> torch.Tensor:
    """clamp(rint(x 2^(bits-1))), ties to even (the product is exact in float32), as int32; integer input passes through."""
    if not x.dtype.is_floating_point:
        return x.to(torch.int32)
    return torch.clamp(torch.round(x.float() * float(1 << (bits - 1))), -float(1 << (bits - 1)), float((1 << (bits - 1)) - 1)).to(torch.int32)


@torch.no_grad()
def encode_flac(wave_or_pcm, lengths=None, sample_rate=16000, bits_per_sample=16, block_size=4096, max_lpc_order=8, max_partition_order=6,
                md5=False, rows=None, starts=None):
    """A batch of waveforms on the device -> a list of FLAC files as bytes, encoded on the GPU in one pass (csrc/flac_enc.hip).

    wave_or_pcm: float32 [B, N] or [B, C, N] (C 1 or 2), quantised as clamp(rint(x 2^(bits-1))) with ties to even -- a wave that came
    from a file of this width returns to its integers -- or int32 PCM of the same shapes.  Item b is samples
    starts[b] .. starts[b] + lengths[b] of row rows[b] (defaults: row b, start 0, the whole row), so segments of one long recording
    are encoded without a copy.  Fixed blocking (`block_size` 16 .. 4608, the last frame shorter); per frame and channel the cheapest,
    by exact bit count, of constant, verbatim, fixed orders 0-4 and LPC orders 1 .. `max_lpc_order` (0 .. 12; 0 = none), each over Rice
    parameters 0-14 and partition orders 0 .. `max_partition_order` (0 .. 6); stereo frames take the cheapest of independent, left/side,
    side/right and mid/side.  The host writes b'fLaC' and STREAMINFO (block sizes = block_size, smallest and largest frame, rate,
    channels, width, total samples, MD5) ahead of the device's frames.

    Read-backs: TWO -- the frame sizes with the per-item status, then the bytes themselves -- plus one for `lengths` when that is a
    device tensor.  `md5=True` adds a third: the integer PCM of every item is quantised on the device, copied to the host (4 bytes
    per sample) and hashed there, which costs about as much as the rest of the call; `md5=False` writes the all-zero "unknown" signature.

    ValueError naming the item for: a length of 0, 2^31 samples or more, a segment outside its row, a non-finite sample (with its
    index), an integer sample outside the width, more than one call indexes; ValueError for an unsupported width, channel count,
    rate or search setting.  RuntimeError without a GPU: there is no CPU fallback."""
    x = wave_or_pcm
    if not isinstance(x, torch.Tensor) or x.dim() not in (2, 3) or x.dtype not in (torch.float32, torch.int32):
        raise ValueError("encode_flac: a float32 or int32 tensor [B, N] or [B, C, N] is encoded")
    C = 1 if x.dim() == 2 else x.shape[1]
    _check_format("encode_flac", sample_rate, bits_per_sample, C)
    if not 16 <= int(block_size) <= 4608 or not 0 <= int(max_lpc_order) <= 12 or not 0 <= int(max_partition_order) <= 6:
        raise ValueError(f"encode_flac: block_size 16 .. 4608, max_lpc_order 0 .. 12 and max_partition_order 0 .. 6 are supported "
                         f"(got {block_size}, {max_lpc_order}, {max_partition_order})")
    R, Nmax = x.shape[0], x.shape[-1]
    if R < 1 or Nmax >= 2 ** 31:
        raise ValueError(f"encode_flac: input of shape {tuple(x.shape)}: at least one row and fewer than 2^31 samples per row are encoded")

    def host_list(v):
        if v is None:
            return None
        v = v.cpu().tolist() if isinstance(v, torch.Tensor) else [int(e) for e in v]
        return [int(e) for e in v]
    rows_l, starts_l, lens_l = host_list(rows), host_list(starts), host_list(lengths)
    B = len(rows_l) if rows_l is not None else len(starts_l) if starts_l is not None else len(lens_l) if lens_l is not None else R
    if rows_l is None:
        if B != R:
            raise ValueError(f"encode_flac: {B} items for {R} rows; pass `rows` to encode segments")
        rows_l = list(range(R))
    starts_l = [0] * B if starts_l is None else starts_l
    lens_l = [Nmax - s for s in starts_l] if lens_l is None else lens_l
    if not (len(rows_l) == len(starts_l) == len(lens_l) == B) or B < 1:
        raise ValueError(f"encode_flac: rows, starts and lengths must have one entry per item ({len(rows_l)}, {len(starts_l)}, {len(lens_l)})")
    ftab, first, out_bytes = _flac_enc_plan(lens_l, rows_l, starts_l, R, Nmax, C, int(bits_per_sample), int(block_size))
    if not torch.cuda.is_available() or not x.is_cuda:
        raise RuntimeError("encode_flac: voice100_amd runs on the GPU only (no CPU fallback): FLAC frames are encoded on the device"
                           + ("" if not torch.cuda.is_available() else f" (got a tensor on {x.device})"))
    F = ftab.shape[0]
    rate = int(sample_rate)
    code, extra = _flac_rate_code(rate)
    x = x.contiguous()
    if x.data_ptr() % 16:
        x = x.clone()
    with torch.cuda.device(x.device):
        ws_bytes = int(N.helper("v100_flac_encode_workspace_bytes", F, C))
        if ws_bytes < 0:
            raise ValueError(f"encode_flac: unsupported batch ({F} frames of {C} channels)")
        d_ftab = torch.from_numpy(ftab).to(x.device)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x.device)
        out = torch.empty((out_bytes,), dtype=torch.uint8, device=x.device)
        Fp = -(-F // 4) * 4
        rep = torch.empty((Fp + 2 * B,), dtype=torch.int32, device=x.device)
        is_float = x.dtype == torch.float32
        N.call("v100_flac_encode", x if is_float else None, None if is_float else x, d_ftab, ws, out, rep[:Fp], rep[Fp:], B, F, R, C, Nmax,
               int(bits_per_sample), int(block_size), int(max_lpc_order), int(max_partition_order), code, extra, out_bytes)
        host = rep.cpu().numpy()                                       # read-back 1: frame sizes and status
        sizes, st = host[:F].astype(np.int64), host[Fp:].reshape(B, 2)
        for b in range(B):
            if st[b, 0]:
                where = 0x7FFFFFFF - int(st[b, 1])
                raise ValueError(f"encode_flac: item {b}: " + _FLAC_ENC_STATUS.get(int(st[b, 0]), "status {c}").format(
                    w=where, bits=bits_per_sample, c=int(st[b, 0])))
        offs = np.concatenate([[0], np.cumsum(sizes)])
        data = out[:int(offs[-1])].cpu().numpy().tobytes()             # read-back 2: the frames
        sums = [bytes(16)] * B
        if md5:
            import hashlib
            seg = torch.cat([x.reshape(R, C, Nmax)[r, :, s:s + n] for r, s, n in zip(rows_l, starts_l, lens_l)], dim=1)
            pcm = _quantise(seg, int(bits_per_sample)).cpu().numpy()   # read-back 3: [C, all samples] int32
            nb, at = bits_per_sample // 8, 0
            for b, n in enumerate(lens_l):
                inter = np.ascontiguousarray(pcm[:, at:at + n].T).reshape(-1)
                sums[b] = hashlib.md5(np.ascontiguousarray(inter.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nb]).tobytes()).digest()
                at += n
    files = []
    for b in range(B):
        f0, f1 = int(first[b]), int(first[b + 1])
        fs = sizes[f0:f1]
        head = _flac_streaminfo(rate, C, int(bits_per_sample), lens_l[b], int(block_size), int(fs.min()), int(fs.max()), sums[b])
        files.append(head + data[int(offs[f0]):int(offs[f1])])
    return files


def _pcm_bytes(waveform, bits_per_sample, who):
    """[C, N] or [N] tensor (float: quantised like encode_flac; integer: taken as PCM) -> (interleaved little-endian bytes, C, N)."""
    x = waveform.detach().cpu() if isinstance(waveform, torch.Tensor) else torch.as_tensor(waveform)
    if x.dim() == 1:
        x = x[None]
    if x.dim() != 2:
        raise ValueError(f"{who}: waveform must be [channels, samples] or [samples] (got {tuple(x.shape)})")
    if x.dtype.is_floating_point and not bool(torch.isfinite(x).all()):
        bad = int((~torch.isfinite(x)).nonzero()[0, 1])
        raise ValueError(f"{who}: a non-finite sample (NaN or infinity) at sample {bad}")
    q = _quantise(x, bits_per_sample).numpy().T                        # [N, C]
    if bits_per_sample == 8:
        raw = (q + 128).astype(np.uint8).tobytes()
    elif bits_per_sample == 16:
        raw = q.astype("<i2").tobytes()
    else:
        raw = np.ascontiguousarray(np.ascontiguousarray(q.astype("<i4")).view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()
    return raw, x.shape[0], x.shape[1]


def save_wav(path, waveform, sample_rate, bits_per_sample=16):
    """Write a PCM WAV file of 8 (unsigned), 16 or 24 bits: waveform [channels, samples] or [samples], on any device, float (quantised
    as clamp(rint(x 2^(bits-1))), ties to even, the rule of encode_flac) or integer PCM.  Needs no GPU; `load_wav` returns the same
    integers over 2^(bits-1).  ValueError for another width, a non-finite sample or an empty waveform."""
    if bits_per_sample not in (8, 16, 24):
        raise ValueError(f"save_wav: bits_per_sample must be 8, 16 or 24 (got {bits_per_sample!r})")
    if isinstance(sample_rate, bool) or int(sample_rate) != sample_rate or not 1 <= int(sample_rate) < 2 ** 32:
        raise ValueError(f"save_wav: sample_rate must be a positive integer (got {sample_rate!r})")
    raw, C, n = _pcm_bytes(waveform, bits_per_sample, "save_wav")
    if n < 1 or not 1 <= C < 65536 or len(raw) >= 2 ** 32 - 36:
        raise ValueError(f"save_wav: {C} channels of {n} samples cannot be written as one WAV file")
    width = bits_per_sample // 8
    fmt = struct.pack("<HHIIHH", _PCM, C, int(sample_rate), int(sample_rate) * C * width, C * width, bits_per_sample)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw) + (len(raw) & 1)) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt)
        f.write(b"data" + struct.pack("<I", len(raw)) + raw + (b"\0" if len(raw) & 1 else b""))


def save_flac(path, waveform, sample_rate, bits_per_sample=16, **enc):
    """Write a FLAC file: waveform [channels, samples] or [samples] (float32 or int32; moved to the GPU if it is not there), encoded by
    `encode_flac` (`enc`: block_size, max_lpc_order, max_partition_order, md5).  RuntimeError without a GPU."""
    x = waveform[None] if waveform.dim() == 1 else waveform
    if x.dim() != 2:
        raise ValueError(f"save_flac: waveform must be [channels, samples] or [samples] (got {tuple(waveform.shape)})")
    if not torch.cuda.is_available():
        raise RuntimeError("save_flac: voice100_amd runs on the GPU only (no CPU fallback): FLAC frames are encoded on the device")
    if not x.is_cuda:
        x = x.to(torch.device("cuda", torch.cuda.current_device()))
    data = encode_flac(x[None], None, sample_rate, bits_per_sample, **enc)[0]
    with open(path, "wb") as f:
        f.write(data)


def _audio_kind(path, who):
    ext = str(path).lower().rsplit(".", 1)[-1] if "." in str(path) else ""
    if ext not in ("wav", "flac"):
        raise ValueError(f"{who}: {path}: the file name must end in .wav or .flac")
    return ext


def save_audio(path, waveform, sample_rate, bits_per_sample=16, **enc):
    """`save_wav` or `save_flac`, by the file name's extension (.wav / .flac); anything else is a ValueError naming the two."""
    if _audio_kind(path, "save_audio") == "wav":
        if enc:
            raise ValueError(f"save_audio: {sorted(enc)} apply to .flac files only")
        return save_wav(path, waveform, sample_rate, bits_per_sample)
    return save_flac(path, waveform, sample_rate, bits_per_sample, **enc)


def save_batch(paths, wave, lengths=None, sample_rate=16000, bits_per_sample=16, **enc):
    """Write row b of wave [B, N] (or [B, C, N]) on the device, up to lengths[b], to paths[b] (.wav or .flac, mixed freely): ONE
    `encode_flac` call for all .flac paths, ONE device-to-host copy for all .wav paths.  Nothing is written when a name has another
    extension (ValueError) or an item is refused."""
    paths = list(paths)
    kinds = [_audio_kind(p, "save_batch") for p in paths]
    if wave.dim() not in (2, 3) or wave.shape[0] != len(paths):
        raise ValueError(f"save_batch: {len(paths)} paths for a wave of shape {tuple(wave.shape)}")
    lens = [wave.shape[-1]] * len(paths) if lengths is None else [int(v) for v in (lengths.cpu().tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(lens) != len(paths):
        raise ValueError(f"save_batch: {len(paths)} paths and {len(lens)} lengths")
    for b, n in enumerate(lens):
        if not 1 <= n <= wave.shape[-1]:
            raise ValueError(f"save_batch: item {b} has length {n}; 1 .. {wave.shape[-1]} samples are written")
    fl = [b for b, k in enumerate(kinds) if k == "flac"]
    wv = [b for b, k in enumerate(kinds) if k == "wav"]
    files = encode_flac(wave, [lens[b] for b in fl], sample_rate, bits_per_sample, rows=fl, **enc) if fl else []
    host = wave[torch.tensor(wv, device=wave.device)][..., :max(lens[b] for b in wv)].cpu() if wv else None
    for k, b in enumerate(wv):
        _pcm_bytes(host[k][..., :lens[b]], bits_per_sample, f"save_batch: item {b}")      # refuses before anything is written
    for b, data in zip(fl, files):
        with open(paths[b], "wb") as f:
            f.write(data)
    for k, b in enumerate(wv):
        save_wav(paths[b], host[k][..., :lens[b]], sample_rate, bits_per_sample)


# ---- the filter bank --------------------------------------------------------------------------------------------------------
ResampleKernel =namedtuple("ResampleKernel", "o n width L dense starts taps")
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
    """A list of WAV and / or FLAC files -> (wave [B, Mmax] float32, zero beyond each utterance, wave_len [B] int32), both on the device, in
    the order of `paths`: per file what the reference's transforms do (load, first channel, resample to `sample_rate`:
    data_modules.py:287-292), row b equal to resample(load_wav(paths[b])[0][0], its rate, sample_rate).  The files are grouped by
    their own rate; a group is one padded block, one host-to-device copy and one resample(..., lengths=) launch, and its rows
    are scattered to their places by one indexed copy.  Files already at `sample_rate` are copied through.  The FLAC files among
    `paths` are decoded together in ONE device pass (decode_flac), whatever their rates, and their rows join the group of their rate
    on the device; WAV rows and all-WAV batches go exactly the way they went before FLAC was read."""
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
    groups = {}                                                       # source rate -> [(row, first channel)]: WAV rows, on the host
    flac_rows, flac_data = [], []
    for row, path in enumerate(paths):
        with open(path, "rb") as f:
            is_flac = f.read(4) == b"fLaC"
            if is_flac:
                flac_rows.append(row)
                flac_data.append(b"fLaC" + f.read())
        if is_flac:
            continue
        waveform, sr = load_wav(path)
        if waveform.shape[1] < 1:
            raise ValueError(f"{path}: no samples")
        groups.setdefault(sr, []).append((row, waveform[0]))
    flac_groups = {}                                                  # source rate -> [(row, index into the decoded block, length)]
    if flac_rows:
        try:
            f_wave, _, f_rates = decode_flac(flac_data, device)       # every FLAC file of the batch in one device pass
        except ValueError as e:                                       # name the path, not the position among the FLAC files
            msg = str(e)
            for k, row in enumerate(flac_rows):
                msg = msg.replace(f"<bytes #{k}>", str(paths[row]))
            raise ValueError(msg) from None
        f_lens = [flac_info(d).total_samples for d in flac_data]
        for k, row in enumerate(flac_rows):
            flac_groups.setdefault(f_rates[k], []).append((row, k, f_lens[k]))
            groups.setdefault(f_rates[k], [])
    done = []                                                         # (rows, y [G, M], y_len [G])
    for sr, items in groups.items():
        fitems = flac_groups.get(sr, [])
        rows = torch.tensor([r for r, _ in items] + [r for r, _, _ in fitems], dtype=torch.int64)
        lens = torch.tensor([w.shape[0] for _, w in items] + [n for _, _, n in fitems], dtype=torch.int32)
        width = int(lens.max())
        block = torch.zeros((len(items), width), dtype=torch.float32)
        for g, (_, w) in enumerate(items):
            block[g, :w.shape[0]] = w
        block = block.to(device)
        if fitems:                                                    # the decoded rows are on the device already
            take = min(width, f_wave.shape[1])
            fblock = torch.zeros((len(fitems), width), dtype=torch.float32, device=device)
            fblock[:, :take] = f_wave[torch.tensor([k for _, k, _ in fitems], device=device), :take]
            block = torch.cat([block, fblock]) if items else fblock
        y, y_len = resample(block, sr, target, lengths=lens)
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
    `sample_rate`); here `load_audio` reads it (WAV or FLAC) and `resample` converts the rate.  sox's `rate` effect is a different low-pass filter
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
        waveform, sr = load_audio(audiopath)
        x = resample(waveform[0].to(torch.device("cuda", torch.cuda.current_device())), sr, self.sample_rate)
        return self.vocoder.encode(x)
