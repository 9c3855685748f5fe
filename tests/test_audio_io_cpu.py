"""voice100_amd.audio_io without a GPU: the WAV reader against files this test writes itself (stdlib `wave` and hand-packed
headers -- never the reader under test), the resampling filter bank against a float64 restatement of the published definition of
torchaudio.functional.resample's default method written out here (independent of audio_io.resample_kernel), the compact form the
kernel takes against the dense table, and the host-side pieces of the C ABI."""
import math
import os
import struct
import wave

import numpy as np
import pytest
import torch

from voice100_amd import audio_io as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (22050, 16000), (16000, 22050), (32000, 16000), (11025, 16000),
         (24000, 16000), (16000, 24000)]
WIDTHS = [17, 19, 7, 9, 7, 13, 7, 10, 7]
PCM_GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


# ---- files ------------------------------------------------------------------------------------------------------------------
def write_stdlib(path, ints, width, rate):
    """ints [frames, channels] -> a PCM file through stdlib `wave` (8-bit unsigned, 16 / 32-bit signed little-endian)."""
    dt = {1: "u1", 2: "<i2", 4: "<i4"}[width]
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ints.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(ints.astype(dt)).tobytes())


def chunk(cid, body, pad=True):
    return cid + struct.pack("<I", len(body)) + body + (b"\0" if (len(body) & 1 and pad) else b"")


def fmt_chunk(tag, channels, rate, bits, extensible=False):
    block = channels * bits // 8
    if not extensible:
        return chunk(b"fmt ", struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits))
    body = struct.pack("<HHIIHH", 0xFFFE, channels, rate, rate * block, block, bits)
    body += struct.pack("<HHI", 22, bits, (1 << channels) - 1) + struct.pack("<H", tag) + PCM_GUID_TAIL
    return chunk(b"fmt ", body)


def riff(*chunks):
    body = b"WAVE" + b"".join(chunks)
    return b"RIFF" + struct.pack("<I", len(body)) + body


def pack24(ints):
    v = ints.astype(np.int64).ravel() & 0xFFFFFF
    return np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=1).astype(np.uint8).tobytes()


def edge_ints(rng, frames, channels, lo, hi):
    """Random integers in [lo, hi] with the extremes and the midpoint planted where there is room."""
    v = rng.integers(lo, hi + 1, size=(frames, channels), dtype=np.int64)
    flat = v.reshape(-1)
    for i, e in enumerate((lo, hi, (lo + hi + 1) // 2, lo + 1)):
        if i < flat.size:
            flat[i] = e
    return v


def check(path, expect, rate):
    w, sr = A.load_wav(path)
    assert sr == rate and isinstance(sr, int)
    assert isinstance(w, torch.Tensor) and w.dtype == torch.float32 and not w.is_cuda and w.is_contiguous()
    assert tuple(w.shape) == expect.T.shape
    assert np.array_equal(w.numpy(), np.ascontiguousarray(expect.T))
    return w


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("frames", [1, 1000])
def test_pcm_files_written_by_the_standard_library(tmp_path, channels, frames):
    rng = np.random.default_rng(frames * 10 + channels)
    v = edge_ints(rng, frames, channels, 0, 255)
    write_stdlib(tmp_path / "u8.wav", v, 1, 8000)
    w = check(tmp_path / "u8.wav", ((v.astype(np.float64) - 128.0) / 128.0).astype(np.float32), 8000)
    assert float(w.reshape(-1)[0]) == -1.0                                           # 0 -> full-scale negative
    if frames * channels >= 3:
        assert float(w.T.reshape(-1)[2]) == 0.0                                      # 128 -> 0.0
    v = edge_ints(rng, frames, channels, -32768, 32767)
    write_stdlib(tmp_path / "s16.wav", v, 2, 44100)
    w = check(tmp_path / "s16.wav", (v.astype(np.float64) / 32768.0).astype(np.float32), 44100)
    assert float(w.reshape(-1)[0]) == -1.0
    v = edge_ints(rng, frames, channels, -2 ** 31, 2 ** 31 - 1)
    write_stdlib(tmp_path / "s32.wav", v, 4, 48000)
    w = check(tmp_path / "s32.wav", (v.astype(np.float64) / 2.0 ** 31).astype(np.float32), 48000)
    assert float(w.reshape(-1)[0]) == -1.0


@pytest.mark.parametrize("extensible", [False, True])
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("frames", [1, 1000])
def test_hand_packed_24_bit_and_float_files(tmp_path, channels, frames, extensible):
    rng = np.random.default_rng(frames * 100 + channels * 10 + extensible)
    v = edge_ints(rng, frames, channels, -2 ** 23, 2 ** 23 - 1)
    p = tmp_path / "s24.wav"
    p.write_bytes(riff(fmt_chunk(1, channels, 22050, 24, extensible), chunk(b"data", pack24(v))))
    w = check(p, (v.astype(np.float64) / 2.0 ** 23).astype(np.float32), 22050)
    assert float(w.reshape(-1)[0]) == -1.0
    f = rng.standard_normal((frames, channels))
    f.reshape(-1)[0] = 1.5                                                           # floats are not clipped
    p = tmp_path / "f32.wav"
    p.write_bytes(riff(fmt_chunk(3, channels, 16000, 32, extensible), chunk(b"fact", struct.pack("<I", frames)),
                       chunk(b"data", f.astype("<f4").tobytes())))
    check(p, f.astype(np.float32), 16000)
    p = tmp_path / "f64.wav"
    p.write_bytes(riff(fmt_chunk(3, channels, 11025, 64, extensible), chunk(b"data", f.astype("<f8").tobytes())))
    check(p, f.astype(np.float32), 11025)
    if extensible:                                                                   # 16-bit PCM inside EXTENSIBLE too
        v = edge_ints(rng, frames, channels, -32768, 32767)
        p = tmp_path / "x16.wav"
        p.write_bytes(riff(fmt_chunk(1, channels, 32000, 16, True), chunk(b"data", v.astype("<i2").tobytes())))
        check(p, (v.astype(np.float64) / 32768.0).astype(np.float32), 32000)


def test_unknown_and_odd_sized_chunks_are_skipped(tmp_path):
    rng = np.random.default_rng(5)
    v = edge_ints(rng, 333, 2, -32768, 32767)
    info = b"INFOISFT" + struct.pack("<I", 5) + b"abcde"                             # 17 bytes: odd
    assert len(info) & 1
    p = tmp_path / "list.wav"
    p.write_bytes(riff(chunk(b"JUNK", b"\x01\x02\x03"), fmt_chunk(1, 2, 16000, 16), chunk(b"LIST", info),
                       chunk(b"data", v.astype("<i2").tobytes()), chunk(b"LIST", info)))
    check(p, (v.astype(np.float64) / 32768.0).astype(np.float32), 16000)
    # an odd-sized data chunk (8-bit mono, 7 frames) followed by its pad byte and another chunk
    v8 = edge_ints(rng, 7, 1, 0, 255)
    p = tmp_path / "odd_data.wav"
    p.write_bytes(riff(fmt_chunk(1, 1, 8000, 8), chunk(b"data", v8.astype("u1").tobytes()), chunk(b"LIST", info)))
    check(p, ((v8.astype(np.float64) - 128.0) / 128.0).astype(np.float32), 8000)


def test_data_chunk_that_overruns_the_file(tmp_path):
    rng = np.random.default_rng(6)
    v = edge_ints(rng, 500, 2, -32768, 32767)
    body = v.astype("<i2").tobytes()
    for declared in (len(body) + 4096, 0xFFFFFFFF):
        p = tmp_path / f"overrun_{declared}.wav"
        p.write_bytes(b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + fmt_chunk(1, 2, 16000, 16)
                      + b"data" + struct.pack("<I", declared) + body)
        check(p, (v.astype(np.float64) / 32768.0).astype(np.float32), 16000)
    # ... and one cut in the middle of a frame: whole frames only
    p = tmp_path / "cut.wav"
    p.write_bytes(b"RIFF" + struct.pack("<I", 0xFFFFFFFF) + b"WAVE" + fmt_chunk(1, 2, 16000, 16)
                  + b"data" + struct.pack("<I", len(body)) + body[:4 * 123 + 3])
    check(p, (v[:123].astype(np.float64) / 32768.0).astype(np.float32), 16000)


def test_what_is_not_a_supported_wav_is_a_value_error_that_names_it(tmp_path):
    p = tmp_path / "mp3.wav"
    p.write_bytes(riff(fmt_chunk(0x0055, 2, 44100, 16), chunk(b"data", b"\0" * 64)))
    with pytest.raises(ValueError, match="0x0055"):
        A.load_wav(p)
    p = tmp_path / "x.flac"
    p.write_bytes(b"fLaC" + b"\0" * 64)
    with pytest.raises(ValueError, match="fLaC"):
        A.load_wav(p)
    whole = riff(fmt_chunk(1, 1, 16000, 16), chunk(b"data", b"\0" * 64))
    p = tmp_path / "trunc.wav"
    p.write_bytes(whole[:12 + 8 + 9])                                                # nine bytes into the body of `fmt `
    with pytest.raises(ValueError, match="fmt"):
        A.load_wav(p)
    p = tmp_path / "trunc_header.wav"
    p.write_bytes(whole[:12 + 5])                                                    # inside the chunk header of `fmt `
    with pytest.raises(ValueError):
        A.load_wav(p)
    p = tmp_path / "adpcm.wav"
    p.write_bytes(riff(fmt_chunk(1, 1, 16000, 12), chunk(b"data", b"\0" * 64)))      # PCM, but 12 bits
    with pytest.raises(ValueError, match="12"):
        A.load_wav(p)
    p = tmp_path / "empty.wav"
    p.write_bytes(b"")
    with pytest.raises(ValueError):
        A.load_wav(p)


def test_the_references_sample_round_trips_through_16_bit_pcm(tmp_path):
    en1 = np.load(os.path.join(ROOT, "tests", "golden", "world_ref_samples.npz"))["en1"]
    assert en1.dtype == np.int16
    write_stdlib(tmp_path / "en1.wav", en1[:, None], 2, 16000)
    w, sr = A.load_wav(tmp_path / "en1.wav")
    assert sr == 16000 and tuple(w.shape) == (1, len(en1))
    assert np.array_equal(w[0].numpy(), en1.astype(np.float32) / np.float32(32768.0))


# ---- the filter bank ----------------------------------------------------------------------------------------------------------
def dense_f64(orig, new, lpw=6, rolloff=0.99):
    """The definition, restated: K[p][j] = sinc(pi t) cos^2(pi t / (2 lpw)) base / o, t = clip((-p/n + (j - width)/o) base, +-lpw)."""
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    K = np.empty((n, 2 * width + o), dtype=np.float64)
    for p in range(n):
        for j in range(2 * width + o):
            t = min(max((-p / n + (j - width) / o) * base, -lpw), lpw)
            s = 1.0 if t == 0 else math.sin(math.pi * t) / (math.pi * t)
            K[p, j] = s * math.cos(math.pi * t / (2 * lpw)) ** 2 * base / o
    return o, n, width, K


@pytest.mark.parametrize("pair,width", list(zip(PAIRS, WIDTHS)))
def test_filter_bank_dense_and_compact(pair, width):
    o, n, w, K = dense_f64(*pair)
    k = A.resample_kernel(*pair)
    assert (k.o, k.n, k.width, k.L) == (o, n, width, 2 * width + 2) and w == width
    assert k.dense.dtype == np.float32 and k.dense.shape == K.shape
    # float32 rounding of a float64 value computed along another route: half an ulp for the rounding, and the two float64
    # evaluations apart by a few 1e-16 relative (sin near a multiple of pi: absolute 1e-16 of a tap scale of <= 1)
    assert np.all(np.abs(k.dense.astype(np.float64) - K) <= 2.0 ** -24 * np.abs(K) + 1e-15)
    assert K[0, width] == min(o, n) * 0.99 / o and k.dense[0, width] == np.float32(K[0, width])         # sinc(0) = 1 exactly
    # the compact rows, put back at starts[p], are the dense table; what they leave out is nothing
    assert k.taps.dtype == np.float32 and k.taps.shape == (n, k.L) and k.starts.dtype == np.int32 and k.starts.shape == (n,)
    rebuilt = np.zeros((n, K.shape[1] + k.L), dtype=np.float32)
    covered = np.zeros(rebuilt.shape, dtype=bool)
    for p in range(n):
        s = int(k.starts[p])
        assert 0 <= s
        rebuilt[p, s:s + k.L] = k.taps[p]
        covered[p, s:s + k.L] = True
    assert np.array_equal(rebuilt[:, :K.shape[1]][covered[:, :K.shape[1]]], k.dense[covered[:, :K.shape[1]]])
    assert not rebuilt[:, K.shape[1]:].any()                                         # beyond the dense row: zero padding
    left_out = ~covered[:, :K.shape[1]]
    assert np.abs(K[left_out]).max(initial=0.0) < 1e-30 and np.abs(k.dense[left_out]).max(initial=0.0) < 1e-30
    assert A.resample_kernel(*pair) is k                                             # cached


def test_filter_bank_arguments():
    assert A.resample_kernel(44100.0, 16000).o == 441
    for bad in ((0, 16000), (16000, -1), (16000.5, 8000), ("16000", 8000), (True, 8000)):
        with pytest.raises(ValueError):
            A.resample_kernel(*bad)
        with pytest.raises(ValueError):
            A.resample(torch.zeros(8), *bad)
    with pytest.raises(ValueError):
        A.resample_kernel(16000, 8000, lowpass_filter_width=0)
    k = A.resample_kernel(16000, 8000, lowpass_filter_width=4, rolloff=0.9)
    assert k.width == math.ceil(4 * 2 / 0.9) and k.L == 2 * k.width + 2


@pytest.mark.parametrize("pair", PAIRS)
def test_output_length_helper(lib, pair):
    g = math.gcd(*pair)
    o, n = pair[0] // g, pair[1] // g
    for length in sorted({1, max(o - 1, 1), o, o + 1, 3 * o, 2 ** 31 - 1}):
        want = -((-n * length) // o)
        assert lib.v100_resample_out_len(length, o, n) == want
        assert A.resample_out_len(length, *pair) == want
    assert lib.v100_resample_out_len(0, o, n) == 0
    assert lib.v100_resample_out_len(-1, o, n) == -1 and lib.v100_resample_out_len(5, 0, n) == -1 and lib.v100_resample_out_len(5, o, 0) == -1


def test_entry_points_without_a_gpu(lib):
    assert A.resample_tile() == lib.v100_resample_tile() >= 64
    with pytest.raises(RuntimeError):
        A.resample(torch.zeros(1000), 44100, 16000)
    with pytest.raises(RuntimeError):
        A.resample(torch.zeros(2, 1000), 44100, 16000, lengths=torch.tensor([1000, 10]))
    x = torch.zeros(1000)
    assert A.resample(x, 16000, 16000) is x
    assert A.resample(x, 32000, 32000.0) is x
    y, lens = A.resample(x[None], 8000, 8000, lengths=[7])
    assert y.data_ptr() == x.data_ptr() and lens.dtype == torch.int32 and lens.tolist() == [7]
    # status codes are returned before anything touches a device
    one = 16
    assert lib.v100_resample_sinc(None, None, one, one, one, None, 1, 8, 4, 2, 1, 13, 28, None) == 3
    assert lib.v100_resample_sinc(one, None, None, one, one, None, 1, 8, 4, 2, 1, 13, 28, None) == 3
    assert lib.v100_resample_sinc(one, None, one, None, one, None, 1, 8, 4, 2, 1, 13, 28, None) == 3
    assert lib.v100_resample_sinc(one, None, one, one, None, None, 1, 8, 4, 2, 1, 13, 28, None) == 3
    for B, Nmax, Mmax, o, n, width, L in ((0, 8, 4, 2, 1, 13, 28), (1, 0, 4, 2, 1, 13, 28), (1, 8, 0, 2, 1, 13, 28), (1, 8, 4, 0, 1, 13, 28),
                                          (1, 8, 4, 2, 0, 13, 28), (1, 8, 4, 2, 1, 0, 28), (1, 8, 4, 2, 1, 13, 0), (65536, 8, 4, 2, 1, 13, 28)):
        assert lib.v100_resample_sinc(one, None, one, one, one, None, B, Nmax, Mmax, o, n, width, L, None) == 1


def test_file_paths_need_the_gpu_too(tmp_path):
    """No CPU fallback behind a path either: a module left on the CPU raises the package's RuntimeError."""
    from voice100_amd.mel import MelSpectrogramAudioTransform
    v = np.zeros((4410, 1), dtype=np.int16)
    write_stdlib(tmp_path / "z.wav", v, 2, 44100)
    with pytest.raises(RuntimeError):
        MelSpectrogramAudioTransform()(str(tmp_path / "z.wav"))
    assert A.WORLDAudioProcessor(16000, True).audio_size == 1 + 25 + 1
    assert A.WORLDAudioProcessor(16000, False).audio_size == 1 + 257 + 1
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            A.WORLDAudioProcessor(16000, False)(str(tmp_path / "z.wav"))
