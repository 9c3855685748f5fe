"""The device resampler (csrc/resample.hip) element by element against the dense definition in float64, and the two file
entry points end to end.

Oracle: y[q n + p] = sum_j K[p][j] x[q o + j - width] with x zero outside the utterance, K the float64 table of the published
definition of torchaudio.functional.resample's default method (restated below, not taken from audio_io), applied to the float32
input.  Bound, for every output: |y_dev - y_64| <= (L + 3) 2^-24 sum_j |K[p][j]| |x_j| + 1e-38 -- the kernel makes L fp32
accumulation steps (L = 2 width + 2 taps kept per phase), rounds each product at most once and uses a table rounded to fp32 once;
each of those is at most 2^-24 of sum |K| |x|.  1e-38 is for outputs that are exactly zero in one of the two.
"""
import math
import os
import wave

import numpy as np
import pytest
import torch

from voice100_amd import _native as N
from voice100_amd import audio_io as A

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(44100, 16000), (48000, 16000), (8000, 16000), (22050, 16000), (16000, 22050), (32000, 16000), (11025, 16000),
         (24000, 16000), (16000, 24000)]
LPW, ROLLOFF = 6, 0.99
_tables = {}


def table_f64(orig, new):
    """(o, n, width, K [n, 2 width + o] float64) of the definition."""
    ent = _tables.get((orig, new))
    if ent is None:
        g = math.gcd(orig, new)
        o, n = orig // g, new // g
        base = min(o, n) * ROLLOFF
        width = math.ceil(LPW * o / base)
        p = np.arange(n, dtype=np.float64)[:, None]
        j = np.arange(2 * width + o, dtype=np.float64)[None, :]
        t = np.clip((-p / n + (j - width) / o) * base, -LPW, LPW)
        with np.errstate(invalid="ignore", divide="ignore"):
            sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
        ent = _tables[(orig, new)] = (o, n, width, sinc * np.cos(np.pi * t / (2 * LPW)) ** 2 * base / o)
    return ent


def out_len(length, o, n):
    return -((-n * length) // o)


def oracle(x32, orig, new):
    """(y float64 [ceil(n len / o)], bound) for one utterance x32 (float32 numpy)."""
    o, n, width, K = table_f64(orig, new)
    M = out_len(len(x32), o, n)
    Q = -(-M // n)
    xp = np.zeros(Q * o + 2 * width, dtype=np.float64)
    m = min(len(x32), len(xp) - width)
    xp[width:width + m] = x32[:m]                     # samples past the last window are not read by any output
    frames = np.lib.stride_tricks.as_strided(xp, (Q, 2 * width + o), (o * xp.strides[0], xp.strides[0]), writeable=False)
    y = (frames @ K.T).reshape(-1)[:M]
    mag = (np.abs(frames) @ np.abs(K).T).reshape(-1)[:M]
    return y, (2 * width + 2 + 3) * 2.0 ** -24 * mag + 1e-38


def tile_edge_length(target, o, n):
    """The shortest utterance with at least `target` outputs (exactly `target` wherever some length gives that count: every
    count when downsampling; an upsampler's counts step by more than one)."""
    length = (target - 1) * o // n + 1
    assert out_len(length, o, n) >= target and (length == 1 or out_len(length - 1, o, n) < target)
    return length


def lengths_for(orig, new):
    o, n, width, _ = table_f64(orig, new)
    tile = A.resample_tile()
    ls = {1, 2, width - 1, width, width + 1, o - 1, o, o + 1, 3 * o, 3 * o - 1, 3 * o + 1}
    ls |= {tile_edge_length(t, o, n) for t in (tile - 1, tile, tile + 1, 2 * tile + 1)}
    if orig in (44100, 22050):
        ls.add(orig)                                  # about one second, the 441-to-something pairs only
    return sorted(l for l in ls if l >= 1)


def signals(length, rng):
    out = {"noise": rng.standard_normal(length).astype(np.float32), "ones": np.ones(length, dtype=np.float32)}
    for name, at in (("impulse_first", 0), ("impulse_last", length - 1), ("impulse_mid", length // 2)):
        x = np.zeros(length, dtype=np.float32)
        x[at] = 1.0
        out[name] = x
    return out


def compare(got, x, orig, new, what):
    y, bound = oracle(x, orig, new)
    assert got.dtype == np.float32 and got.shape == y.shape, (what, got.shape, y.shape)
    err = np.abs(got.astype(np.float64) - y)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{what}: output {worst} of {len(y)}: got {got[worst]!r}, float64 {y[worst]!r}, bound {bound[worst]:.3e}"
    return float((err / bound).max())


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_every_output_within_the_derived_bound(cuda, pair):
    orig, new = pair
    rng = np.random.default_rng(orig + new)
    worst = 0.0
    for length in lengths_for(orig, new):
        for name, x in signals(length, rng).items():
            got = A.resample(torch.from_numpy(x).to(cuda), orig, new)
            assert got.is_cuda and got.dim() == 1
            worst = max(worst, compare(got.cpu().numpy(), x, orig, new, f"{orig}->{new} len {length} {name}"))
    print(f"{orig}->{new}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_ragged_batch_in_one_launch(cuda, pair):
    orig, new = pair
    o, n, width, _ = table_f64(orig, new)
    tile = A.resample_tile()
    lens = [1, o + 1, tile_edge_length(tile + 1, o, n), 3 * o, tile_edge_length(2 * tile + 1, o, n) + 3 * o]
    B, Nmax = len(lens), max(lens)
    rng = np.random.default_rng(7 * orig + new)
    x = np.full((B, Nmax), np.nan, dtype=np.float32)                  # what lies beyond a row's length must never be read
    for b, l in enumerate(lens):
        x[b, :l] = rng.standard_normal(l).astype(np.float32)
    xd = torch.from_numpy(x).to(cuda)
    singles = [A.resample(torch.from_numpy(x[b, :l].copy()).to(cuda), orig, new).cpu().numpy() for b, l in enumerate(lens)]
    want_lens = [out_len(l, o, n) for l in lens]
    Mmax = out_len(Nmax, o, n)
    # the launch itself, into an output filled with a sentinel
    k = A.resample_kernel(orig, new)
    taps, starts = torch.from_numpy(k.taps.copy()).to(cuda), torch.from_numpy(k.starts.copy()).to(cuda)
    y = torch.full((B, Mmax), 777.0, dtype=torch.float32, device=cuda)
    ol = torch.full((B,), -5, dtype=torch.int32, device=cuda)
    before = N.launch_count()
    N.call("v100_resample_sinc", xd, torch.tensor(lens, dtype=torch.int32, device=cuda), taps, starts, y, ol, B, Nmax, Mmax,
           k.o, k.n, k.width, k.L)
    assert N.launch_count() - before == 1
    y = y.cpu().numpy()
    assert ol.cpu().tolist() == want_lens
    for b, (m, single) in enumerate(zip(want_lens, singles)):
        assert len(single) == m
        assert np.array_equal(y[b, :m].view(np.uint32), single.view(np.uint32)), f"row {b} differs from its single-utterance run"
        assert not y[b, m:].view(np.uint32).any(), f"row {b} is not exactly zero beyond its length"
        compare(y[b, :m], x[b, :lens[b]], orig, new, f"{orig}->{new} ragged row {b}")
    # the public entry point: lengths on the host or on the device, the same bits
    for lengths in (lens, torch.tensor(lens, device=cuda)):
        y2, ol2 = A.resample(xd, orig, new, lengths=lengths)
        assert y2.shape == (B, Mmax) and ol2.is_cuda and ol2.dtype == torch.int32 and ol2.cpu().tolist() == want_lens
        assert np.array_equal(y2.cpu().numpy().view(np.uint32), y.view(np.uint32))


def test_null_lengths_and_status_codes(cuda):
    orig, new = 44100, 16000
    k = A.resample_kernel(orig, new)
    taps, starts = torch.from_numpy(k.taps.copy()).to(cuda), torch.from_numpy(k.starts.copy()).to(cuda)
    B, Nmax = 3, 2 * k.o + 5
    Mmax = out_len(Nmax, k.o, k.n)
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((B, Nmax)).astype(np.float32)).to(cuda)
    ys = []
    for lens in (None, torch.full((B,), Nmax, dtype=torch.int32, device=cuda)):
        y = torch.full((B, Mmax), 777.0, dtype=torch.float32, device=cuda)
        ol = torch.full((B,), -5, dtype=torch.int32, device=cuda)
        N.call("v100_resample_sinc", x, lens, taps, starts, y, ol, B, Nmax, Mmax, k.o, k.n, k.width, k.L)
        assert ol.cpu().tolist() == [Mmax] * B
        ys.append(y.cpu().numpy())
    assert np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32))
    for b in range(B):
        compare(ys[0][b], x[b].cpu().numpy(), orig, new, f"NULL lens row {b}")
    assert np.array_equal(A.resample(x, orig, new).cpu().numpy().view(np.uint32), ys[0].view(np.uint32))       # [B, N] without lengths
    # out_lens is optional
    y = torch.full((B, Mmax), 777.0, dtype=torch.float32, device=cuda)
    N.call("v100_resample_sinc", x, None, taps, starts, y, None, B, Nmax, Mmax, k.o, k.n, k.width, k.L)
    assert np.array_equal(y.cpu().numpy().view(np.uint32), ys[0].view(np.uint32))
    # status codes, with real device pointers everywhere else; neither launches anything
    lib = N.load()
    before = N.launch_count()
    args = (None, taps.data_ptr(), starts.data_ptr(), y.data_ptr(), None, B, Nmax, Mmax)
    assert lib.v100_resample_sinc(None, *args, k.o, k.n, k.width, k.L, N.stream_ptr()) == 3
    assert lib.v100_resample_sinc(x.data_ptr(), *args, 0, k.n, k.width, k.L, N.stream_ptr()) == 1
    assert lib.v100_resample_sinc(x.data_ptr(), *args, -k.o, k.n, k.width, k.L, N.stream_ptr()) == 1
    assert N.launch_count() == before
    torch.cuda.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.uint32), ys[0].view(np.uint32))


# ---- from a file path ---------------------------------------------------------------------------------------------------------
def write_pcm16(path, ints, rate):
    """ints [frames, channels] int16 -> a WAV file, through stdlib `wave`."""
    with wave.open(str(path), "wb") as w:
        w.setnchannels(ints.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(ints.astype("<i2")).tobytes())


def tone_and_noise(frames, rate, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / rate
    ch0 = 0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.05 * rng.standard_normal(frames)
    ch1 = 0.3 * rng.standard_normal(frames)                           # a second channel that must not leak into the result
    return np.round(np.clip(np.stack([ch0, ch1], axis=1), -1.0, 1.0) * 32767.0).astype(np.int16)


def test_mel_from_a_file_path(cuda, tmp_path):
    from voice100_amd.mel import MelSpectrogramAudioTransform
    mel = MelSpectrogramAudioTransform().to(cuda)
    frames = 22050
    v = tone_and_noise(frames, 44100, 11)
    path = tmp_path / "stereo_44k.wav"
    write_pcm16(path, v, 44100)
    got = mel(str(path))
    w, sr = A.load_wav(path)
    assert sr == 44100 and tuple(w.shape) == (2, frames)
    want = mel.transform(A.resample(w[0].to(cuda), 44100, 16000))
    assert got.is_cuda and tuple(got.shape) == (1 + (-(-160 * frames // 441)) // 160, 64)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())
    # the resampled waveform that went in is the oracle's, within the bound
    compare(A.resample(w[0].to(cuda), 44100, 16000).cpu().numpy(), w[0].numpy(), 44100, 16000, "file 44100->16000")
    # the same samples as a 16 kHz mono file: no resampling launch
    path16 = tmp_path / "mono_16k.wav"
    write_pcm16(path16, v[:, :1], 16000)
    samples = torch.from_numpy(v[:, 0].astype(np.float32) / np.float32(32768.0)).to(cuda)
    c0 = N.launch_count()
    want16 = mel.transform(samples)
    c1 = N.launch_count()
    got16 = mel(str(path16))
    c2 = N.launch_count()
    assert torch.equal(got16, want16) and tuple(got16.shape) == (1 + frames // 160, 64)
    assert c2 - c1 == c1 - c0 >= 1


def test_world_features_from_a_file_path(cuda, tmp_path):
    from voice100_amd.vocoder import WORLDVocoder
    en1 = np.load(os.path.join(ROOT, "tests", "golden", "world_ref_samples.npz"))["en1"].astype(np.float32) / np.float32(32768.0)
    up, _ = oracle(en1, 16000, 22050)                                 # the reference's sample as a 22.05 kHz recording
    v = np.round(np.clip(up, -1.0, 1.0) * 32767.0).astype(np.int16)
    path = tmp_path / "en1_22k.wav"
    write_pcm16(path, v[:, None], 22050)
    for use_mcep in (False, True):
        proc = A.WORLDAudioProcessor(16000, use_mcep=use_mcep)
        f0, feat, codeap = proc(str(path))
        w, sr = A.load_wav(path)
        assert sr == 22050
        x = A.resample(w[0].to(cuda), 22050, 16000)
        voc = WORLDVocoder(16000, use_mcep=use_mcep)
        T = voc.frames(x.shape[0])
        assert x.shape[0] == out_len(len(v), 441, 320)
        want = voc.encode(x)
        for got, ref, shape in zip((f0, feat, codeap), want, ((T,), (T, 25 if use_mcep else 257), (T, 1))):
            assert not got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == shape
            assert torch.equal(got, ref)
        assert int((f0 > 0).sum()) > T // 10                          # voiced speech came through
    assert A.WORLDAudioProcessor(16000, True).audio_size == 1 + 25 + 1
