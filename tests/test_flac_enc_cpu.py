"""The FLAC encoder (K30) without a GPU: the numpy mirror of its search (tests/_flac_enc_ref.py) round-trips through the reference
decoder and keeps its size theorems, the resonance fixture shows that the LPC candidates earn their place, save_wav / load_wav /
stdlib wave agree at 8, 16 and 24 bits, every refusal of the writers is raised, and the kernels' own per-lane bodies -- compiled as a
plain host program from tools/flac_enc_host.cpp, no sanitizer here -- produce the mirror's bytes on the whole case list."""
import os
import shutil
import struct
import subprocess
import wave

import numpy as np
import pytest
import torch

import _flac_enc_cases as K
import _flac_enc_ref as M
import _flac_ref as R
from voice100_amd import audio_io as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def encoded():
    return [M.encode(c.pcm, c.rate, c.bits, c.block_size, c.max_lpc_order, c.max_partition_order, md5=True) for c in K.cases()]


def test_mirror_round_trips_and_keeps_its_size_order(encoded):
    names = [c.name for c in K.cases()]
    assert len(set(names)) == len(names) >= 40
    for c, e in zip(K.cases(), encoded):
        d = R.decode(e.data)
        assert np.array_equal(d.pcm, c.pcm) and d.md5_ok is True, c.name
        assert d.sample_rate == c.rate and d.bits_per_sample == c.bits, c.name
        fi = A.flac_info(e.data)
        assert (fi.min_blocksize, fi.max_blocksize, fi.total_samples) == (c.block_size, c.block_size, c.pcm.shape[1]), c.name
        assert len(e.frames) == -(-c.pcm.shape[1] // c.block_size) <= 3, c.name
        for b, f, v, nbytes in zip(e.bits, e.fixed_bits, e.verbatim_bits, e.frame_bytes):
            assert b <= f <= v, (c.name, b, f, v)
            assert nbytes <= 15 + (v + 7) // 8 + 2, c.name
    by = {c.name: e for c, e in zip(K.cases(), encoded)}
    assert [s.kind for s in by["noise"].frames[0].subs] == ["verbatim"]                 # full-scale white noise: verbatim wins
    assert [s.kind for s in by["zeros"].frames[0].subs] == ["constant"] and by["shifted3"].frames[0].subs[0].wasted == 3
    assert by["stereo_identical"].frames[0].assign in (8, 9, 10) and by["stereo_independent"].frames[0].assign == 1
    assert by["w24_resonance"].frames[0].subs[0].kind == "lpc" and by["w24_resonance"].frames[0].subs[0].order > 8


@pytest.mark.parametrize("block", [4096, 1024])
def test_lpc_beats_the_fixed_predictors_on_the_resonance_fixture(block):
    for seed in range(4):
        x = K.resonance(block, seed)
        e = M.encode(x[None], 16000, 16, block_size=block, max_lpc_order=12)
        ratio = sum(e.bits) / sum(e.fixed_bits)
        print(f"resonance fixture, {block} samples, seed {seed}: LPC order {e.frames[0].subs[0].order}, {ratio:.3f} of the fixed-only optimum")
        assert e.frames[0].subs[0].kind == "lpc" and ratio <= 0.85


@pytest.mark.parametrize("bits", [8, 16, 24])
def test_save_wav_load_wav_and_stdlib_wave_agree(tmp_path, bits):
    rng = np.random.default_rng(bits)
    full = 1 << (bits - 1)
    q = rng.integers(-full, full, (2, 301)).astype(np.int32)
    q[:, :4] = [[-full, full - 1, 0, -1]] * 2
    p = tmp_path / "a.wav"
    A.save_wav(p, torch.from_numpy(q.astype(np.float32) / full), 22050, bits)            # exact in float32 up to 24 bits
    got, sr = A.load_wav(p)
    assert sr == 22050 and np.array_equal(np.rint(got.numpy().astype(np.float64) * full).astype(np.int32), q)
    with wave.open(str(p), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (2, bits // 8, 22050, 301)
        raw = np.frombuffer(f.readframes(301), np.uint8).reshape(301, 2, bits // 8).astype(np.int64)
    v = sum(raw[:, :, k] << (8 * k) for k in range(bits // 8))
    v = v - 128 if bits == 8 else (v ^ full) - full
    assert np.array_equal(v.T, q)
    # integer PCM goes in unchanged, a mono [samples] tensor is one channel, and the quantiser rounds ties to even and clamps
    A.save_wav(p, torch.from_numpy(q[0]), 8000, bits)
    got, sr = A.load_wav(p)
    assert got.shape == (1, 301) and np.array_equal(np.rint(got.numpy().astype(np.float64) * full).astype(np.int32), q[:1])
    ties = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, 3e9, -3e9]) / full
    A.save_wav(p, ties, 8000, bits)
    got, _ = A.load_wav(p)
    assert np.rint(got.numpy()[0].astype(np.float64) * full).tolist() == [0, 2, 2, 0, -2, full - 1, -full]
    if bits == 16:
        with wave.open(str(tmp_path / "b.wav"), "wb") as f:
            f.setnchannels(2)
            f.setsampwidth(2)
            f.setframerate(22050)
            f.writeframes(q.T.astype("<i2").tobytes())
        A.save_wav(p, torch.from_numpy(q), 22050, 16)
        assert p.read_bytes() == (tmp_path / "b.wav").read_bytes()                       # the same file stdlib wave writes


def test_writers_refuse_what_they_cannot_write(tmp_path):
    x = torch.zeros(2, 64)
    with pytest.raises(ValueError, match="item 1 has length 0"):
        A.encode_flac(x, [64, 0])
    with pytest.raises(ValueError, match="item 0 has 2147483648 samples"):
        A.encode_flac(x, [2 ** 31, 5])
    with pytest.raises(ValueError, match="item 1 .*outside the input"):
        A.encode_flac(x, [64, 65])
    with pytest.raises(ValueError, match="item 0 .*outside the input"):
        A.encode_flac(x, [8], rows=[2], starts=[0])
    with pytest.raises(ValueError, match="bits_per_sample must be 8, 16 or 24"):
        A.encode_flac(x, bits_per_sample=32)
    with pytest.raises(ValueError, match="1 or 2 channels"):
        A.encode_flac(torch.zeros(1, 3, 64))
    with pytest.raises(ValueError, match="sample_rate"):
        A.encode_flac(x, sample_rate=655351)
    with pytest.raises(ValueError, match="block_size 16 .. 4608"):
        A.encode_flac(x, block_size=8192)
    with pytest.raises(ValueError, match="max_lpc_order 0 .. 12"):
        A.encode_flac(x, max_lpc_order=13)
    with pytest.raises(ValueError, match="float32 or int32"):
        A.encode_flac(x.double())
    with pytest.raises(ValueError, match="more frames or bytes than one call indexes \\(at item 0"):
        A._flac_enc_plan([2 ** 30] * 4, range(4), [0] * 4, 4, 2 ** 30, 1, 16, 16)
    with pytest.raises(ValueError, match="one call indexes \\(at item 4"):
        A._flac_enc_plan([2 ** 22 * 16] * 8, range(8), [0] * 8, 8, 2 ** 26, 1, 16, 16)
    with pytest.raises(RuntimeError, match="GPU only"):                # a CPU tensor: there is no CPU encoder, with or without a device
        A.encode_flac(x)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):
            A.save_flac(tmp_path / "a.flac", x[0], 16000)
        with pytest.raises(RuntimeError, match="GPU only"):
            A.save_audio(tmp_path / "a.FLAC", x[0], 16000)
        with pytest.raises(RuntimeError, match="GPU only"):
            A.save_batch([tmp_path / "a.flac", tmp_path / "b.wav"], x, [64, 64], 16000)
    for name in ("a.mp3", "a", "a.flac.ogg"):
        with pytest.raises(ValueError, match="\\.wav or \\.flac"):
            A.save_audio(tmp_path / name, x[0], 16000)
    with pytest.raises(ValueError, match="\\.wav or \\.flac"):
        A.save_batch([tmp_path / "a.wav", tmp_path / "b.aiff"], x, [64, 64], 16000)
    with pytest.raises(ValueError, match="item 1 has length 0"):
        A.save_batch([tmp_path / "a.wav", tmp_path / "b.wav"], x, [64, 0], 16000)
    with pytest.raises(ValueError, match="bits_per_sample must be 8, 16 or 24"):
        A.save_wav(tmp_path / "a.wav", x, 16000, 12)
    with pytest.raises(ValueError, match="non-finite sample .*at sample 7"):
        bad = x.clone()
        bad[1, 7] = float("nan")
        A.save_wav(tmp_path / "a.wav", bad, 16000)
    with pytest.raises(ValueError, match="cannot be written"):
        A.save_wav(tmp_path / "a.wav", torch.zeros(1, 0), 16000)
    assert not os.listdir(tmp_path)                                    # every refusal came before a file was opened
    A.save_audio(tmp_path / "ok.WAV", x, 16000)                       # the extension is matched without regard to case
    assert A.load_wav(tmp_path / "ok.WAV")[0].shape == (2, 64)


def test_frame_table_layout():
    ftab, first, out_bytes = A._flac_enc_plan([1, 4096, 4097, 100], [3, 0, 0, 1], [5, 0, 10, 0], 4, 5000, 2, 16, 4096)
    assert first.tolist() == [0, 1, 2, 4, 5] and ftab.dtype == np.int32 and ftab.shape == (5, 8)
    assert ftab[:, :5].tolist() == [[3, 5, 1, 0, 0], [0, 0, 4096, 0, 1], [0, 10, 4096, 0, 2], [0, 4106, 1, 1, 2], [1, 0, 100, 0, 3]]
    assert out_bytes % 16 == 0 and out_bytes >= sum(18 + (16 + 33 * n + 7) // 8 for n in (1, 4096, 4096, 1, 100))
    assert A._flac_rate_code(16000) == (5, 0) and A._flac_rate_code(12345) == (13, 12345)
    assert A._flac_rate_code(655350) == (14, 65535) and A._flac_rate_code(100001) == (0, 0)


def test_pipeline_writers_refuse_without_writing(tmp_path):
    from voice100_amd.infer import TTSPipeline, cut_utterances
    chain = TTSPipeline(None, None, None)
    with pytest.raises(ValueError, match='no "wave"'):
        chain.save({"f0": torch.zeros(1, 4)}, [tmp_path / "a.wav"])
    wave_ = torch.zeros(16000)
    utt = {"start_s": 0.125, "end_s": 0.25}
    with pytest.raises(ValueError, match="alignment failed"):
        cut_utterances(wave_, 16000, {"ok": False, "utterances": [utt]}, [tmp_path / "a.wav"])
    with pytest.raises(ValueError, match="2 paths for 1 utterances"):
        cut_utterances(wave_, 16000, {"ok": True, "utterances": [utt]}, [tmp_path / "a.wav", tmp_path / "b.wav"])
    with pytest.raises(ValueError, match="utterance 0 .*holds no samples"):
        cut_utterances(wave_, 16000, {"ok": True, "utterances": [{"start_s": 2.0, "end_s": 2.5}]}, [tmp_path / "a.wav"])
    assert not os.listdir(tmp_path)
    got = cut_utterances(wave_, 16000, {"ok": True, "utterances": [utt, {"start_s": 0.9375, "end_s": 1.5}]},
                         [tmp_path / "a.wav", tmp_path / "b.wav"], pad_s=0.0625)         # WAV needs no GPU; the second is clamped
    assert got == [(1000, 5000), (14000, 16000)]
    assert A.load_wav(tmp_path / "a.wav")[0].shape == (1, 4000) and A.load_wav(tmp_path / "b.wav")[0].shape == (1, 2000)


def test_entry_point_refuses_null_pointers_and_bad_shapes():
    """v100_flac_encode returns a status before it touches a pointer or the device."""
    import ctypes
    from voice100_amd import _native as N
    lib = N.load()
    one = ctypes.c_void_p(16)
    good = dict(B=1, F=1, R=1, C=1, N=100, bits=16, bs=4096, lpc=8, po=6, code=5, extra=0, out_bytes=4096)

    def call(wave=one, pcm=None, ftab=one, ws=one, out=one, report=one, status=one, **kw):
        a = dict(good, **kw)
        return lib.v100_flac_encode(wave, pcm, ftab, ws, out, report, status, a["B"], a["F"], a["R"], a["C"], a["N"], a["bits"], a["bs"], a["lpc"],
                                    a["po"], a["code"], a["extra"], a["out_bytes"], None)
    assert call(wave=None, pcm=None) == 3
    for name in ("ftab", "ws", "out", "report", "status"):
        assert call(**{name: None}) == 3, name
    for bad in (dict(B=0), dict(F=0), dict(B=2), dict(F=(1 << 24) + 1), dict(R=0), dict(C=3), dict(N=0), dict(N=2 ** 31), dict(bits=12), dict(bits=32),
                dict(bs=15), dict(bs=4609), dict(lpc=13), dict(lpc=-1), dict(po=7), dict(code=12), dict(code=15), dict(extra=65536),
                dict(out_bytes=8), dict(out_bytes=4098), dict(out_bytes=2 ** 40)):
        assert call(**bad) == 1, bad
    assert lib.v100_flac_encode_workspace_bytes(0, 1) == -1 and lib.v100_flac_encode_workspace_bytes(1, 3) == -1
    assert lib.v100_flac_encode_workspace_bytes(1689, 1) >= 1689 * (36 * 4 + 16 + 8)
    assert lib.v100_flac_encode_workspace_bytes(10, 2) >= 10 * (4 * 36 * 4 + 16 + 8)


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_host_build_of_the_kernel_bodies_matches_the_mirror(tmp_path, encoded):
    """csrc/flac_enc.hip under FLAC_ENC_HOST_EMU: the same per-lane bodies the kernels run, one thread at a time."""
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler (CXX, c++, g++, clang++) on this machine")
    exe = tmp_path / "flac_enc_host"
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-w", "-I", os.path.join(ROOT, "voice100_amd", "csrc"),
                    os.path.join(ROOT, "tools", "flac_enc_host.cpp"), "-o", str(exe)], check=True)
    cases = K.cases()
    floats = {"len4097", "sine", "w8_resonance", "w24_resonance", "stereo_near"}     # these go in as float32, the others as int32
    with open(tmp_path / "in.bin", "wb") as f:
        for c in cases:
            code, extra = A._flac_rate_code(c.rate)
            is_float = c.name in floats
            f.write(np.array([c.pcm.shape[0], c.pcm.shape[1], c.bits, c.block_size, c.max_lpc_order, c.max_partition_order, code, extra,
                              is_float, 0], np.int32).tobytes())
            data = c.pcm.astype(np.float32) / np.float32(1 << (c.bits - 1)) if is_float else c.pcm.astype(np.int32)
            f.write(np.ascontiguousarray(data).tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True)
    raw, at = (tmp_path / "out.bin").read_bytes(), 0
    for c, e in zip(cases, encoded):
        code, _, nbytes = struct.unpack_from("<qqq", raw, at)
        got, at = raw[at + 24:at + 24 + nbytes], at + 24 + nbytes
        assert code == 0, c.name
        assert got == e.data[e.header_len:], (c.name, [M.describe(s) for s in e.frames[0].subs])
    assert at == len(raw)
    assert subprocess.run([str(exe), "--adversarial"], capture_output=True).returncode == 0
