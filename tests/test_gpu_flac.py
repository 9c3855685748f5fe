"""FLAC decoded on the device (csrc/flac.hip, audio_io.decode_flac / load_flac / load_batch) against the reference decoder of
tests/_flac_ref.py.  The format is lossless: every comparison is torch.equal, on the int32 PCM and on float32 = pcm / 2^(bits - 1).
The whole case list of tests/_flac_cases.py -- the three RFC examples, every subframe type, LPC orders / precisions / shifts with
coefficients at the ends of their range, five sample widths, every residual form, wasted bits, every channel assignment, the block
sizes and header forms, 2,100 frames under fixed blocking, variable blocking, payloads that spell frame headers -- is decoded ONCE
as one mixed batch (different rates, widths, channel counts and lengths in one call), and the tests below read that result."""
import wave

import numpy as np
import pytest
import torch

import _flac_cases as K
import _flac_ref as R
from voice100_amd import audio_io as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def reference():
    """The reference decoder's PCM per case (computed once; the encoder's own input is compared with it on the CPU side)."""
    out = {}
    for c in K.cases():
        d = R.decode(c.data)
        assert d.md5_ok is True
        out[c.name] = torch.from_numpy(d.pcm)
    return out


@pytest.fixture(scope="module")
def batch(cuda):
    cs = K.cases()
    wave_, lengths, rates, pcm = A.decode_flac([c.data for c in cs], cuda, channels="all", verify_md5=True, return_pcm=True)
    first, first_len, _ = A.decode_flac([c.data for c in cs], cuda)
    return {"cases": cs, "wave": wave_.cpu(), "lengths": lengths.cpu(), "rates": rates, "pcm": pcm.cpu(), "first": first.cpu(),
            "first_len": first_len.cpu()}


def _check(batch, reference, names):
    cs = batch["cases"]
    assert names
    for b, c in enumerate(cs):
        if c.name not in names:
            continue
        want = reference[c.name]
        C, n = want.shape
        assert int(batch["lengths"][b]) == n and batch["rates"][b] == c.rate, c.name
        assert torch.equal(batch["pcm"][b, :C, :n], want), c.name
        scale = np.float32(2.0 ** (c.bits - 1))
        assert torch.equal(batch["wave"][b, :C, :n], want.to(torch.float32) / scale), c.name
        assert torch.equal(batch["first"][b, :n], want[0].to(torch.float32) / scale), c.name
        # exact zeros beyond the file's length and in the channels it does not have
        assert not batch["pcm"][b, :, n:].any() and not batch["pcm"][b, C:].any(), c.name
        assert not batch["wave"][b, :, n:].any() and not batch["wave"][b, C:].any() and not batch["first"][b, n:].any(), c.name


def _names(prefix):
    return [c.name for c in K.cases() if c.name.startswith(prefix)]


def test_the_batch_is_mixed(batch):
    cs = batch["cases"]
    assert batch["wave"].shape == (len(cs), 8, max(c.pcm.shape[1] for c in cs)) and batch["wave"].dtype == torch.float32
    assert batch["pcm"].dtype == torch.int32 and batch["lengths"].dtype == torch.int32 and batch["first"].dim() == 2
    assert len(set(batch["rates"])) >= 11 and len({c.bits for c in cs}) == 5 and len({c.pcm.shape[0] for c in cs}) == 4
    assert batch["lengths"].tolist() == [c.pcm.shape[1] for c in cs] and torch.equal(batch["lengths"], batch["first_len"])


def test_rfc_examples(batch, reference, tmp_path):
    _check(batch, reference, _names("rfc_"))
    for name, hx, pcm, rate, bits in K.VECTORS:
        p = tmp_path / f"{name}.flac"
        p.write_bytes(bytes.fromhex(hx))
        w, sr = A.load_flac(p, verify_md5=True)
        assert sr == rate and w.dtype == torch.float32 and not w.is_cuda
        assert torch.equal(w, torch.tensor(pcm, dtype=torch.float32) / 2.0 ** (bits - 1)), name
        w2, sr2 = A.load_audio(p)
        assert sr2 == rate and torch.equal(w2, w)


def test_every_subframe_type(batch, reference):
    _check(batch, reference, ["types16"])


def test_lpc_orders_precisions_shifts_and_the_64_bit_accumulator(batch, reference):
    _check(batch, reference, ["lpc_cross", "lpc_wide24"])


def test_sample_widths_coded_in_the_header_and_taken_from_streaminfo(batch, reference):
    assert len(_names("bits")) == 10
    _check(batch, reference, _names("bits"))


def test_residual_forms(batch, reference):
    _check(batch, reference, ["residual_forms"])


def test_wasted_bits_on_plain_and_side_channels(batch, reference):
    _check(batch, reference, ["wasted"])


def test_channel_assignments(batch, reference):
    _check(batch, reference, ["stereo", "channels3", "channels8"])
    x = reference["stereo"]
    assert ((x[0] + x[1]) % 2 == 1).any() and ((x[0] + x[1]) % 2 == 0).any()      # odd and even mid + side sums


def test_block_sizes_and_header_forms(batch, reference):
    assert len(_names("block")) == 8 and len(_names("rate")) == 12
    _check(batch, reference, _names("block") + _names("rate"))


def test_frame_and_sample_numbering(batch, reference):
    _check(batch, reference, ["frames2100", "block_codes_variable"])


def test_false_candidates_decode_to_the_payload(batch, reference):
    _check(batch, reference, ["false_header", "false_frame"])
    # alone too: the spelled frames are real candidates for the scan, and stay off the chain
    for name in ("false_header", "false_frame"):
        c = next(c for c in K.cases() if c.name == name)
        _, _, _, pcm = A.decode_flac([c.data], channels="all", return_pcm=True, verify_md5=True)
        assert torch.equal(pcm[0].cpu(), reference[name])


def test_md5_mismatch_is_reported(cuda):
    c = next(c for c in K.cases() if c.name == "types16")
    bad = bytearray(c.data)
    bad[8 + 18] ^= 0xFF                                                # STREAMINFO's MD5
    with pytest.raises(ValueError, match="<bytes #1>: FLAC MD5 mismatch"):
        A.decode_flac([c.data, bytes(bad)], cuda, verify_md5=True)
    A.decode_flac([c.data, bytes(bad)], cuda)                          # not asked: not checked


def test_refusals_name_file_and_frame_and_disturb_no_other_row(cuda, reference, tmp_path):
    data, _, _, pcm = K.refusal_base()
    other = next(c for c in K.cases() if c.name == "rfc_2")
    want = torch.from_numpy(pcm)
    for name, damaged, frame, word in K.refusals():
        p = tmp_path / f"{name}.flac"
        p.write_bytes(damaged)
        with pytest.raises(ValueError) as e:
            A.decode_flac([other.data, str(p), data], cuda)
        msg = str(e.value)
        assert str(p) in msg and word in msg and (f"frame {frame}" in msg or f"after {frame} frames" in msg), msg
        # the device's own answer: the damaged file has a status, its neighbours decode as if it were not there
        wave_, lengths, got, st, _, _ = A._flac_decode_device([other.data, damaged, data], cuda, "all", True)
        assert st[0, 0] == 0 and st[2, 0] == 0 and st[1, 0] != 0 and st[1, 1] == frame, (name, st)
        assert torch.equal(got[0, :2, :19].cpu(), reference["rfc_2"]) and torch.equal(got[2, :1, :768].cpu(), want)
        assert not got[0, :, 19:].any() and not got[2, 1:].any()
    with pytest.raises(ValueError, match="frame 2 fails its CRC-16"):
        A.load_flac(tmp_path / "flipped_bit.flac")


def _write_wav(path, pcm, rate):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(pcm.shape[0])
        f.setsampwidth(2)
        f.setframerate(rate)
        f.writeframes(np.ascontiguousarray(pcm.T).astype("<i2").tobytes())


def _write_flac(path, pcm, rate, bs=1152):
    pcm = np.asarray(pcm, np.int64)
    frames = []
    for at in range(0, pcm.shape[1], bs):
        n = min(bs, pcm.shape[1] - at)
        subs = [R.rice_params(ch[at:at + n], R.Sub("fixed", order=min(2, n), method=0), n) for ch in pcm]
        frames.append(R.Frame(n, subs))
    path.write_bytes(R.encode(pcm, rate, 16, frames))


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """The same 16-bit PCM as WAV and as FLAC: (rate, channels, samples)."""
    root = tmp_path_factory.mktemp("flac_wav_pairs")
    rng = np.random.default_rng(5)
    wavs, flacs = [], []
    for k, (rate, channels, n) in enumerate(((16000, 1, 5000), (44100, 2, 7001), (16000, 1, 2333), (44100, 1, 4410), (8000, 1, 1200))):
        pcm = (rng.standard_normal((channels, n)) * 4000).astype(np.int16)
        _write_wav(root / f"u{k}.wav", pcm, rate)
        _write_flac(root / f"u{k}.flac", pcm, rate)
        wavs.append(str(root / f"u{k}.wav"))
        flacs.append(str(root / f"u{k}.flac"))
    return wavs, flacs


def test_load_batch_on_flac_equals_load_batch_on_wav(pairs, cuda):
    wavs, flacs = pairs
    want, want_len = A.load_batch(wavs, 16000, cuda)                   # 16 kHz rows copied through, 44.1 and 8 kHz rows resampled
    got, got_len = A.load_batch(flacs, 16000, cuda)
    assert torch.equal(got, want) and torch.equal(got_len, want_len) and got.dtype == torch.float32 and got_len.dtype == torch.int32
    same, same_len = A.load_batch([flacs[0], flacs[2]], 16000, cuda)   # already at the rate
    assert torch.equal(same, want[[0, 2], :5000]) and same_len.tolist() == [5000, 2333]
    mixed = [flacs[0], wavs[1], flacs[2], flacs[3], wavs[4], wavs[0], flacs[1]]
    got, got_len = A.load_batch(mixed, 16000, cuda)
    assert torch.equal(got, want[[0, 1, 2, 3, 4, 0, 1]]) and torch.equal(got_len, want_len[[0, 1, 2, 3, 4, 0, 1]])
    w, sr = A.load_flac(flacs[1], verify_md5=True)
    w2, sr2 = A.load_wav(wavs[1])
    assert sr == sr2 == 44100 and torch.equal(w, w2)                   # the shape and values torchaudio.load gives for either file
    with pytest.raises(ValueError, match="u9.flac"):
        bad = str(pairs[1][0]).replace("u0.flac", "u9.flac")
        open(bad, "wb").write(open(flacs[0], "rb").read()[:-40])
        A.load_batch([wavs[0], bad], 16000, cuda)


def test_transform_collate_and_pipeline_take_flac_paths(pairs, cuda):
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.data import AudioTextCollate
    from voice100_amd.infer import ASRPipeline
    from voice100_amd.mel import MelSpectrogramAudioTransform
    wavs, flacs = pairs
    tr = MelSpectrogramAudioTransform().to(cuda)
    assert torch.equal(tr(flacs[1]), tr(wavs[1]))                      # one path: load_audio, first channel, resample, transform
    gen = torch.Generator().manual_seed(1)
    texts = [torch.randint(1, 29, (n,), generator=gen) for n in (7, 12, 3, 9, 5)]
    collate = AudioTextCollate(tr)
    (a, al), (t, tl) = collate(list(zip(flacs, texts)))
    (a2, al2), (t2, tl2) = collate(list(zip(wavs, texts)))
    assert torch.equal(a, a2) and torch.equal(al, al2) and torch.equal(t, t2) and torch.equal(tl, tl2)
    torch.manual_seed(3)
    model = AudioToTextCTC(64, 32, 29, 64).to(cuda).eval()
    pipe = ASRPipeline(model, tr)
    alphabet = "_abcdefghijklmnopqrstuvwxyz' "

    def decode(ids):
        return "".join(alphabet[int(i)] for i in ids)
    assert pipe.transcribe(flacs, decode) == pipe.transcribe(wavs, decode)
