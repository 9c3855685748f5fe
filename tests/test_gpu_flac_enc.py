"""The FLAC encoder on the device (csrc/flac_enc.hip, K30).  Everything is lossless, so every assertion is an equality: the files decode
to the integers they were made from through the reference decoder (tests/_flac_ref.py) and through the device's own decoder
(decode_flac), their bytes equal those of the numpy mirror of the search (tests/_flac_enc_ref.py, packed by _flac_ref.encode_frame),
a second call gives the same bytes, and the writers on top -- save_batch, TTSPipeline.save, cut_utterances -- return through
load_batch / load_audio what they were given.  One encode_flac call per (width, channels, rate, block size, search setting), built once."""
import numpy as np
import pytest
import torch

import _flac_enc_cases as K
import _flac_enc_ref as M
import _flac_ref as R

pytestmark = pytest.mark.gpu

FLOAT_GROUP = (16, 1, 16000, 4096, 8, 6)          # this group goes in as float32, the way a synthesised wave does; the others as int32 PCM


def _groups():
    groups = {}
    for c in K.cases():
        groups.setdefault((c.bits, c.pcm.shape[0], c.rate, c.block_size, c.max_lpc_order, c.max_partition_order), []).append(c)
    return groups


@pytest.fixture(scope="module")
def mirror():
    return {c.name: M.encode(c.pcm, c.rate, c.bits, c.block_size, c.max_lpc_order, c.max_partition_order, md5=True) for c in K.cases()}


def _encode_group(key, items, cuda):
    from voice100_amd.audio_io import encode_flac
    bits, C, rate, bs, lpc, po = key
    width = max(c.pcm.shape[1] for c in items)
    block = np.zeros((len(items), C, width), np.int32)
    for k, c in enumerate(items):
        block[k, :, :c.pcm.shape[1]] = c.pcm
    x = torch.from_numpy(block).to(cuda)
    if key == FLOAT_GROUP:
        x = x.float() / float(1 << (bits - 1))
    if C == 1:
        x = x[:, 0].contiguous()
    return encode_flac(x, [c.pcm.shape[1] for c in items], rate, bits, bs, lpc, po, md5=True)


@pytest.fixture(scope="module")
def device_files(cuda):
    out = {}
    for key, items in _groups().items():
        for c, data in zip(items, _encode_group(key, items, cuda)):
            out[c.name] = data
    return out


def _fields(data, at, bps, assign, n):
    """The predictor fields of the first subframe of the frame whose subframes begin at byte `at` (for a mismatch report)."""
    br = R._Bits(data, at)
    br.read(1)
    typ = br.read(6)
    wasted = br.unary() + 1 if br.read(1) else 0
    w = bps + (1 if assign == 9 else 0) - wasted
    if typ < 8:
        return f"type={typ} wasted={wasted}"
    order = typ - 8 if typ < 32 else (typ & 31) + 1
    for _ in range(order):
        br.read(w)
    extra = ""
    if typ >= 32:
        prec = br.read(4) + 1
        extra = f" precision={prec} shift={br.signed(5)} coefs={[br.signed(prec) for _ in range(order)]}"
    br.read(2)
    porder = br.read(4)
    return f"type={typ} order={order} wasted={wasted}{extra} porder={porder} first param={br.read(4)}"


def _explain(name, got, e, bps):
    """Where two files part: the first differing frame and its predictor fields on both sides."""
    if got[:e.header_len] != e.data[:e.header_len]:
        return f"{name}: the STREAMINFO blocks differ: {got[:e.header_len].hex()} vs {e.data[:e.header_len].hex()}"
    at = e.header_len
    for k, (size, fr) in enumerate(zip(e.frame_bytes, e.frames)):
        if got[at:at + size] != e.data[at:at + size]:
            hl = next(h for h in range(5, 17) if R.crc8(e.data[at:at + h]) == e.data[at + h]) + 1
            ga = got[at + 3] >> 4
            return (f"{name}: frame {k} differs; device: assign={ga} {_fields(got, at + hl, bps, ga, fr.bs)}; "
                    f"mirror: assign={e.data[at + 3] >> 4} {M.describe(fr.subs[0])}")
        at += size
    return f"{name}: {len(got)} bytes vs {len(e.data)}"


def test_files_decode_through_the_reference_decoder(device_files):
    for c in K.cases():
        d = R.decode(device_files[c.name])
        assert np.array_equal(d.pcm, c.pcm) and d.md5_ok is True, c.name
        assert (d.sample_rate, d.bits_per_sample) == (c.rate, c.bits), c.name


def test_files_decode_through_the_device_decoder(device_files):
    from voice100_amd.audio_io import decode_flac
    cases = K.cases()
    wave, lengths, rates, pcm = decode_flac([device_files[c.name] for c in cases], channels="all", verify_md5=True, return_pcm=True)
    pcm, lengths = pcm.cpu().numpy(), lengths.cpu().numpy()
    for b, c in enumerate(cases):
        C, n = c.pcm.shape
        assert lengths[b] == n and rates[b] == c.rate, c.name
        assert np.array_equal(pcm[b, :C, :n], c.pcm), c.name


def test_bytes_equal_the_mirror(device_files, mirror):
    for c in K.cases():
        got, e = device_files[c.name], mirror[c.name]
        if got != e.data:
            print(_explain(c.name, got, e, c.bits))
        assert got == e.data, c.name


def test_a_second_call_gives_the_same_bytes(device_files, cuda):
    groups = _groups()
    for key in (FLOAT_GROUP, (16, 2, 16000, 4096, 8, 6), (24, 1, 16000, 4096, 12, 6)):
        for c, data in zip(groups[key], _encode_group(key, groups[key], cuda)):
            assert data == device_files[c.name], c.name


def test_segments_of_one_row(cuda):
    from voice100_amd.audio_io import encode_flac
    x = K.resonance(8193, 0)
    row = torch.from_numpy(np.stack([np.zeros_like(x), x])).to(cuda)            # the segments come from row 1
    segs = [(0, 100), (50, 4096), (4000, 4193), (8192, 1)]
    files = encode_flac(row, [n for _, n in segs], rows=[1] * len(segs), starts=[a for a, _ in segs], md5=True)
    for (a, n), data in zip(segs, files):
        assert data == M.encode(x[a:a + n], 16000, 16, md5=True).data, (a, n)


def test_float_input_is_clamped_and_non_finite_input_is_refused(cuda):
    from voice100_amd.audio_io import encode_flac
    w = torch.zeros(2, 40, device=cuda)
    w[0, :6] = torch.tensor([1.5, -1.5, 0.25, 0.5 / 32768, 1.5 / 32768, -2.5 / 32768], device=cuda)
    w[1, 3] = 0.125
    files = encode_flac(w)
    assert R.decode(files[0]).pcm[0, :7].tolist() == [32767, -32768, 8192, 0, 2, -2, 0]
    assert R.decode(files[1]).pcm[0, :5].tolist() == [0, 0, 0, 4096, 0]
    assert R.decode(files[0]).md5_ok is None                                    # md5=False: the all-zero "unknown" signature
    w[1, 5] = float("nan")
    w[1, 9] = float("inf")
    with pytest.raises(ValueError, match="item 1: a non-finite sample .*at sample 5"):
        encode_flac(w)
    q = torch.zeros(1, 2, 20, dtype=torch.int32, device=cuda)
    q[0, 1, 17] = 128
    with pytest.raises(ValueError, match="item 0: an integer sample outside the 8-bit range at sample 17"):
        encode_flac(q, bits_per_sample=8)


def _exact16(rows, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    q = np.stack([np.rint(9000 * np.sin(t * (0.02 + 0.01 * r)) + rng.normal(0, 40, n)) for r in range(rows)]).astype(np.int32)
    return q


def test_save_batch_then_load_batch(cuda, tmp_path):
    from voice100_amd.audio_io import load_batch, save_batch
    q = _exact16(5, 9000, 1)
    lens = [9000, 4097, 1, 5000, 8193]
    wave = torch.from_numpy(q.astype(np.float32) / 32768.0).to(cuda)
    paths = [tmp_path / name for name in ("a.flac", "b.wav", "c.flac", "d.flac", "e.wav")]
    save_batch(paths, wave, torch.tensor(lens, device=cuda), 16000)
    got, got_len = load_batch(paths, 16000)
    assert got_len.tolist() == lens and got.shape == (5, 9000)
    for b, n in enumerate(lens):
        assert torch.equal(got[b, :n], wave[b, :n]) and not got[b, n:].any(), b
    assert paths[0].read_bytes() == M.encode(q[0], 16000, 16).data              # the files are the encoder's, with the unknown MD5


def test_tts_pipeline_save(cuda, tmp_path):
    from voice100_amd.audio_io import _quantise, load_audio
    from voice100_amd.infer import TTSPipeline
    from voice100_amd.tts import AlignTextToAudioModel, TextToAlignTextModel
    from voice100_amd.vocoder import WORLDVocoder
    torch.manual_seed(4)
    al = TextToAlignTextModel(vocab_size=29, hidden_size=64).to(cuda).eval()
    with torch.no_grad():
        al.layers[4].bias.copy_(torch.tensor([0.6931, 1.3863], device=cuda))
    au = AlignTextToAudioModel(vocab_size=29, hidden_size=64, use_mcep=True).to(cuda).eval()
    with torch.no_grad():
        au.norm.f0_mean.fill_(150.0); au.norm.f0_std.fill_(30.0); au.norm.codeap_mean.fill_(-12.0); au.norm.codeap_std.fill_(3.0)
    v = WORLDVocoder(use_mcep=True).to(cuda)
    chain = TTSPipeline(al, au, v)
    out = chain(torch.randint(1, 29, (3, 12), device=cuda), torch.tensor([12, 7, 9], device=cuda))
    paths = [tmp_path / "a.flac", tmp_path / "b.wav", tmp_path / "c.flac"]
    chain.save(out, paths)
    for b, p in enumerate(paths):
        n = int(out["wave_len"][b])
        got, sr = load_audio(p)
        assert sr == v.sample_rate and got.shape == (1, n)
        assert torch.equal(got[0], _quantise(out["wave"][b, :n], 16).cpu().float() / 32768.0), b
    with pytest.raises(ValueError, match='no "wave"'):
        chain.save({k: t for k, t in out.items() if k != "wave"}, paths)


def test_cut_utterances(cuda, tmp_path):
    from voice100_amd.audio_io import load_audio
    from voice100_amd.infer import cut_utterances
    q = _exact16(1, 20000, 2)[0]
    wave = torch.from_numpy(q.astype(np.float32) / 32768.0).to(cuda)
    utts = [{"start_s": 0.0, "end_s": 0.25}, {"start_s": 0.25, "end_s": 0.78125}, {"start_s": 0.8125, "end_s": 1.25}]
    paths = [tmp_path / "u0.flac", tmp_path / "u1.wav", tmp_path / "u2.flac"]
    ranges = cut_utterances(wave, 16000, {"ok": True, "utterances": utts}, paths, pad_s=0.03125)
    assert ranges == [(0, 4500), (3500, 13000), (12500, 20000)]
    for (a, e), p in zip(ranges, paths):
        got, sr = load_audio(p)
        assert sr == 16000 and torch.equal(got[0], wave[a:e].cpu()), p
    assert paths[2].read_bytes() == M.encode(q[12500:20000], 16000, 16).data
    with pytest.raises(ValueError, match="alignment failed"):
        cut_utterances(wave, 16000, {"ok": False, "utterances": utts}, [tmp_path / "x.flac"] * 3)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["u0.flac", "u1.wav", "u2.flac"]
