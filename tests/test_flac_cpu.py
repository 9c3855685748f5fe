"""FLAC without a GPU: the test-side oracle (tests/_flac_ref.py) pinned by the three worked examples of the format's RFC (libFLAC 1.3.3
streams, kept as literals in tests/_flac_cases.py), the explicit encoder against the reference decoder over the whole list the GPU
test decodes, audio_io.flac_info on the examples and on every refusal, load_audio's dispatch, and load_flac's refusal to run without
a device.  The last test is self-activating: it decodes every *.flac under tests/golden/flac (or V100_FLAC_DIR) with verify_md5 and
skips while there is none -- parity with libFLAC-encoded files rests on the three examples and the format description until then."""
import glob
import os
import wave

import numpy as np
import pytest
import torch

import _flac_cases as K
import _flac_ref as R
from voice100_amd import audio_io as A

FLAC_DIR = os.environ.get("V100_FLAC_DIR", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flac"))


def _vector(name):
    return next(c for c in K.cases() if c.name == name)


def test_reference_decoder_on_the_rfc_examples():
    for name, hx, pcm, rate, bits in K.VECTORS:
        d = R.decode(bytes.fromhex(hx))
        assert d.pcm.tolist() == pcm and d.sample_rate == rate and d.bits_per_sample == bits, name
        assert d.md5_ok is True, name
    # every frame's CRC-8 and CRC-16 were checked on the way (decode_frame raises on a mismatch); a damaged byte is caught
    bad = bytearray.fromhex(K.VECTORS[2][1])
    bad[-6] ^= 1
    with pytest.raises(ValueError, match="CRC-16"):
        R.decode(bytes(bad))


def test_encoder_round_trips_through_the_reference_decoder():
    names = [c.name for c in K.cases()]
    assert len(set(names)) == len(names) > 40
    for c in K.cases():
        d = R.decode(c.data)
        assert np.array_equal(d.pcm, c.pcm) and d.pcm.dtype == np.int32, c.name
        assert d.sample_rate == c.rate and d.bits_per_sample == c.bits and d.md5_ok is True, c.name


def test_encoder_reproduces_the_first_rfc_example_byte_for_byte():
    # the explicit choices of that stream: one sample, 8-bit block-size form, verbatim subframes with 2 and 4 wasted bits
    fr = R.Frame(1, [R.Sub("verbatim", wasted=2), R.Sub("verbatim", wasted=4)], assign=1, bs_form=8, rate_form="code", size_form="code")
    frame = R.encode_frame(np.array([[25588], [10416]]), 0, 44100, 16, fr)
    assert frame == K.RFC_1_FRAME
    assert R.pcm_md5(np.array([[25588], [10416]]), 16) == bytes.fromhex(K.VECTORS[0][1])[26:42]


def test_flac_info_on_the_rfc_examples():
    i1, i2, i3 = (A.flac_info(bytes.fromhex(v[1])) for v in K.VECTORS)
    assert i1 == A.FlacInfo(44100, 2, 16, 1, 4096, 4096, bytes.fromhex("3e84b41807dc690307586a3dad1a2e0f"), 42)
    assert (i2.sample_rate, i2.channels, i2.bits_per_sample, i2.total_samples, i2.min_blocksize, i2.max_blocksize) == (44100, 2, 16, 19, 4096, 4096)
    assert i2.md5 == bytes.fromhex("d5b0564975e98b8d8b930422757b8103")
    assert i2.first_frame_offset == 4 + 38 + 22 + 62 + 10        # STREAMINFO, seek table, comment, padding: all skipped
    assert (i3.sample_rate, i3.channels, i3.bits_per_sample, i3.total_samples, i3.first_frame_offset) == (32000, 1, 8, 24, 42)


def test_flac_info_from_a_path(tmp_path):
    p = tmp_path / "a.flac"
    p.write_bytes(bytes.fromhex(K.VECTORS[2][1]))
    assert A.flac_info(p) == A.flac_info(bytes.fromhex(K.VECTORS[2][1]))
    assert A.flac_info(str(p)).total_samples == 24


def _with_streaminfo(**kw):
    f = dict(rate=16000, channels=1, bps=16, total=100, min_bs=16, max_bs=16)
    f.update(kw)
    return R.container(R.streaminfo(f["rate"], f["channels"], f["bps"], f["total"], f["min_bs"], f["max_bs"]), b"")


def test_flac_info_refusals(tmp_path):
    good = bytes.fromhex(K.VECTORS[1][1])
    p = tmp_path / "x.wav"
    with wave.open(str(p), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(8000)
        f.writeframes(b"\0\0" * 8)
    with pytest.raises(ValueError, match="not a FLAC file.*RIFF"):
        A.flac_info(p)
    with pytest.raises(ValueError, match="Ogg"):
        A.flac_info(b"OggS\0\2" + bytes(40))
    with pytest.raises(ValueError, match="ID3"):
        A.flac_info(b"ID3\4\0\0\0\0\0\x0a" + bytes(10) + good)
    with pytest.raises(ValueError, match="truncated FLAC metadata"):
        A.flac_info(good[:60])                                        # inside the seek table
    with pytest.raises(ValueError, match="truncated FLAC metadata"):
        A.flac_info(good[:42])                                        # after STREAMINFO, which was not the last block
    with pytest.raises(ValueError, match="not STREAMINFO"):
        A.flac_info(b"fLaC" + good[42:])
    with pytest.raises(ValueError, match="total_samples 0"):
        A.flac_info(_with_streaminfo(total=0))
    with pytest.raises(ValueError, match="32 bits per sample"):
        A.flac_info(_with_streaminfo(bps=32))
    with pytest.raises(ValueError, match="2\\^31"):
        A.flac_info(_with_streaminfo(total=2 ** 31))
    assert A.flac_info(_with_streaminfo(total=2 ** 31 - 1, channels=8)).channels == 8        # the field holds 1 to 8 channels: no ninth to refuse
    with pytest.raises(ValueError, match="block sizes"):
        A.flac_info(_with_streaminfo(min_bs=0))


def test_plan_layout_is_padded_and_bounded():
    datas = [c.data for c in K.cases()[:6]]
    infos = [A.flac_info(d) for d in datas]
    buf, table, S, H, stage, longest = A._flac_plan(datas, infos, [str(k) for k in range(6)])
    assert buf.size % 16 == 0 and table.shape == (6, 16) and table.dtype == np.int32
    for b, (d, fi) in enumerate(zip(datas, infos)):
        begin, end = int(table[b, 0]), int(table[b, 1])
        assert begin % 16 == 0 and bytes(buf[begin:end]) == d[fi.first_frame_offset:]
        nxt = int(table[b + 1, 0]) if b + 1 < 6 else buf.size
        assert nxt - end >= 16 and not buf[end:nxt].any()             # a wide read past a file's end meets zeros, inside the buffer
        assert table[b, 9] >= -(-fi.total_samples // fi.min_blocksize) and table[b, 11] >= 2 * table[b, 9]
        assert table[b, 11] & (table[b, 11] - 1) == 0
    assert S == int(table[:, 9].sum()) and H == int(table[:, 11].sum()) and longest == max(int(t[1] - t[0]) for t in table)
    with pytest.raises(ValueError, match="workspace"):
        big = A.FlacInfo(16000, 8, 16, 2 ** 31 - 1, 16, 65535, bytes(16), 42)
        A._flac_plan([datas[0]], [big], ["big"])


def test_load_audio_dispatch(tmp_path):
    p = tmp_path / "noise.bin"
    p.write_bytes(b"OggS" + bytes(64))
    with pytest.raises(ValueError, match="neither WAV nor FLAC.*OggS"):
        A.load_audio(p)
    w = tmp_path / "a.wav"
    with wave.open(str(w), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(8000)
        f.writeframes(np.arange(8, dtype="<i2").tobytes())
    got, sr = A.load_audio(w)
    want, _ = A.load_wav(w)
    assert sr == 8000 and torch.equal(got, want)
    fl = tmp_path / "a.flac"
    fl.write_bytes(bytes.fromhex(K.VECTORS[0][1]))
    with pytest.raises(ValueError, match="not a RIFF/WAVE"):          # load_wav itself is unchanged
        A.load_wav(fl)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU only"):          # fLaC dispatches to load_flac, which needs the device
            A.load_audio(fl)


def test_load_flac_without_a_gpu_is_a_runtime_error(tmp_path):
    fl = tmp_path / "a.flac"
    fl.write_bytes(bytes.fromhex(K.VECTORS[0][1]))
    with pytest.raises(ValueError, match="not a FLAC file"):          # the container is checked first, on the host
        A.decode_flac([b"RIFFxxxxWAVE"])
    if torch.cuda.is_available():                                      # with a device the same call is the decoder (tests/test_gpu_flac.py)
        w, sr = A.load_flac(fl)
        assert sr == 44100 and w.shape == (2, 1)
        return
    with pytest.raises(RuntimeError, match="GPU only"):
        A.load_flac(fl)
    with pytest.raises(RuntimeError, match="GPU only"):
        A.decode_flac([fl])


def test_flac_files_in_the_tree_decode_to_their_md5():
    """Any .flac with a non-zero STREAMINFO MD5 is its own test vector."""
    files = sorted(glob.glob(os.path.join(FLAC_DIR, "**", "*.flac"), recursive=True))
    if not files:
        pytest.skip(f"no *.flac under {FLAC_DIR}: no file from another encoder exists in this tree -- put libFLAC-encoded files (LibriSpeech's) "
                    "there or point V100_FLAC_DIR at them (parity with libFLAC stays on the three RFC examples until then)")
    for path in files:
        data = open(path, "rb").read()
        assert R.decode(data).md5_ok is not False, path                # the oracle agrees with the file's own checksum
    if not torch.cuda.is_available():
        pytest.skip("the device decoder needs a GPU; the reference decoder verified the files' MD5s")
    for k in range(0, len(files), 32):
        A.decode_flac(files[k:k + 32], verify_md5=True)
