"""infer.LongASRPipeline (K31) on the GPU.  On planted logits: the segment table is the numpy mirror's, every segment's ids, length and
score are what ctc_beam_search (or the greedy decode and ctc_segment) gives on that slice alone, to the bit -- batching and padding
must not show --, the timed fields are ctc_segment's on the slice moved by seg_start, and max_batch changes nothing.  End to end: a
small untrained AudioToTextCTC on random features, max_frames 512 (forced cuts), against the public parts called by hand, and
through transcribe on a WAV file written with save_wav."""
import math

import numpy as np
import pytest
import torch

import _cut_points_ref as R
from voice100_amd.asr import AudioToTextCTC
from voice100_amd.decode import CTCSegments, ctc_beam_search, ctc_cut_points, ctc_greedy_decode, ctc_segment
from voice100_amd.infer import LongASRPipeline, long_transcript_records, windowed_logits
from voice100_amd.lm import NGramLM

pytestmark = pytest.mark.gpu

ALPHABET = "_ abcdefghijklmnopqrstuvwxyz'"
decode = lambda ids: "".join(ALPHABET[int(i)] for i in ids)  # noqa: E731
CUT = dict(max_frames=3000, min_gap=25, margin=0.0, pad=5, min_frames=50)
FRAME_FIELDS = ("start", "end", "word_start", "word_end")


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.fixture(scope="module")
def planted(cuda):
    """About 3000 frames, 6-10 utterances of 200-400 frames with pauses of 30-80, at 8 nats over unit noise."""
    x, lab = R.planted(31, 3000, speech=(200, 400), amp=8.0)
    table = R.mirror(x[None], None, **CUT)
    assert 6 <= int(table[3][0]) <= 10 and not table[2].any()
    texts = []
    for s, e in zip(table[0][0], table[1][0]):
        seq = lab[s:e]
        seq = seq[np.concatenate([[True], seq[1:] != seq[:-1]])]
        texts.append([int(v) for v in seq if v != 0])
    lm = NGramLM.fit(texts, 29, 3).compile().to(cuda)
    return torch.from_numpy(x).to(cuda), table, lm


def configs(lm):
    return {"greedy": {}, "beam4": dict(beam_size=4), "beam16": dict(beam_size=16),
            "beam16lm": dict(beam_size=16, lm=lm, lm_weight=0.7, length_bonus=0.3)}


@pytest.mark.parametrize("name", ["greedy", "beam4", "beam16", "beam16lm"])
def test_segments_equal_the_parts_on_each_slice(cuda, planted, name):
    x, table, lm = planted
    kw = configs(lm)[name]
    pipe = LongASRPipeline(None, frame_seconds=0.02, **kw, **CUT)
    out = pipe.segments(logits=x)
    S = int(table[3][0])
    for k, ref in zip(("seg_start", "seg_end", "forced"), table[:3]):
        assert out[k].dtype == torch.int32 and np.array_equal(out[k].cpu().numpy(), ref[0]), k
    assert out["ids"].shape[0] == S and out["ids"].dtype == torch.int64 and out["frame_seconds"] == 0.02
    L = out["ids"].shape[1]
    assert L == max(int(out["ids_len"].max()), 1)
    for i in range(S):
        s, e = int(table[0][0, i]), int(table[1][0, i])
        piece = x[s:e].clone()[None]
        if name == "greedy":
            ids, n = ctc_greedy_decode(piece)
            ids, n = ids[0], n[0]
        else:
            ids, n, score = ctc_beam_search(piece, None, kw["beam_size"], 1, lm=kw.get("lm"), lm_weight=kw.get("lm_weight", 0.5),
                                            length_bonus=kw.get("length_bonus", 0.0))[:3]
            ids, n, score = ids[0, 0], n[0, 0], score[0, 0]
        n_i = int(n)
        assert int(out["ids_len"][i]) == n_i and n_i > 0
        assert torch.equal(out["ids"][i, :n_i], ids[:n_i]) and not out["ids"][i, n_i:].any()
        seg = ctc_segment(piece, None, ids[None, :n_i].contiguous(), n.reshape(1))
        if name == "greedy":
            score = seg.log_prob[0]
        assert torch.equal(bits(out["score"][i:i + 1]), bits(score.reshape(1))), (name, i)
        nw = int(seg.n_words[0])
        assert int(out["n_words"][i]) == nw
        for k in CTCSegments._fields:
            want = getattr(seg, k)
            if want.dim() == 1:
                assert torch.equal(bits(out[k][i:i + 1]), bits(want)), k
                continue
            width = nw if k.startswith("word_") else n_i
            want = want[0, :width] + (s if k in FRAME_FIELDS else 0)
            assert torch.equal(bits(out[k][i, :width]), bits(want)), (name, i, k)
            assert not out[k][i, width:].any(), (name, i, k)
    assert bool((out["start"][:, 0] >= out["seg_start"]).all()) and bool((out["end"].amax(1) <= out["seg_end"]).all())


@pytest.mark.parametrize("name", ["greedy", "beam16lm"])
def test_result_does_not_depend_on_max_batch(cuda, planted, name):
    x, table, lm = planted
    kw = configs(lm)[name]
    want = LongASRPipeline(None, frame_seconds=0.02, max_batch=32, **kw, **CUT).segments(logits=x)
    for max_batch in (1, 3):
        got = LongASRPipeline(None, frame_seconds=0.02, max_batch=max_batch, **kw, **CUT).segments(logits=x)
        assert got.keys() == want.keys()
        for k, v in want.items():
            if isinstance(v, torch.Tensor):
                assert got[k].shape == v.shape and torch.equal(bits(got[k]), bits(v)), (max_batch, k)
    untimed = LongASRPipeline(None, frame_seconds=0.02, **kw, **CUT).segments(logits=x, timed=False)
    for k in ("seg_start", "ids", "ids_len", "score"):
        assert torch.equal(bits(untimed[k]), bits(want[k])), k
    assert ("start" in untimed) == (name == "greedy")


def test_rows_without_speech_and_refusals(cuda, planted):
    x, _, _ = planted
    quiet = torch.zeros(500, 29, device=cuda)
    quiet[:, 0] = 5.0
    out = LongASRPipeline(None, frame_seconds=0.02).segments(logits=quiet)
    assert out["seg_start"].shape == (0,) and out["ids"].shape == (0, 1) and out["score"].shape == (0,) and out["start"].shape == (0, 1)
    assert LongASRPipeline(None).segments(logits=quiet)["frame_seconds"] is None
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        LongASRPipeline(None).segments(logits=x.cpu())
    with pytest.raises(RuntimeError, match="no mel"):
        LongASRPipeline(None).segments("a.wav")
    with pytest.raises(RuntimeError, match="blank"):
        LongASRPipeline(None, blank=1)


@pytest.fixture(scope="module")
def model(cuda):
    torch.manual_seed(5)
    return AudioToTextCTC(64, 32, 29, 32).to(cuda).eval()


def test_end_to_end_equals_the_parts_called_by_hand(cuda, model):
    gen = torch.Generator().manual_seed(8)
    feats = (torch.randn(6001, 64, generator=gen) * 2 - 4).to(cuda)
    pipe = LongASRPipeline(model, frame_seconds=0.02, keep=700, max_frames=512, max_batch=4)
    out = pipe.segments(feats=feats)
    logits = windowed_logits(model, feats, 700)
    assert logits.shape[0] == 3001
    cp = ctc_cut_points(logits[None], None, max_frames=512)
    S = int(cp.n_seg[0])
    assert S >= 6 and int(cp.forced.sum()) >= 1                   # nothing taught this model to pause: the cuts are forced
    for k, v in (("seg_start", cp.start), ("seg_end", cp.end), ("forced", cp.forced)):
        assert torch.equal(out[k], v[0]), k
    assert int((cp.end - cp.start).max()) <= 512
    for i in range(S):
        s, e = int(cp.start[0, i]), int(cp.end[0, i])
        piece = logits[s:e].clone()[None]
        ids, n = ctc_greedy_decode(piece)
        n_i = int(n[0])
        assert int(out["ids_len"][i]) == n_i and torch.equal(out["ids"][i, :n_i], ids[0, :n_i])
        seg = ctc_segment(piece, None, ids[:, :max(n_i, 1)].contiguous(), n)
        assert torch.equal(bits(out["score"][i:i + 1]), bits(seg.log_prob))
        assert torch.equal(out["end"][i, :n_i], seg.end[0, :n_i] + s)


def test_transcribe_a_wav_file(cuda, model, tmp_path):
    from voice100_amd.audio_io import load_batch, save_wav
    from voice100_amd.mel import MelSpectrogramAudioTransform
    gen = torch.Generator().manual_seed(9)
    seconds = 20.0005
    wave = torch.randn(round(16000 * seconds), generator=gen) * 0.1
    path = str(tmp_path / "chapter.wav")
    save_wav(path, wave.clamp(-0.99, 0.99), 16000)
    mel = MelSpectrogramAudioTransform().to(cuda)
    pipe = LongASRPipeline(model, mel, keep=400, max_frames=256, min_frames=20)
    res = pipe.transcribe(path, decode)
    loaded = load_batch([path], 16000, cuda)[0][0]
    out = pipe.segments(loaded)
    assert out["frame_seconds"] == res["frame_seconds"] == 160 / 16000 * 2
    fs, duration = res["frame_seconds"], loaded.shape[0] / 16000
    S = out["seg_start"].shape[0]
    assert len(res["utterances"]) == S >= 3
    rows = []
    for i, u in enumerate(res["utterances"]):
        n = int(out["ids_len"][i])
        rows.append(out["ids"][i, :n].tolist())
        assert u["text"] == decode(rows[-1]) and u["score"] == float(out["score"][i]) and u["forced"] == bool(out["forced"][i])
        assert u["start_s"] == int(out["seg_start"][i]) * fs and u["end_s"] == min(int(out["seg_end"][i]) * fs, duration)
        assert 0 <= u["start_s"] < u["end_s"] <= duration
        assert [w["word"] for w in u["words"]] == u["text"].split() and len(u["words"]) == int(out["n_words"][i])
        for w, word in enumerate(u["words"]):
            assert word["start"] == int(out["word_start"][i, w]) * fs
            assert word["end"] == min(int(out["word_end"][i, w]) * fs, duration)
            assert word["confidence"] == pytest.approx(math.exp(float(out["word_log_confidence"][i, w])), rel=1e-6)
            assert u["start_s"] <= word["start"] < word["end"] <= u["end_s"]
    joined = []
    for r in rows:
        if r and joined and joined[-1] != 1 and r[0] != 1:
            joined.append(1)
        joined.extend(r)
    assert res["text"] == decode(joined)
    lines = long_transcript_records(res)
    assert len(lines) == S and lines[0] == f"{res['utterances'][0]['start_s']:.3f}|{res['utterances'][0]['end_s']:.3f}|" \
                                           f"{res['utterances'][0]['score']:.4f}|{res['utterances'][0]['text']}"
