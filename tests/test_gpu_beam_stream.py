"""The resumable beam search (K32): decode.CTCBeamStream, decode.ctc_beam_search_long and LongASRPipeline.whole.

The backbone is equality of BITS: a chunked run keeps the beam, the two fp64 offsets and the trie between launches, so it does the
one call's floating-point operations in the one call's order, and every returned tensor must be torch.equal to ctc_beam_search's on
the same frames, whatever the chunk size.  ctc_beam_search itself is held to the float64 oracles by tests/test_gpu_beam.py and
tests/test_gpu_beam_lm.py; past its 4096 frames the planted cases of tests/_beam_stream_cases.py are held to those oracles here."""
import numpy as np
import pytest
import torch

import _beam_lm_ref as lm_ref
import _beam_ref as ref
from _beam_stream_cases import CHUNK_SHAPES, LM_CASE, LONG, chunks_of, long_leaves, planted, shape_logits
from test_gpu_beam_lm import bits, device_lm
from voice100_amd import _native as N
from voice100_amd.decode import CTCBeamStream, ctc_beam_search, ctc_beam_search_long
from voice100_amd.infer import LongASRPipeline

pytestmark = pytest.mark.gpu

LM_SETTINGS = [(0.5, 0.0), (1.0, 1.0), (0.3, -0.5)]    # (lm_weight, length_bonus)


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, c) in enumerate(zip(got, want)):
        assert a.shape == c.shape and a.dtype == c.dtype and torch.equal(bits(a), bits(c)), f"{what}: output {i} differs"


def lm_of(dev, kind, V):
    if kind == "automaton":
        return device_lm(dev, lm_ref.random_automaton(11, V, 31 + V) + (0,))
    return device_lm(dev, lm_ref.fit_lm(V)[0])


@pytest.mark.parametrize("shape", CHUNK_SHAPES, ids=["T%d-V%d-W%d" % s for s in CHUNK_SHAPES])
def test_chunked_equals_one_call(cuda, shape):
    T, V, W = shape
    x, lengths = shape_logits(T, V, W)
    xt, lt = torch.from_numpy(x).to(cuda), torch.tensor(lengths, dtype=torch.int32, device=cuda)
    nbest = min(W, 4)
    for lens in (lt, None):
        want = ctc_beam_search(xt, lens, W, nbest)
        for chunk in chunks_of(T):
            same(ctc_beam_search_long(xt, lens, W, nbest, chunk=chunk), want, f"{shape} chunk {chunk} lengths {lens is not None}")


@pytest.mark.parametrize("kind", ["automaton", "fit"])
@pytest.mark.parametrize("shape", CHUNK_SHAPES, ids=["T%d-V%d-W%d" % s for s in CHUNK_SHAPES])
def test_chunked_equals_one_call_with_an_lm(cuda, shape, kind):
    T, V, W = shape
    x, lengths = shape_logits(T, V, W)
    xt, lt = torch.from_numpy(x).to(cuda), torch.tensor(lengths, dtype=torch.int32, device=cuda)
    lm, nbest = lm_of(cuda, kind, V), min(W, 4)
    for use_eos in (True, False):
        for alpha, beta in LM_SETTINGS:
            kw = dict(lm=lm, lm_weight=alpha, length_bonus=beta, use_eos=use_eos)
            want = ctc_beam_search(xt, lt, W, nbest, **kw)
            assert len(want) == 5
            for chunk in chunks_of(T):
                same(ctc_beam_search_long(xt, lt, W, nbest, chunk=chunk, **kw), want, f"{shape} {kind} {kw} chunk {chunk}")


@pytest.mark.parametrize("with_lm", [False, True], ids=["plain", "lm"])
def test_hand_driven_stream(cuda, with_lm):
    """Pushes of 3, 1, 20, ... frames with ragged lengths per push, rows of length 0 among them: after every push the n best equal
    ctc_beam_search on the frames each row has run so far."""
    B, V, W = 6, 29, 8
    pushes = [3, 1, 20, 7, 2, 31]
    rng = np.random.default_rng(32)
    kw = dict(lm=lm_of(cuda, "fit", V), lm_weight=0.5, length_bonus=0.3) if with_lm else {}
    stream = CTCBeamStream(B, V, W, max_frames=sum(pushes), device=cuda, **kw)
    first = stream.hypotheses(W)                         # before the first push: the empty hypothesis alone, ids of width 0
    assert first[0].shape == (B, W, 0) and not bool(first[1].any()) and len(first) == (5 if with_lm else 3)
    assert bool((first[2][:, 0] == 0).all()) and bool((first[2][:, 1:] == -float("inf")).all())
    rows = [np.zeros((0, V), np.float32) for _ in range(B)]          # the frames each row has run
    for j, T in enumerate(pushes):
        x = (rng.standard_normal((B, T, V)) * 3).astype(np.float32)
        lens = rng.integers(0, T + 1, B)
        lens[j % B] = 0                                  # a row without frames in this push ...
        lens[(j + 1) % B] = T                            # ... and one with all of them
        if j == 2:
            lens = None                                  # every row, all frames
        before = N.launch_count()
        stream.push(torch.from_numpy(x).to(cuda), None if lens is None else torch.tensor(lens, dtype=torch.int32, device=cuda))
        assert N.launch_count() - before == 1
        for b in range(B):
            rows[b] = np.concatenate([rows[b], x[b, :T if lens is None else lens[b]]])
        width = max(len(r) for r in rows)
        so_far = np.zeros((B, width, V), np.float32)
        for b in range(B):
            so_far[b, :len(rows[b])] = rows[b]
        st, sl = torch.from_numpy(so_far).to(cuda), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=cuda)
        for final in ((False, True) if with_lm else (False,)):
            want = ctc_beam_search(st, sl, W, W, use_eos=final, **kw)
            got = stream.hypotheses(W, final=final)
            again = stream.hypotheses(W, final=final)                        # reading does not disturb the state
            same(again, got, f"push {j}: two reads")
            assert got[0].shape == (B, W, stream.frames) and not bool(got[0][:, :, width:].any())
            same((got[0][:, :, :width],) + tuple(got[1:]), want, f"after push {j} final {final}")
    assert stream.frames == sum(pushes)
    got = stream.finish(W)
    same((got[0][:, :, :width],) + tuple(got[1:]), ctc_beam_search(st, sl, W, W, **kw), "finish")
    for closed in (lambda: stream.push(torch.zeros((B, 1, V), device=cuda)), lambda: stream.hypotheses(1)):
        with pytest.raises(RuntimeError, match="finished"):
            closed()


def test_past_4096_frames(cuda):
    T, V, W = LONG["T"], LONG["V"], LONG["W"]
    x = planted(T, V, LONG["seed"], LONG["peak"])
    xt = torch.from_numpy(np.stack([x, x])).to(cuda)
    lt = torch.tensor(LONG["lengths"], dtype=torch.int32, device=cuda)
    want = ctc_beam_search_long(xt, lt, W, W, chunk=4096)
    assert want[0].shape == (2, W, T)
    for chunk in (1000, 333):
        same(ctc_beam_search_long(xt, lt, W, W, chunk=chunk), want, f"chunk {chunk}")
    ids, lens, scores = (o.cpu().numpy() for o in want)
    for b, leaves in enumerate(long_leaves()):
        assert leaves is not None                        # the oracle decides both rows: nothing is skipped
        hyps = [tuple(int(v) for v in ids[b, r, :lens[b, r]]) for r in range(W)]
        ok, err = ref.accept(leaves, hyps, [float(s) for s in scores[b]])
        print(f"row {b}: {LONG['lengths'][b]} frames, score {scores[b, 0]:.4f}, {lens[b, 0]} labels, score_rel_err {err:.3e}")
        assert ok, (b, err, hyps[0], float(scores[b, 0]), leaves[0][0])
    lm = lm_of(cuda, "fit", V)                           # with the LM past 4096 frames: chunk invariance only (see _beam_stream_cases)
    kw = dict(lm=lm, lm_weight=0.5, length_bonus=0.3)
    want = ctc_beam_search_long(xt, lt, W, W, chunk=4096, **kw)
    assert bool(torch.isfinite(want[2][:, 0]).all())
    for chunk in (1000, 333):
        same(ctc_beam_search_long(xt, lt, W, W, chunk=chunk, **kw), want, f"lm chunk {chunk}")


def test_lm_stream_against_the_fused_oracle(cuda):
    c = LM_CASE
    x = planted(c["T"], c["V"], c["seed"], c["peak"])
    fit, look = lm_ref.fit_lm(c["V"])
    leaves = lm_ref.beam_search_fork(x, c["W"], look, c["alpha"], c["beta"])
    assert leaves is not None and len(leaves) == 1
    xt = torch.from_numpy(x[None]).to(cuda)
    kw = dict(lm=device_lm(cuda, fit), lm_weight=c["alpha"], length_bonus=c["beta"])
    out = ctc_beam_search_long(xt, None, c["W"], c["W"], chunk=c["chunk"], **kw)
    same(out, ctc_beam_search(xt, None, c["W"], c["W"], **kw), "one call")
    ids, lens, scores, ctc, lms = (o.cpu().numpy() for o in out)
    hyps = [tuple(int(v) for v in ids[0, r, :lens[0, r]]) for r in range(c["W"])]
    ok, err = lm_ref.accept(leaves, hyps, *([float(s) for s in a[0]] for a in (scores, ctc, lms)))
    print(f"score {scores[0, 0]:.4f}, {lens[0, 0]} labels, score_rel_err {err:.3e}")
    assert ok, (err, hyps[0], float(scores[0, 0]), leaves[0][0])


@pytest.mark.parametrize("with_lm", [False, True], ids=["plain", "lm"])
def test_a_row_of_nans_and_a_row_of_length_0(cuda, with_lm):
    T, V, W = 33, 29, 8
    x = (np.random.default_rng(5).standard_normal((4, T, V)) * 3).astype(np.float32)
    x[1] = np.nan
    xt, lt = torch.from_numpy(x).to(cuda), torch.tensor([T, T, 0, 20], dtype=torch.int32, device=cuda)
    kw = dict(lm=lm_of(cuda, "fit", V), lm_weight=0.5, length_bonus=0.3) if with_lm else {}
    want = ctc_beam_search(xt, lt, W, 4, **kw)
    for chunk in (1, 7, 20, T):
        same(ctc_beam_search_long(xt, lt, W, 4, chunk=chunk, **kw), want, f"chunk {chunk}")
    ctc = want[3] if with_lm else want[2]
    assert want[1][2].tolist() == [0] * 4 and float(ctc[2, 0]) == 0.0       # no frame: the empty hypothesis


def test_capacity(cuda):
    V, W = 8, 4
    stream = CTCBeamStream(1, V, W, max_frames=10, device=cuda)
    x = torch.randn((1, 6, V), device=cuda)
    stream.push(x)
    before = N.launch_count()
    with pytest.raises(RuntimeError, match="max_frames"):
        stream.push(x[:, :5])                            # 6 + 5 > 10: refused on the host
    with pytest.raises(RuntimeError):
        stream.push(x[:, :0])
    with pytest.raises(RuntimeError):
        stream.push(torch.zeros((1, 4097, V), device=cuda))
    with pytest.raises(RuntimeError):
        stream.push(x.cpu())
    with pytest.raises(RuntimeError):
        stream.hypotheses(W + 1)
    assert N.launch_count() == before and stream.frames == 6
    stream.push(x[:, :4])                                # exactly full
    same(stream.finish(W), ctc_beam_search(torch.cat([x, x[:, :4]], 1), None, W, W), "a full stream")
    for W, F in ((64, 1 << 19), (16, 1 << 21), (1, 1 << 25)):
        with pytest.raises(RuntimeError, match="2\\^25"):
            CTCBeamStream(1, V, W, max_frames=F, device=cuda)
        with pytest.raises(RuntimeError):
            ctc_beam_search_long(torch.zeros((1, 1, V), device=cuda).expand(1, F, V), beam_size=W)
    for kw in ({"beam_size": 65}, {"beam_size": 0}, {"beam_size": 4, "nbest": 5}, {"nbest": 0}, {"blank": 8}, {"chunk": 0}, {"chunk": 4097}):
        with pytest.raises(RuntimeError):
            ctc_beam_search_long(x, **kw)
    assert N.launch_count() == before + 3                # the push, the read and the one call: no refusal launched anything


@pytest.mark.parametrize("with_lm", [False, True], ids=["plain", "lm"])
def test_pipeline_whole(cuda, with_lm):
    c = LM_CASE
    x = torch.from_numpy(planted(c["T"], c["V"], c["seed"], c["peak"])).to(cuda)
    kw = dict(lm=lm_of(cuda, "fit", c["V"]), lm_weight=0.5, length_bonus=0.3) if with_lm else {}
    pipe = LongASRPipeline(None, beam_size=4, frame_seconds=0.02, **kw)
    out = pipe.whole(logits=x, chunk=256)
    want = ctc_beam_search_long(x[None], None, 4, 1, **kw)
    n = int(want[1][0, 0])
    assert n > 50 and int(out["ids_len"]) == n and out["ids"].shape == (n,) and torch.equal(out["ids"], want[0][0, 0, :n])
    assert torch.equal(bits(out["score"]), bits(want[2][0, 0])) and out["frame_seconds"] == 0.02
    assert ("ctc_score" in out and "lm_score" in out) == with_lm
    if with_lm:
        assert torch.equal(bits(out["ctc_score"]), bits(want[3][0, 0])) and torch.equal(bits(out["lm_score"]), bits(want[4][0, 0]))
    assert pipe.band >= 2 * n + 1 and int(out["ok"]) == 1                    # the exact Viterbi
    start, end = out["start"].cpu(), out["end"].cpu()
    assert start.dtype == torch.int32 and start.shape == (n,) and end.shape == (n,)
    assert bool((start < end).all()) and bool((end[:-1] <= start[1:]).all()) and int(start[0]) >= 0 and int(end[-1]) <= c["T"]
    assert "start" not in pipe.whole(logits=x, timed=False)
    with pytest.raises(RuntimeError, match="greedily"):
        LongASRPipeline(None, frame_seconds=0.02).whole(logits=x)


def test_transcribe_whole_a_wav_file(cuda, tmp_path):
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.audio_io import load_batch, save_wav
    from voice100_amd.mel import MelSpectrogramAudioTransform
    alphabet = "_ abcdefghijklmnopqrstuvwxyz'"
    decode = lambda ids: "".join(alphabet[int(i)] for i in ids)  # noqa: E731
    torch.manual_seed(3)
    model = AudioToTextCTC(64, 32, 29, 32).to(cuda).eval()
    wave = torch.randn(round(16000 * 10.0005), generator=torch.Generator().manual_seed(9)) * 0.1
    path = str(tmp_path / "chapter.wav")
    save_wav(path, wave.clamp(-0.99, 0.99), 16000)
    pipe = LongASRPipeline(model, MelSpectrogramAudioTransform().to(cuda), beam_size=4, keep=200)
    res = pipe.transcribe_whole(path, decode)
    loaded = load_batch([path], 16000, cuda)[0][0]
    out = pipe.whole(loaded, chunk=100)                  # the chunking changes nothing
    fs, duration, n = res["frame_seconds"], loaded.shape[0] / 16000, int(out["ids_len"])
    assert fs == out["frame_seconds"] == 160 / 16000 * 2 and int(out["ok"]) == 1
    ids, start, end = out["ids"][:n].tolist(), out["start"][:n].tolist(), out["end"][:n].tolist()
    assert res["text"] == decode(ids) and res["score"] == float(out["score"]) and set(res) == {"text", "words", "score", "frame_seconds"}
    assert [w["word"] for w in res["words"]] == res["text"].split()
    at = 0
    for w in res["words"]:                               # a word is a maximal run of labels other than the separator (id 1)
        while ids[at] == 1:
            at += 1
        last = at + len(w["word"]) - 1
        assert w["start"] == start[at] * fs and w["end"] == min(end[last] * fs, duration) and set(w) == {"word", "start", "end"}
        assert 0 <= w["start"] < w["end"] <= duration
        at = last + 1
    with pytest.raises(RuntimeError, match="separator"):
        LongASRPipeline(model, pipe.mel, beam_size=4, sep=None).transcribe_whole(path, decode)
