"""decode.rescore_nbest (K34, csrc/rescore.hip) and the pipelines' second pass against the float64 oracle of tests/_rescore_ref.py.

Per case of the list: n_words, n_oov and order equal the oracle's (tests/test_rescore_cpu.py shows for the oracle alone that its keys are
far enough apart, or exact ties, for that comparison to be exact), the re-ordered ids, lens and first_scores are the gather by order, the
two score tensors lie within the bound derived in _rescore_ref, two calls give equal bits, and a poisoned workspace changes nothing."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _cut_points_ref as C
import _rescore_ref as R
from conftest import load_golden, sub
from voice100_amd import _native as N
from voice100_amd.asr import AudioToTextCTC
from voice100_amd.decode import Rescored, _rescore_launch, ctc_beam_search, ctc_beam_search_long, rescore_nbest
from voice100_amd.infer import ASRPipeline, LongASRPipeline
from voice100_amd.lm import NGramLM, WordNGramLM

pytestmark = pytest.mark.gpu

CASES = R.case_list()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and torch.equal(bits(x), bits(y))) for x, y in zip(a, b))


_ON_DEVICE = {}


def on(dev, lm):
    """The compiled model's tables on the device, once per model; the host copy stays what the CPU tests see."""
    if id(lm) not in _ON_DEVICE:
        twin = WordNGramLM(lm.order, lm.ngrams, lm.sep, lm.blank, lm.symbols, lm.unk_logp)
        twin.pool, twin.pool_len, twin.word_table, twin.ngram_table, twin.meta = lm.pool, lm.pool_len, lm.word_table, lm.ngram_table, lm.meta
        _ON_DEVICE[id(lm)] = (twin.to(dev), lm)
    return _ON_DEVICE[id(lm)][0]


def compare(name, out, ref, ids, lens, scores):
    B, nbest, T = ids.shape
    assert isinstance(out, Rescored) and out._fields == ("ids", "lens", "scores", "first_scores", "word_lm_scores", "n_words", "n_oov", "order")
    assert out.ids.dtype == torch.int64 and out.ids.shape == (B, nbest, T)
    for k in ("lens", "n_words", "n_oov", "order"):
        assert getattr(out, k).dtype == torch.int32 and getattr(out, k).shape == (B, nbest), k
    for k in ("scores", "first_scores", "word_lm_scores"):
        assert getattr(out, k).dtype == torch.float32 and getattr(out, k).shape == (B, nbest), k
    got = {k: getattr(out, k).cpu().numpy() for k in out._fields}
    for k in ("order", "n_words", "n_oov"):
        assert np.array_equal(got[k], ref[k]), (name, k, got[k], ref[k])
    rows, order = np.arange(B)[:, None], got["order"].astype(np.int64)
    assert np.array_equal(got["ids"], ids[rows, order]) and np.array_equal(got["lens"], lens[rows, order]), name
    assert np.array_equal(got["first_scores"].view(np.int32), scores[rows, order].view(np.int32)), name
    worst = {}
    for k, b in (("scores", "bound_score"), ("word_lm_scores", "bound_lm")):
        absent = np.isinf(ref[k])
        assert np.array_equal(got[k][absent], ref[k][absent].astype(np.float32)), (name, k)
        err = np.abs(got[k][~absent].astype(np.float64) - ref[k][~absent])
        worst[k] = float(np.max(err / np.maximum(ref[b][~absent], 1e-300), initial=0.0))
        print(f"{name}: {k} at most {worst[k]:.3f} of the bound")
        assert np.all(err <= ref[b][~absent]), (name, k, worst[k])
    absent = ~(scores[rows, order] > -math.inf)
    assert not got["word_lm_scores"][absent].any() and not got["n_words"][absent].any() and not got["n_oov"][absent].any()
    return worst


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_case_against_the_oracle(cuda, case):
    name, lm, ids, lens, scores, kw = CASES[case]
    ref = R.oracle(lm, ids, lens, scores, **kw)
    dlm = on(cuda, lm)
    args = tuple(torch.from_numpy(a).to(cuda) for a in (ids, lens, scores))
    before = N.launch_count()
    out = rescore_nbest(*args, dlm, **kw)
    assert N.launch_count() - before == 1                # one launch; the inputs are left as they were
    assert all(np.array_equal(a.cpu().numpy().view(np.int32), h.view(np.int32)) for a, h in zip(args, (ids, lens, scores)))
    compare(name, out, ref, ids, lens, scores)
    assert same(out, rescore_nbest(*args, dlm, **kw))    # two calls: equal bits
    B, nbest, T = ids.shape
    nbytes = N.helper("v100_nbest_rescore_workspace_bytes", B, nbest, T)
    PAD = 256
    for poison in (0xFF, 0x7F, 0x00):                    # a poisoned workspace inside canaries: the same bits, the canaries untouched
        ws = torch.full((nbytes + 2 * PAD,), poison, dtype=torch.uint8, device=cuda)
        again = _rescore_launch(*args, dlm, kw.get("lm_weight", 0.5), kw.get("word_bonus", 0.0), kw.get("sep", 1), kw.get("use_eos", True),
                                ws=ws[PAD:PAD + nbytes])
        assert same(out, again), (name, poison)
        assert bool((ws[:PAD] == poison).all()) and bool((ws[PAD + nbytes:] == poison).all())


def test_planted_flip(cuda):
    """two hypotheses that differ in one word, the wrong one slightly ahead in the first pass, only the right word in the model"""
    lm, (ids, lens, scores) = R.flip_case()
    dlm = on(cuda, lm)
    args = tuple(torch.from_numpy(a).to(cuda) for a in (ids, lens, scores))
    out = rescore_nbest(*args, dlm)
    compare("flip", out, R.oracle(lm, ids, lens, scores), ids, lens, scores)
    assert out.order.tolist() == [[1, 0]] and out.n_oov.tolist() == [[0, 1]]
    assert out.ids[0, 0, :11].tolist() == R.spell("the cat sat")
    still = rescore_nbest(*args, dlm, lm_weight=0.0)
    compare("flip, weight 0", still, R.oracle(lm, ids, lens, scores, lm_weight=0.0), ids, lens, scores)
    assert still.order.tolist() == [[0, 1]] and torch.equal(bits(still.scores), bits(args[2]))


def test_largest_shape_and_refusals(cuda):
    """4096 labels (2048 words, the scratch's full width) on 64 hypotheses; then what the call refuses, by name, before any launch"""
    lm, lex = CASES[0][1], None
    dlm = on(cuda, lm)
    rng = np.random.default_rng(5)
    ids = rng.integers(2, 9, size=(1, 64, 4096)).astype(np.int64)
    ids[:, :, 1::2] = 1                                   # single-label words at every even position: 2048 words
    ids[0, 1, 1::4] = 6                                   # ... and rows of 1024 words of three labels
    lens = np.full((1, 64), 4096, dtype=np.int32)
    lens[0, 2:] = rng.integers(0, 4097, size=62)
    scores = R.first_scores(rng, 1, 64).astype(np.float32)
    keep = [0, 1, 2, 63]                                  # the oracle, in Python, on four of the rows
    ref = R.oracle(lm, ids[:, keep], lens[:, keep], scores[:, keep])
    out = rescore_nbest(*(torch.from_numpy(a).to(cuda) for a in (ids, lens, scores)), dlm)
    order = out.order[0].cpu().numpy()
    assert sorted(order.tolist()) == list(range(64))
    where = [int(np.nonzero(order == j)[0][0]) for j in keep]
    assert out.n_words[0, where[0]] == 2048 and out.n_words[0, where[1]] == 1024
    back = {j: r for r, j in zip(where, keep)}
    for r in range(4):
        j = keep[int(ref["order"][0, r])]
        assert int(out.n_words[0, back[j]]) == ref["n_words"][0, r] and int(out.n_oov[0, back[j]]) == ref["n_oov"][0, r]
        assert abs(float(out.word_lm_scores[0, back[j]]) - ref["word_lm_scores"][0, r]) <= ref["bound_lm"][0, r]
        assert abs(float(out.scores[0, back[j]]) - ref["scores"][0, r]) <= ref["bound_score"][0, r]
    s = out.scores[0]
    assert bool((s[:-1] >= s[1:]).all())

    small = tuple(torch.from_numpy(a).to(cuda) for a in CASES[0][2:5])
    before = N.launch_count()
    with pytest.raises(RuntimeError, match="nbest = 65 <= 64"):
        rescore_nbest(torch.zeros((1, 65, 4), dtype=torch.int64, device=cuda), torch.zeros((1, 65), dtype=torch.int32, device=cuda),
                      torch.zeros((1, 65), device=cuda), dlm)
    with pytest.raises(RuntimeError, match="T = 4097 <= 4096"):
        rescore_nbest(torch.zeros((1, 2, 4097), dtype=torch.int64, device=cuda), torch.zeros((1, 2), dtype=torch.int32, device=cuda),
                      torch.zeros((1, 2), device=cuda), dlm)
    with pytest.raises(RuntimeError, match="not compiled"):
        rescore_nbest(*small, WordNGramLM.from_arpa(R.ARPA_UNK, R.SYMBOLS))
    with pytest.raises(RuntimeError, match="word_lm.to"):
        rescore_nbest(*small, lm)
    with pytest.raises(RuntimeError, match="finite"):
        rescore_nbest(*small, dlm, lm_weight=math.inf)
    with pytest.raises(RuntimeError, match="as ctc_beam_search returns them"):
        rescore_nbest(small[0], small[1][:, :0], small[2], dlm)
    broken = WordNGramLM(lm.order, lm.ngrams, lm.sep)
    broken.pool, broken.pool_len, broken.word_table, broken.ngram_table = dlm.pool, dlm.pool_len, dlm.word_table, dlm.ngram_table
    broken.meta = lm.meta.copy()
    broken.meta[lm.order + 1] *= 8                        # a capacity that runs past the table
    with pytest.raises(RuntimeError, match="do not fit"):
        rescore_nbest(*small, broken)
    assert N.launch_count() == before
    lib = N.load()
    assert lib.v100_nbest_rescore_workspace_bytes(1, 65, 8) == -1 and lib.v100_nbest_rescore_workspace_bytes(1, 64, 4097) == -1
    assert lib.v100_nbest_rescore_workspace_bytes(3, 64, 4096) == 3 * 16 * 8 * 2048 and lib.v100_nbest_rescore_workspace_bytes(2, 5, 7) == 2 * 5 * 8 * 4
    one = ctypes.c_void_p(16)
    assert lib.v100_nbest_rescore(None, one, one, one, 1, one, 4, one, 3, one, 1, 0, 0, one, one, one, one, one, one, one, one, one, 1, 1, 4, 1,
                                  0.5, 0.0, 1, None) == 3
    # width 0: every hypothesis is empty
    empty = rescore_nbest(torch.zeros((2, 3, 0), dtype=torch.int64, device=cuda), torch.zeros((2, 3), dtype=torch.int32, device=cuda),
                          torch.tensor([[-1.0, -2.0, -math.inf]] * 2, device=cuda), dlm)
    assert empty.ids.shape == (2, 3, 0) and not empty.n_words.any() and empty.order.tolist() == [[0, 1, 2]] * 2
    assert empty.scores[0, 2] == -math.inf and empty.scores[0, 0] > empty.scores[0, 1]


@pytest.fixture(scope="module")
def tiny(cuda):
    model = AudioToTextCTC(64, 32, 29, 32)
    model.load_state_dict(sub(load_golden("asr_tiny.npz"), "state/"), strict=True)
    model = model.to(cuda).eval()
    gen = torch.Generator().manual_seed(12)
    frames = (96, 61, 80, 33)
    feats = torch.randn(4, max(frames), 64, generator=gen).to(cuda)
    lengths = torch.tensor(frames, dtype=torch.int32, device=cuda)
    with torch.no_grad():
        logits, out_len = model(feats), model.output_length(lengths)
    # a word model over what the beam search says on these rows, so that some of its words are known
    hyp = ctc_beam_search(logits, out_len, 8, 8)
    rows = [hyp[0][b, r, :int(hyp[1][b, r])].tolist() for b in range(4) for r in range(0, 8, 3)]
    wlm = WordNGramLM.fit(rows, 1, 3, unk_logp=-6.0).compile().to(cuda)
    return model, feats, lengths, logits, out_len, wlm


def test_pipeline(cuda, tiny):
    model, feats, lengths, logits, out_len, wlm = tiny
    kw = dict(word_lm=wlm, word_lm_weight=0.9, word_bonus=0.2)
    pipe = ASRPipeline(model, beam_size=8, nbest=3, **kw)
    plain = ASRPipeline(model, beam_size=8, nbest=3)
    text = torch.randint(1, 29, (4, 9), generator=torch.Generator().manual_seed(3)).to(cuda)
    text_len = torch.tensor([9, 4, 7, 1], dtype=torch.int32, device=cuda)
    for args, lens in (((feats,), None), ((feats, lengths), out_len)):
        first = ctc_beam_search(logits, lens, 8, 8)       # rescore_size defaults to beam_size
        want = rescore_nbest(*first, wlm, 0.9, 0.2)
        got = pipe.nbest(*args)
        assert isinstance(got, Rescored) and same(got, Rescored(*(t[:, :3] for t in want)))
        ids, n = pipe(*args)
        assert torch.equal(ids, got.ids[:, 0]) and torch.equal(n, got.lens[:, 0])
        assert same(plain.nbest(*args), ctc_beam_search(logits, lens, 8, 3))                  # without a word model: today's bits
        assert same(plain(*args), tuple(t[:, 0] for t in ctc_beam_search(logits, lens, 8, 1)[:2]))
    narrow = ASRPipeline(model, beam_size=8, nbest=2, rescore_size=4, **kw).nbest(feats, lengths)
    assert same(narrow, Rescored(*(t[:, :2] for t in rescore_nbest(*ctc_beam_search(logits, out_len, 8, 4), wlm, 0.9, 0.2))))
    s = pipe.score(feats, lengths, text, text_len)
    assert torch.equal(s["ids"], pipe(feats, lengths)[0])
    e = pipe.evaluate([(feats, lengths, text, text_len)])
    assert e["utterances"] == 4 and e["char_errors"] == int(s["char_errors"].sum())
    seg = ASRPipeline(model, beam_size=8, frame_seconds=0.02, **kw).segments(feats, lengths)
    assert torch.equal(seg["ids"], pipe(feats, lengths)[0]) and torch.equal(seg["ids_len"], pipe(feats, lengths)[1])
    # with a fused character model the fused score is the first pass
    clm = NGramLM.fit([[2, 3, 1, 4], [5, 1, 2, 3]], 29, 2).compile().to(cuda)
    fused = ASRPipeline(model, beam_size=8, nbest=2, lm=clm, lm_weight=0.3, **kw).nbest(feats, lengths)
    first = ctc_beam_search(logits, out_len, 8, 8, lm=clm, lm_weight=0.3)
    assert same(fused, Rescored(*(t[:, :2] for t in rescore_nbest(*first[:3], wlm, 0.9, 0.2))))


def test_long_pipeline(cuda):
    x, lab = C.planted(31, 1400, speech=(120, 260), amp=6.0)
    seq = lab[np.concatenate([[True], lab[1:] != lab[:-1]])]
    text = [int(v) for v in seq if v != 0]
    wlm = WordNGramLM.fit([text[i:i + 40] for i in range(0, len(text), 40)], 1, 2, unk_logp=-5.0).compile().to(cuda)
    xt = torch.from_numpy(x).to(cuda)
    kw = dict(beam_size=8, word_lm=wlm, word_lm_weight=0.8, word_bonus=0.1, rescore_size=6, frame_seconds=0.02, min_frames=20)
    want = LongASRPipeline(None, max_batch=4, **kw).segments(logits=xt)
    got = LongASRPipeline(None, max_batch=1, **kw).segments(logits=xt)
    assert int(want["seg_start"].shape[0]) >= 3 and got.keys() == want.keys()
    for k, v in want.items():
        if isinstance(v, torch.Tensor):
            assert got[k].shape == v.shape and torch.equal(bits(got[k]), bits(v)), k
    s, e = int(want["seg_start"][1]), int(want["seg_end"][1])                       # a piece is rescored as an utterance of its own
    piece = rescore_nbest(*ctc_beam_search(xt[s:e].clone()[None], None, 8, 6), wlm, 0.8, 0.1)
    n = int(piece.lens[0, 0])
    assert int(want["ids_len"][1]) == n and torch.equal(want["ids"][1, :n], piece.ids[0, 0, :n])
    assert torch.equal(bits(want["score"][1:2]), bits(piece.scores[0, :1]))
    whole = LongASRPipeline(None, **kw).whole(logits=xt, timed=False)
    first = ctc_beam_search_long(xt[None], None, 8, 6)
    width = max(int(first[1].max()), 1)
    ref = rescore_nbest(first[0][:, :, :width].contiguous(), first[1], first[2], wlm, 0.8, 0.1)
    n = int(ref.lens[0, 0])
    assert int(whole["ids_len"]) == n and torch.equal(whole["ids"][:n], ref.ids[0, 0, :n])
    assert torch.equal(bits(whole["score"].reshape(1)), bits(ref.scores[0, :1]))
    assert torch.equal(bits(whole["word_lm_score"].reshape(1)), bits(ref.word_lm_scores[0, :1]))
    untouched = LongASRPipeline(None, beam_size=8, frame_seconds=0.02, min_frames=20).whole(logits=xt, timed=False)
    assert int(untouched["ids_len"]) == int(first[1][0, 0]) and "word_lm_score" not in untouched
