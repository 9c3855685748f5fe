"""decode.mbr_nbest (K35, csrc/mbr.hip) and the pipelines' MBR stage against the float64 oracle of tests/_mbr_ref.py.

Per case of the list: dist, ref_dist, ref_n, n_tokens and order equal the oracle's (tests/test_mbr_cpu.py shows for the oracle alone that
its risks are far enough apart, or equal, for the order to be exact), posterior, risk and expected_len lie within the bound derived in
_mbr_ref, the rank-ordered outputs are the gather by order, order is the stable argsort of the returned risk, dist is symmetric, the
distances equal K23's edit_distance on the same rows, two calls give equal bits, and the workspace's content changes nothing."""
import math

import numpy as np
import pytest
import torch

import _cut_points_ref as C
import _mbr_ref as R
from conftest import load_golden, sub
from voice100_amd import _native as N
from voice100_amd.asr import AudioToTextCTC
from voice100_amd.decode import MBR, _mbr_launch, ctc_beam_search, ctc_beam_search_long, edit_distance, mbr_nbest, rescore_nbest
from voice100_amd.infer import ASRPipeline, LongASRPipeline
from voice100_amd.lm import WordNGramLM

pytestmark = pytest.mark.gpu

CASES = R.case_list()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return all((x is None and y is None) or (x.shape == y.shape and torch.equal(bits(x), bits(y))) for x, y in zip(a, b))


def to_numpy(out):
    return {k: None if v is None else v.cpu().numpy() for k, v in zip(out._fields, out)}


def on(dev, ids, lens, scores, kw):
    args = tuple(torch.from_numpy(a).to(dev) for a in (ids, lens, scores))
    kw = {k: torch.from_numpy(v).to(dev) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    return args, kw


def k23_pairs(ids, lens, scores, sep, ref=None, ref_len=None):
    """dist and ref_dist from ONE batched decode.edit_distance call over every (i, j) and (i, ref) of every utterance; -1 where absent"""
    B, n, T = ids.shape
    here = scores > -math.inf
    hyp, hl = ids[:, :, None].expand(B, n, n, T).reshape(-1, T), lens[:, :, None].expand(B, n, n).reshape(-1)
    oth, ol = ids[:, None].expand(B, n, n, T).reshape(-1, T), lens[:, None].expand(B, n, n).reshape(-1)
    both = (here[:, :, None] & here[:, None]).reshape(-1)
    if ref is not None:
        Tr = ref.shape[1]
        W = max(T, Tr)
        pad = lambda t, w: torch.nn.functional.pad(t, (0, W - w))            # noqa: E731
        hyp, oth = torch.cat([pad(hyp, T), pad(ids.reshape(-1, T), T)]), torch.cat([pad(oth, T), pad(ref[:, None].expand(B, n, Tr).reshape(-1, Tr), Tr)])
        hl = torch.cat([hl.clamp(0, T), lens.reshape(-1).clamp(0, T)])
        ol = torch.cat([ol.clamp(0, T), ref_len.to(torch.int32)[:, None].expand(B, n).reshape(-1).clamp(0, Tr)])
        both = torch.cat([both, here.reshape(-1)])
    d = edit_distance(hyp.contiguous(), hl.contiguous(), oth.contiguous(), ol.contiguous(), sep=sep)[0]
    d = torch.where(both, d, torch.full_like(d, -1))
    return d[:B * n * n].reshape(B, n, n), (d[B * n * n:].reshape(B, n) if ref is not None else None)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_case_against_the_oracle(cuda, case):
    name, ids, lens, scores, kw = CASES[case]
    ref = R.oracle(ids, lens, scores, **kw)
    args, dkw = on(cuda, ids, lens, scores, kw)
    B, n, T = ids.shape
    has_ref = "ref" in kw
    before = N.launch_count()
    out = mbr_nbest(*args, **dkw)
    assert N.launch_count() - before == (3 if n > 1 or has_ref else 2)       # no pair: no pair launch
    assert all(np.array_equal(a.cpu().numpy().view(np.int32), h.view(np.int32)) for a, h in zip(args, (ids, lens, scores)))
    assert isinstance(out, MBR) and out._fields == R.FIELDS
    assert out.ids.dtype == torch.int64 and out.ids.shape == (B, n, T) and out.dist.shape == (B, n, n) and out.expected_len.shape == (B,)
    for k in ("lens", "n_tokens", "order", "dist"):
        assert getattr(out, k).dtype == torch.int32, k
    for k in ("scores", "risk", "posterior", "expected_len"):
        assert getattr(out, k).dtype == torch.float32, k
    assert (out.ref_dist is None and out.ref_n is None) if not has_ref else (out.ref_dist.shape == (B, n) and out.ref_n.shape == (B,))
    bad, worst = R.check(name, to_numpy(out), ref, ids, lens, scores)
    print(f"{name}: worst error over bound {worst}")
    assert bad == []
    # an independent check against K23 on the same rows
    d, rd = k23_pairs(*args, kw.get("sep", R.SEP), dkw.get("ref"), dkw.get("ref_len"))
    assert torch.equal(out.dist, d) and (rd is None or torch.equal(out.ref_dist, rd))
    assert same(out, mbr_nbest(*args, **dkw))            # two calls: equal bits
    nbytes = N.helper("v100_nbest_mbr_workspace_bytes", B, n, T, kw["ref"].shape[1] if has_ref else 0)
    PAD = 256
    for poison in (0x00, 0xFF):                          # the workspace's content inside canaries: the same bits, the canaries untouched
        ws = torch.full((nbytes + 2 * PAD,), poison, dtype=torch.uint8, device=cuda)
        again = _mbr_launch(*args, kw.get("sep", R.SEP), kw.get("scale", 1.0), dkw.get("ref"), dkw.get("ref_len"), ws=ws[PAD:PAD + nbytes])
        assert same(out, again), (name, poison)
        assert bool((ws[:PAD] == poison).all()) and bool((ws[PAD + nbytes:] == poison).all())


def test_the_mbr_choice_is_not_rank_0(cuda):
    ids, lens, scores = R.flip_case()
    out = mbr_nbest(*(torch.from_numpy(a).to(cuda) for a in (ids, lens, scores)))
    assert bool((out.order[:, 0] != 0).all()) and out.order.tolist() == [[1, 2, 0]]
    assert out.ids[0, 0, :7].tolist() == R.words(15, 16, 17, 18) and float(out.risk[0, 0]) == pytest.approx(1.9, rel=1e-6)
    sharp = mbr_nbest(*(torch.from_numpy(a).to(cuda) for a in (ids, lens, scores)), scale=50.0)      # nearly one-hot: the best score again
    assert sharp.order.tolist() == [[0, 1, 2]]


def long_rows(rng, T=4096, n=64):
    """n copies of a base row of T ids, each with at most 8 scattered edits"""
    base = rng.integers(2, 29, size=T).tolist()
    rows = []
    for k in range(n):
        row = list(base)
        for _ in range(int(rng.integers(0, 9)) if k else 0):
            at, what = int(rng.integers(0, len(row))), int(rng.integers(0, 3))
            if what == 0:
                row[at] = int(rng.integers(2, 29))
            elif what == 1:
                del row[at]
            else:
                row.insert(at, int(rng.integers(2, 29)))
        rows.append(row[:T])
    return rows


def test_limit_shape_and_refusals(cuda):
    """N = 64 rows of 4096 ids, B = 1: every pair against K23 (one batched call), eight against the numpy oracle; then the refusals"""
    rng = np.random.default_rng(64)
    rows = long_rows(rng)
    rows[7] = rows[7][:4096 - 700]                       # a middle that ends before the other's
    ids, lens = R.pack([rows], 4096)
    scores = np.sort(rng.uniform(-9.0, -1.0, size=(1, 64)))[:, ::-1].astype(np.float32).copy()
    args = tuple(torch.from_numpy(a).to(cuda) for a in (ids, lens, scores))
    out = mbr_nbest(*args, sep=None)
    iu = torch.triu_indices(64, 64, 1, device=cuda)
    d = edit_distance(args[0][0, iu[0]].contiguous(), args[1][0, iu[0]].contiguous(), args[0][0, iu[1]].contiguous(),
                      args[1][0, iu[1]].contiguous())[0]
    assert torch.equal(out.dist[0, iu[0], iu[1]], d) and torch.equal(out.dist[0], out.dist[0].T) and not out.dist[0].diagonal().any()
    for i, j in ((0, 1), (1, 0), (7, 8), (2, 63), (31, 32), (5, 7), (62, 63), (40, 11)):
        assert int(out.dist[0, i, j]) == R.levenshtein(rows[i], rows[j]), (i, j)
    assert out.n_tokens[0].tolist() == [len(rows[j]) for j in out.order[0].tolist()]
    order = out.order[0].cpu().numpy()
    key = np.empty(64, dtype=np.float32)
    key[order] = out.risk[0].cpu().numpy()
    assert np.array_equal(np.argsort(key, kind="stable"), order)
    post = R.oracle(np.zeros((1, 64, 1), dtype=np.int64), np.zeros((1, 64), dtype=np.int32), scores)["posterior"][0]
    risk = np.array([sum(post[j] * float(out.dist[0, i, j]) for j in range(64) if j != i) for i in range(64)])
    assert np.all(np.abs(key.astype(np.float64) - risk) <= R.bound(risk))
    # the word level at the same width: up to 2048 words a row
    w_ids = ids.copy()
    w_ids[:, :, 1::2] = R.SEP
    w_args = (torch.from_numpy(w_ids).to(cuda),) + args[1:]
    w_out = mbr_nbest(*w_args)
    w_d = edit_distance(w_args[0][0, iu[0]].contiguous(), args[1][0, iu[0]].contiguous(), w_args[0][0, iu[1]].contiguous(),
                        args[1][0, iu[1]].contiguous(), sep=R.SEP)[0]
    assert torch.equal(w_out.dist[0, iu[0], iu[1]], w_d) and int(w_out.n_tokens.max()) == 2048

    small = tuple(torch.from_numpy(a).to(cuda) for a in R.flip_case())
    before = N.launch_count()
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device=cuda)     # noqa: E731
    with pytest.raises(RuntimeError, match="nbest = 65 <= 64"):
        mbr_nbest(z(1, 65, 4, dt=torch.int64), z(1, 65), z(1, 65, dt=torch.float32))
    with pytest.raises(RuntimeError, match="T = 4097 <= 4096"):
        mbr_nbest(z(1, 2, 4097, dt=torch.int64), z(1, 2), z(1, 2, dt=torch.float32))
    with pytest.raises(RuntimeError, match="Tr = 4097 <= 4096"):
        mbr_nbest(*small, ref=z(1, 4097, dt=torch.int64), ref_len=z(1))
    for scale in (-1.0, math.inf, math.nan):
        with pytest.raises(RuntimeError, match="scale"):
            mbr_nbest(*small, scale=scale)
    with pytest.raises(RuntimeError, match="as ctc_beam_search returns them"):
        mbr_nbest(small[0], small[1][:, :0], small[2])
    with pytest.raises(RuntimeError, match="ref \\[B, Tr\\]"):
        mbr_nbest(*small, ref=z(2, 4, dt=torch.int64), ref_len=z(2))
    with pytest.raises(RuntimeError, match="workspace"):
        _mbr_launch(*small, 1, 1.0, None, None, ws=torch.zeros(8, dtype=torch.uint8, device=cuda))
    assert N.launch_count() == before
    # width 0: every hypothesis is empty
    empty = mbr_nbest(z(2, 3, 0, dt=torch.int64), z(2, 3), torch.tensor([[-1.0, -2.0, -math.inf]] * 2, device=cuda),
                      ref=z(2, 0, dt=torch.int64), ref_len=z(2))
    assert empty.ids.shape == (2, 3, 0) and not empty.n_tokens.any() and empty.order.tolist() == [[0, 1, 2]] * 2
    assert empty.dist[0].tolist() == [[0, 0, -1], [0, 0, -1], [-1, -1, -1]] and empty.ref_dist.tolist() == [[0, 0, -1]] * 2
    assert empty.risk[0].tolist() == [0.0, 0.0, math.inf] and not empty.ref_n.any() and not empty.expected_len.any()


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
    hyp = ctc_beam_search(logits, out_len, 8, 8)
    rows = [hyp[0][b, r, :int(hyp[1][b, r])].tolist() for b in range(4) for r in range(0, 8, 3)]
    wlm = WordNGramLM.fit(rows, 1, 3, unk_logp=-6.0).compile().to(cuda)
    return model, feats, lengths, logits, out_len, wlm


def cut(m, n):
    return MBR(*(t[:, :n] for t in m[:7]), *m[7:])


def test_pipeline(cuda, tiny):
    model, feats, lengths, logits, out_len, wlm = tiny
    plain = ASRPipeline(model, beam_size=8, nbest=3)
    for level, sep in (("word", 1), ("id", None)):
        pipe = ASRPipeline(model, beam_size=8, nbest=3, mbr=level, mbr_scale=0.5)
        for args, lens in (((feats,), None), ((feats, lengths), out_len)):
            want = mbr_nbest(*ctc_beam_search(logits, lens, 8, 8), sep=sep, scale=0.5)       # mbr_size defaults to beam_size
            got = pipe.nbest(*args)
            assert isinstance(got, MBR) and same(got, cut(want, 3)) and got.ids.shape[1] == 3 and got.dist.shape == (4, 8, 8)
            ids, n = pipe(*args)
            assert torch.equal(ids, want.ids[:, 0]) and torch.equal(n, want.lens[:, 0])
            # mbr=None: what a pipeline built without the argument returns
            none = ASRPipeline(model, beam_size=8, nbest=3, mbr=None)
            assert same(none.nbest(*args), plain.nbest(*args)) and same(none(*args), plain(*args))
            assert same(plain.nbest(*args), ctc_beam_search(logits, lens, 8, 3))
    kw = dict(word_lm=wlm, word_lm_weight=0.9, word_bonus=0.2)
    both = ASRPipeline(model, beam_size=8, nbest=2, rescore_size=6, mbr="word", **kw)        # mbr_size defaults to rescore_size
    assert both.mbr_size == 6
    second = rescore_nbest(*ctc_beam_search(logits, out_len, 8, 6), wlm, 0.9, 0.2)
    want = mbr_nbest(second.ids, second.lens, second.scores)
    assert same(both.nbest(feats, lengths), cut(want, 2))
    ids, n = both(feats, lengths)
    assert torch.equal(ids, want.ids[:, 0]) and torch.equal(n, want.lens[:, 0])
    narrow = ASRPipeline(model, beam_size=8, nbest=2, mbr="word", mbr_size=4).nbest(feats, lengths)
    assert same(narrow, cut(mbr_nbest(*ctc_beam_search(logits, out_len, 8, 4)), 2))
    # what is built on the call follows
    pipe = ASRPipeline(model, beam_size=8, mbr="word", frame_seconds=0.02)
    text = torch.randint(1, 29, (4, 9), generator=torch.Generator().manual_seed(3)).to(cuda)
    text_len = torch.tensor([9, 4, 7, 1], dtype=torch.int32, device=cuda)
    s = pipe.score(feats, lengths, text, text_len)
    assert torch.equal(s["ids"], pipe(feats, lengths)[0])
    e = pipe.evaluate([(feats, lengths, text, text_len)])
    assert e["utterances"] == 4 and e["char_errors"] == int(s["char_errors"].sum())
    seg = pipe.segments(feats, lengths)
    assert torch.equal(seg["ids"], pipe(feats, lengths)[0]) and torch.equal(seg["ids_len"], pipe(feats, lengths)[1])


def test_long_pipeline(cuda):
    x, _ = C.planted(31, 1400, speech=(120, 260), amp=6.0)
    xt = torch.from_numpy(x).to(cuda)
    kw = dict(beam_size=8, frame_seconds=0.02, min_frames=20)
    long = LongASRPipeline(None, mbr="word", mbr_scale=0.5, mbr_size=6, **kw)
    assert (long.asr.mbr, long.asr.mbr_scale, long.asr.mbr_size) == ("word", 0.5, 6)
    whole = long.whole(logits=xt, timed=False)
    first = ctc_beam_search_long(xt[None], None, 8, 6)
    width = max(int(first[1].max()), 1)
    want = mbr_nbest(first[0][:, :, :width].contiguous(), first[1], first[2], scale=0.5)
    n = int(want.lens[0, 0])
    assert int(whole["ids_len"]) == n and torch.equal(whole["ids"][:n], want.ids[0, 0, :n])
    assert torch.equal(bits(whole["score"].reshape(1)), bits(want.scores[0, :1]))
    assert torch.equal(bits(whole["risk"].reshape(1)), bits(want.risk[0, :1]))
    assert torch.equal(bits(whole["expected_len"].reshape(1)), bits(want.expected_len[:1]))
    # a piece of segments() is selected as an utterance of its own
    seg = long.segments(logits=xt)
    s, e = int(seg["seg_start"][1]), int(seg["seg_end"][1])
    piece = mbr_nbest(*ctc_beam_search(xt[s:e].clone()[None], None, 8, 6), scale=0.5)
    n = int(piece.lens[0, 0])
    assert int(seg["ids_len"][1]) == n and torch.equal(seg["ids"][1, :n], piece.ids[0, 0, :n])
    untouched = LongASRPipeline(None, **kw).whole(logits=xt, timed=False)
    assert int(untouched["ids_len"]) == int(first[1][0, 0]) and "risk" not in untouched
