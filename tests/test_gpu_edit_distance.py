"""decode.edit_distance / edit_distance_both (K23, csrc/edit_distance.hip), infer.ErrorRate and ASRPipeline.score / evaluate against
the host references of tests/_edit_ref.py.  Every assertion is exact equality: the distance and the token counts are integers and
unique.  The kernel's seams: lane l of the wave owns a strip of S reference tokens, S = 1, 2, 4, 8, 16, 32, 64 -- the smallest with
64 S >= the reference's tokens -- so the strip width changes after 64, 128, 256, 512, 1024 and 2048 reference tokens; the
hypothesis' tokens are fetched 64 rows at a time, and the word segmentation walks 64 positions at a time."""
import numpy as np
import pytest
import torch

from _edit_ref import lev_rows, score_rows, split_words, word_ids
from conftest import load_golden, sub
from voice100_amd import _native as N
from voice100_amd.asr import AudioToTextCTC
from voice100_amd.decode import edit_distance, edit_distance_both
from voice100_amd.infer import ASRPipeline, ErrorRate

pytestmark = pytest.mark.gpu

SEAMS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000)
STRIP_SEAMS = (512, 513, 1024, 1025, 2048, 2049)         # reference lengths at which the strip width S changes (beyond SEAMS)


def pad(rows, width=None, garbage=None):
    """rows (sequences of ints) -> ([B, width] int64 zero padded -- or padded with random ids from `garbage` --, lengths [B] int32)."""
    width = max([len(r) for r in rows] + [1]) if width is None else width
    out = np.zeros((len(rows), width), np.int64) if garbage is None else garbage.integers(-3, 31, (len(rows), width)).astype(np.int64)
    for b, r in enumerate(rows):
        out[b, :len(r)] = np.asarray(r, np.int64)
    return out, np.array([len(r) for r in rows], np.int32)


def run(dev, hyp_rows, ref_rows, sep=None, th=None, tr=None, garbage=None):
    """One call on padded batches; returns ((dist, hyp_n, ref_n) as lists, the host reference's)."""
    h, hl = pad(hyp_rows, th, garbage)
    r, rl = pad(ref_rows, tr, garbage)
    got = edit_distance(*(torch.from_numpy(x).to(dev) for x in (h, hl, r, rl)), sep=sep)
    assert all(g.dtype == torch.int32 and g.shape == (len(hyp_rows),) for g in got)
    return [g.tolist() for g in got], score_rows(h, hl, r, rl, sep)


def edits(rng, row, rate, vocab):
    """`row` with about `rate` of its positions substituted, deleted or followed by an insertion."""
    out = []
    for x in row:
        u = rng.random()
        if u < rate / 3:
            continue
        out.append(int(rng.integers(*vocab)) if u < 2 * rate / 3 else int(x))
        if u > 1 - rate / 3:
            out.append(int(rng.integers(*vocab)))
    return out


def test_id_mode_seams(cuda):
    rng = np.random.default_rng(0)
    pairs = [(n, m) for n in SEAMS for m in SEAMS] + [(n, m) for n in (1, 65, 300) for m in STRIP_SEAMS]
    hyp = [rng.integers(1, 5, n).tolist() for n, _ in pairs]                 # a small vocabulary: many matches, many ties
    ref = [rng.integers(1, 5, m).tolist() for _, m in pairs]
    got, want = run(cuda, hyp, ref)
    assert got == want
    assert want[1] == [n for n, _ in pairs] and want[2] == [m for _, m in pairs]


def test_id_mode_extremes(cuda):
    rng = np.random.default_rng(1)
    big_h, big_r = rng.integers(1, 29, 4096).tolist(), rng.integers(1, 29, 4096).tolist()
    got, want = run(cuda, [big_h, big_h, [7], [], big_r], [big_r, [5], big_r, [], big_r])
    assert got == want and want[0][3] == 0 and want[0][4] == 0
    got, want = run(cuda, [[]], [[]])                                        # 0 x 0 alone
    assert got == want == [[0], [0], [0]]
    e = torch.zeros((2, 0), dtype=torch.int64, device=cuda)                  # tensors without a column
    z = torch.zeros(2, dtype=torch.int32, device=cuda)
    assert [g.tolist() for g in edit_distance(e, z, e, z)] == [[0, 0]] * 3
    with pytest.raises(RuntimeError, match="4096"):
        edit_distance(torch.zeros((1, 4097), dtype=torch.int64, device=cuda), z[:1], torch.zeros((1, 8), dtype=torch.int64, device=cuda), z[:1])


def test_id_mode_content(cuda):
    rng = np.random.default_rng(2)
    base = rng.integers(1, 29, 700).tolist()
    hyp, ref = [], []
    hyp.append(base); ref.append(base)                                       # identical
    hyp.append(rng.integers(1, 10, 333).tolist()); ref.append(rng.integers(10, 20, 190).tolist())   # no common id
    for n, m in ((500, 400), (131, 517), (64, 64)):                          # binary vocabulary: long runs of ties
        hyp.append(rng.integers(0, 2, n).tolist()); ref.append(rng.integers(0, 2, m).tolist())
    hyp += [base, base, base]; ref += [base[:250], base[-250:], base[200:450]]                       # prefix, suffix, interior slice
    for n in (40, 300, 700):                                                 # about 10 % edits
        ref.append(base[:n]); hyp.append(edits(rng, base[:n], 0.1, (1, 29)))
    got, want = run(cuda, hyp, ref)
    assert got == want
    assert want[0][0] == 0 and want[0][1] == 333 and want[0][5:8] == [450, 450, 450]


def test_padding_is_never_read(cuda):
    rng = np.random.default_rng(3)
    ref = [rng.integers(1, 29, m).tolist() for m in (0, 1, 64, 65, 130, 300)]
    hyp = [edits(rng, r, 0.2, (1, 29)) for r in ref]
    hyp[0] = [4, 5]
    for sep in (None, 1):
        plain, want = run(cuda, hyp, ref, sep)
        assert plain == want
        for th, tr in ((None, None), (1500, 2100)):                          # garbage in the padding; widths far beyond the rows
            got, _ = run(cuda, hyp, ref, sep, th, tr, garbage=np.random.default_rng(4))
            assert got == plain, (sep, th, tr)
    # lengths outside [0, width] are clamped
    h, hl = pad(hyp)
    r, rl = pad(ref)
    hl2, rl2 = hl.copy(), rl.copy()
    hl2[1], rl2[2], hl2[3] = 10 ** 6, 10 ** 6, -5
    got = edit_distance(*(torch.from_numpy(x).to(cuda) for x in (h, hl2, r, rl2)))
    assert [g.tolist() for g in got] == score_rows(h, hl2, r, rl2)


def test_ids_compare_on_64_bits(cuda):
    rng = np.random.default_rng(5)
    small = rng.integers(0, 6, 150)
    hyp = [(2 ** 40 + small).tolist(), (-small - 1).tolist(), small.tolist(), (small + 2 ** 32).tolist(),
           [-2 ** 63, 2 ** 63 - 1, 0, -1], (small * 2 ** 32).tolist()]
    other = rng.integers(0, 6, 170)
    ref = [(2 ** 40 + other).tolist(), (-other - 1).tolist(), (small + 2 ** 32).tolist(), (small + 2 ** 33).tolist(),
           [2 ** 63 - 1, -2 ** 63, -1, 0], (other * 2 ** 32).tolist()]
    got, want = run(cuda, hyp, ref)
    assert got == want and want[0][2] == 150 and want[0][3] == 150           # equal low halves, different high halves: no match
    sep = 2 ** 40 + 1                                                        # words of 64-bit ids, a 64-bit separator
    got, want = run(cuda, hyp[:1] + [[5, sep, 5 + 2 ** 32]], ref[:1] + [[5 + 2 ** 32, sep, 5]], sep=sep)
    assert got == want and want[0][1] == 2


def test_batch_sizes(cuda):
    rng = np.random.default_rng(6)
    for B, top in ((1, 200), (70, 200), (1100, 20)):                         # one pair; 70; more workgroups than the device has CUs
        ref = [rng.integers(1, 8, rng.integers(0, top)).tolist() for _ in range(B)]
        hyp = [edits(rng, r, 0.3, (1, 8)) for r in ref]
        for sep in (None, 1):
            got, want = run(cuda, hyp, ref, sep)
            assert got == want, (B, sep)


def test_word_mode(cuda):
    S = 1
    long_a, long_b = list(range(2, 102)), list(range(2, 101)) + [7]          # words longer than 64 ids, equal up to the last id
    many = [x for k in range(300) for x in (2 + k % 5, S)]                   # 300 one-id words
    cases = [
        ([S, S, 2, 3, S, S, 4, S], [2, 3, S, 4]),                            # leading, doubled, trailing separators: the same words
        ([S, S, S, S], [2, 3, S, 4]),                                        # a row of separators only
        ([S, S], []),
        ([2, 3, 4], [2, 3, 4]),                                              # one word, no separator at all
        ([2, 3, 4], [2, 3, 5]),
        ([2, 3, S, 2, 3, 4], [2, 3, 4, S, 2, 3]),                            # words that differ only in length
        ([2, 3], [2, 3, 4]),
        (long_a + [S] + long_b, long_b + [S] + long_a + [S] + long_a),
        (long_a, long_a[:64]),
        (many, many[:-2] + [9, 9, S]),
        (many[2:], many),
        ([x for x in many if x != S], many),                                 # one 300-id word against 300 words
        ([5, 6, 7, 8], [5, 6, 9, 8]),                                        # (sep absent from the data: below)
    ]
    got, want = run(cuda, [c[0] for c in cases], [c[1] for c in cases], sep=S)
    assert got == want
    assert want[0][:4] == [0, 2, 0, 0] and want[1][:4] == [2, 0, 0, 1] and want[2][:4] == [2, 2, 0, 1]      # hyp_n / ref_n count words
    assert want[1][9] == 300 and want[2][9] == 300 and want[1][11] == 1
    got, want = run(cuda, [c[0] for c in cases], [c[1] for c in cases], sep=777)         # sep absent: every non-empty row is one word
    assert got == want and all(n <= 1 for n in want[1])
    # the str.split() cross-check on decoded strings, ids over " abc" with the space as the separator
    rng = np.random.default_rng(7)
    alphabet = " abc"
    ref = [rng.choice(4, rng.integers(0, 400), p=(0.25, 0.25, 0.25, 0.25)).tolist() for _ in range(40)]
    hyp = [edits(rng, r, 0.1, (0, 4)) for r in ref]
    got, _ = run(cuda, hyp, ref, sep=0)
    for b in range(40):
        hw, rw = ("".join(alphabet[x] for x in row).split() for row in (hyp[b], ref[b]))
        hi, ri = word_ids(hw, rw)
        assert (got[0][b], got[1][b], got[2][b]) == (lev_rows(hi, ri), len(hw), len(rw)), b
        assert [tuple(alphabet.index(c) for c in w) for w in hw] == split_words(hyp[b], 0)


@pytest.fixture(scope="module")
def batch(cuda):
    """A validation-like batch: references over the 29-symbol vocabulary with a space about every sixth id, hypotheses = the
    references with about 10 % edits; host scores at both levels, computed once."""
    rng = np.random.default_rng(8)
    ref = [np.where(rng.random(m) < 1 / 6, 1, rng.integers(2, 29, m)).tolist() for m in rng.integers(0, 300, 24)]
    hyp = [edits(rng, r, 0.1, (1, 29)) for r in ref]
    h, hl = pad(hyp, garbage=np.random.default_rng(9))
    r, rl = pad(ref, garbage=np.random.default_rng(10))
    dev = tuple(torch.from_numpy(x).to(cuda) for x in (h, hl, r, rl))
    return {"dev": dev, "chars": score_rows(h, hl, r, rl), "words": score_rows(h, hl, r, rl, sep=1)}


def test_both_levels_totals_launches_and_determinism(batch, cuda):
    dev, chars, words = batch["dev"], batch["chars"], batch["words"]
    edit_distance_both(*dev)                             # (the library is loaded: the count below is of launches alone)
    before = N.launch_count()
    both = edit_distance_both(*dev, sep=1)
    assert N.launch_count() - before <= 2
    assert all(t.shape == (2, 24) and t.dtype == torch.int32 for t in both)
    assert [t[0].tolist() for t in both] == chars and [t[1].tolist() for t in both] == words
    again = edit_distance_both(*dev, sep=1)
    assert all(torch.equal(a, b) for a, b in zip(both, again))               # two runs are bit-equal
    want = torch.tensor([[sum(c) for c in chars], [sum(c) for c in words]], dtype=torch.int64)
    totals = torch.zeros((2, 3), dtype=torch.int64, device=cuda)
    full = edit_distance_both(*dev, sep=1, totals=totals)
    assert all(torch.equal(a, b) for a, b in zip(both, full)) and torch.equal(totals.cpu(), want)
    assert edit_distance_both(*dev, sep=1, totals=totals, per_row=False) is None         # totals only; a second call accumulates
    assert torch.equal(totals.cpu(), 2 * want)
    for sep, rows in ((None, chars), (1, words)):        # the one-level call: per-row only, both, totals only
        t1 = torch.zeros(3, dtype=torch.int64, device=cuda)
        assert [t.tolist() for t in edit_distance(*dev, sep=sep)] == rows
        assert [t.tolist() for t in edit_distance(*dev, sep=sep, totals=t1)] == rows
        assert edit_distance(*dev, sep=sep, totals=t1, per_row=False) is None
        assert t1.tolist() == [2 * sum(c) for c in rows]
    with pytest.raises(RuntimeError):
        edit_distance(*dev, per_row=False)               # nothing asked for
    with pytest.raises(RuntimeError):
        edit_distance(*dev, totals=torch.zeros(3, dtype=torch.int32, device=cuda))


def test_error_rate(cuda):
    rng = np.random.default_rng(11)
    meter, phones = ErrorRate(), ErrorRate(sep=None)
    want = np.zeros((2, 3), np.int64)
    batches = []
    for B, top in ((5, 40), (1, 130), (9, 300)):         # three batches of different widths and B
        ref = [np.where(rng.random(m) < 1 / 6, 1, rng.integers(2, 29, m)).tolist() for m in rng.integers(1, top, B)]
        hyp = [edits(rng, r, 0.15, (1, 29)) for r in ref]
        h, hl = pad(hyp)
        r, rl = pad(ref)
        want += np.array([[sum(c) for c in score_rows(h, hl, r, rl)], [sum(c) for c in score_rows(h, hl, r, rl, sep=1)]])
        batches.append(tuple(torch.from_numpy(x).to(cuda) for x in (h, hl, r, rl)))
    meter.update(*batches[0])
    phones.update(*batches[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")              # update must not synchronise with the host
    try:
        for b in batches[1:]:
            meter.update(*b)
            phones.update(*b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out = meter.compute()
    assert out == {"cer": int(want[0, 0]) / int(want[0, 2]), "wer": int(want[1, 0]) / int(want[1, 2]), "char_errors": int(want[0, 0]),
                   "chars": int(want[0, 2]), "word_errors": int(want[1, 0]), "words": int(want[1, 2]), "utterances": 15}
    assert phones.compute() == {"cer": out["cer"], "char_errors": out["char_errors"], "chars": out["chars"], "utterances": 15}
    meter.reset()
    assert meter.totals.tolist() == [[0, 0, 0], [0, 0, 0]] and meter.compute()["utterances"] == 0
    meter.update(*batches[1])
    assert meter.compute()["chars"] == int(batches[1][3].sum())


def test_pipeline_score_and_evaluate(cuda):
    model = AudioToTextCTC(64, 32, 29, 32)
    model.load_state_dict(sub(load_golden("asr_tiny.npz"), "state/"), strict=True)
    pipe = ASRPipeline(model.to(cuda).eval())
    gen = torch.Generator().manual_seed(12)
    rng = np.random.default_rng(13)
    data, hyps, refs = [], [], []
    for frames in ((96, 61, 80, 33), (48, 70, 19, 64)):  # two ragged batches of 4
        feats = torch.randn(4, max(frames), 64, generator=gen).to(cuda)
        lengths = torch.tensor(frames, dtype=torch.int32, device=cuda)
        ref = [np.where(rng.random(m) < 1 / 5, 1, rng.integers(2, 29, m)).tolist() for m in rng.integers(1, 30, 4)]
        t, tl = pad(ref)
        text, text_len = torch.from_numpy(t).to(cuda), torch.from_numpy(tl).to(cuda)
        ids, n = pipe(feats, lengths)
        out = pipe.score(feats, lengths, text, text_len)
        assert torch.equal(out["ids"], ids) and torch.equal(out["ids_len"], n)
        chars, words = score_rows(ids.cpu().numpy(), n.cpu().numpy(), t, tl), score_rows(ids.cpu().numpy(), n.cpu().numpy(), t, tl, sep=1)
        assert [out[k].tolist() for k in ("char_errors", "hyp_chars", "chars")] == chars
        assert [out[k].tolist() for k in ("word_errors", "hyp_words", "words")] == words
        data.append((feats, lengths, text, text_len))
        hyps += [chars, words]
    res = pipe.evaluate(data)
    ce, cn = sum(hyps[0][0]) + sum(hyps[2][0]), sum(hyps[0][2]) + sum(hyps[2][2])
    we, wn = sum(hyps[1][0]) + sum(hyps[3][0]), sum(hyps[1][2]) + sum(hyps[3][2])
    assert res == {"cer": ce / cn, "wer": we / wn, "char_errors": ce, "chars": cn, "word_errors": we, "words": wn, "utterances": 8}
