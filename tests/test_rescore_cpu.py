"""lm.WordNGramLM (K34) without a GPU: the ARPA round trip and its errors, fit against NGramLM.fit, the compiled tables through the numpy
mirror of tests/_rescore_ref.py, unknown words, the condition on the case list that makes the GPU test's ranking comparison exact, and
the pipelines' refusal of a word model without a beam."""
import math

import numpy as np
import pytest
import torch

import _rescore_ref as R
from voice100_amd.lm import MAX_ORDER, NGramLM, WordNGramLM

BOS, EOS, UNK = WordNGramLM.BOS, WordNGramLM.EOS, WordNGramLM.UNK


def test_arpa_read():
    lm = WordNGramLM.from_arpa(R.ARPA_UNK, R.SYMBOLS)
    the, cat, sat = (tuple(R.spell(w)) for w in ("the", "cat", "sat"))
    assert lm.order == 3 and [len(t) for t in lm.ngrams] == [6, 6, 2] and not lm.has_bos and not lm.has_eos
    ln10 = math.log(10.0)
    assert lm.ngrams[0][(cat,)] == (-1.1 * ln10, 0.125 * ln10) and lm.ngrams[0][(UNK,)] == (-1.2 * ln10, -0.31 * ln10)
    assert lm.ngrams[2][(the, UNK, sat)] == (-0.35 * ln10, 0.0) and (tuple(R.spell("it's")),) in lm.ngrams[0]
    # the float64 walk: a listed trigram, a back-off through a listed context, one through an unlisted context, an unknown word
    assert lm.log_prob((the, cat), sat) == -0.2 * ln10
    assert lm.log_prob((cat, sat), the) == 0.0 + -0.2 * ln10 + -0.9 * ln10                    # (cat sat) has no weight, (sat) -0.2
    assert lm.log_prob((sat, sat), cat) == -0.2 * ln10 + -1.1 * ln10                           # (sat sat) is not listed
    dog = tuple(R.spell("dog"))
    assert lm.token(dog) == UNK and lm.log_prob((the,), dog) == -0.7 * ln10 and lm.log_prob((the, dog), sat) == -0.35 * ln10
    assert lm.log_prob_eos((the,)) == 0.0
    both = WordNGramLM.from_arpa(R.ARPA_BOS, R.SYMBOLS, unk_logp=-7.5)
    assert both.has_bos and both.has_eos and both.start_history() == (BOS,)
    assert both.log_prob_eos((BOS, the, cat)) == -0.45 * ln10 and both.log_prob((BOS,), the) == -0.25 * ln10


def test_arpa_skips_foreign_tokens():
    """n-grams that hold a token with a character outside the symbols are skipped, and still count against the header"""
    text = R.ARPA_BOS.replace("-1.4\tsat", "-1.4\tsät").replace("-0.65\tcat sat", "-0.65\tcat sät")
    lm = WordNGramLM.from_arpa(text, R.SYMBOLS)
    assert [len(t) for t in lm.ngrams] == [4, 3]


def test_arpa_round_trip():
    for text, kw in ((R.ARPA_UNK, {}), (R.ARPA_BOS, {"unk_logp": -7.5})):
        lm = WordNGramLM.from_arpa(text, R.SYMBOLS, **kw)
        again = WordNGramLM.from_arpa(lm.to_arpa(), R.SYMBOLS, **kw)
        assert again.order == lm.order and [set(t) for t in again.ngrams] == [set(t) for t in lm.ngrams]
        for t, u in zip(lm.ngrams, again.ngrams):
            for g, (lp, bow) in t.items():
                assert abs(u[g][0] - lp) < 3e-9 and abs(u[g][1] - bow) < 3e-9
    fitted, _ = R.fit_model(5, 3, size=8, count=20)
    again = WordNGramLM.from_arpa(fitted.to_arpa(R.SYMBOLS), R.SYMBOLS)
    assert [set(t) for t in again.ngrams] == [set(t) for t in fitted.ngrams]
    with pytest.raises(ValueError, match="symbols"):
        fitted.to_arpa()


@pytest.mark.parametrize("damage, line", [
    (lambda t: t.replace("\\data\\", "\\date\\"), 1),
    (lambda t: t.replace("ngram 2=4", "ngram 3=4"), 3),
    (lambda t: t.replace("-0.5\tthe cat", "-0.5\tthe cat x y"), 14),
    (lambda t: t.replace("-0.5\tthe cat", "zero\tthe cat"), 14),
    (lambda t: t.replace("-0.5\tthe cat", "-0.5\tdog cat"), 14),
    (lambda t: t.replace("-0.45\tcat </s>\n", ""), 17),
    (lambda t: t.replace("\\end\\", ""), 19),
])
def test_arpa_errors_name_the_line(damage, line):
    with pytest.raises(ValueError, match=f"ARPA line {line}:"):
        WordNGramLM.from_arpa(damage(R.ARPA_BOS), R.SYMBOLS)
    with pytest.raises(ValueError, match="above the limit"):
        WordNGramLM.from_arpa("\\data\\\n" + "".join(f"ngram {n}=1\n" for n in range(1, MAX_ORDER + 2)), R.SYMBOLS)


def test_fit_equals_ngramlm_fit_on_word_numbers():
    rng = np.random.default_rng(3)
    lex = R.lexicon(rng, 12)
    sents = R.sentences(rng, lex, 40)
    num = {w: i + 1 for i, w in enumerate(sorted(lex))}
    for order in (1, 2, 4):
        words = WordNGramLM.fit([R.join(s) for s in sents], R.SEP, order)
        base = NGramLM.fit([[num[w] for w in s] for s in sents], len(lex) + 1, order)
        name = {i: w for w, i in num.items()}
        name[base.bos], name[base.eos] = BOS, EOS
        for t, u in zip(base.ngrams, words.ngrams):
            assert {tuple(name[x] for x in g): v for g, v in t.items()} == u                 # equal float64 values, entry by entry
        for s in sents[:10]:
            hw, hn = list(words.start_history()), list(base.start_history())
            for w in s:
                assert words.log_prob(hw, w) == base.log_prob(hn, num[w])
                hw.append(w)
                hn.append(num[w])
            assert words.log_prob_eos(hw) == base.log_prob_eos(hn)
    # leading, trailing and doubled separators do not make words
    a = WordNGramLM.fit([[1, 1, 5, 6, 1, 1, 7, 1]], 1, 2)
    assert a.ngrams[0].keys() == WordNGramLM.fit([[5, 6, 1, 7]], 1, 2).ngrams[0].keys() == {(BOS,), (EOS,), ((5, 6),), ((7,),)}


def models():
    out = [(name, lm) for name, lm in {id(c[1]): (c[0], c[1]) for c in R.case_list()}.values()]
    return out + [("fit, table_bits 1", R.fit_model(21, 4, size=30, count=50, table_bits=1)[0])]


def test_every_listed_entry_is_found_and_no_other():
    wrapped = 0
    for name, lm in models():
        wid = lm.word_ids
        cap = lm.word_table.shape[0]
        assert cap & (cap - 1) == 0 and lm.word_table.dtype == torch.int32 and lm.ngram_table.dtype == torch.int32 and lm.pool.dtype == torch.int64
        vocab = [g[0] for g in lm.ngrams[0] if not isinstance(g[0], str)]
        assert sorted(wid[w] for w in vocab) == list(range(3, 3 + len(vocab))) and (wid[UNK], wid[BOS], wid[EOS]) == (0, 1, 2)
        for w in vocab:
            got, probes = R.mirror_word_id(lm, w)
            assert got == wid[w], (name, w)
            wrapped += (R.table_hash(len(w), w) & (cap - 1)) + probes > cap
            for other in (w + (2,), w[:-1], w[:-1] + (w[-1] + 1,), (w[0] + (1 << 40),) + w[1:]):
                if other and other not in wid:
                    assert R.mirror_word_id(lm, other)[0] == 0, (name, other)
        for n, table in enumerate(lm.ngrams, 1):
            c = int(lm.meta[lm.order + n - 1])
            for g, (lp, bow) in table.items():
                key = [wid[t] for t in g]
                got, probes = R.mirror_ngram(lm, key)
                assert got is not None and got[0] == np.float32(lp) and got[1] == np.float32(bow), (name, g)
                wrapped += (R.table_hash(n, key) & (c - 1)) + probes > c
                for other in (key[:-1] + [key[-1] + 1], [key[0] + 7] + key[1:], key[::-1]):
                    spelled = tuple(next((t for t, i in wid.items() if i == k), None) for k in other)
                    if spelled not in table:
                        assert R.mirror_ngram(lm, other)[0] is None, (name, g, other)
    assert wrapped >= 3                                  # table_bits: some chains run past the table's end and go on at slot 0


def test_capacities():
    lm, _ = R.fit_model(11, 3)
    entries = [len(t) for t in lm.ngrams]
    for n, e in enumerate(entries):
        c = int(lm.meta[lm.order + n])
        assert 2 * e <= c < 4 * e                        # load <= 1/2, and no more than the next power of two
    vocab = sum(not isinstance(g[0], str) for g in lm.ngrams[0])
    assert 2 * vocab <= lm.word_table.shape[0] < 4 * vocab
    full, _ = R.fit_model(11, 3, table_bits=0)
    for n, e in enumerate(entries):
        c = int(full.meta[lm.order + n])
        assert e <= c < 2 * e
    assert list(full.meta[:3]) == [0, int(full.meta[3]) * 3, int(full.meta[3]) * 3 + int(full.meta[4]) * 4]
    assert full.ngram_table.numel() == sum(int(full.meta[3 + n]) * (n + 3) for n in range(3))


def test_unknown_words():
    listed = WordNGramLM.from_arpa(R.ARPA_UNK, R.SYMBOLS).compile()            # <unk> is listed: no unk_logp is needed, its entries are used
    ln10 = math.log(10.0)
    assert listed.ngrams[0][(UNK,)] == (-1.2 * ln10, -0.31 * ln10)
    got, _ = R.mirror_ngram(listed, [listed.word_ids[tuple(R.spell("the"))], 0])
    assert got[0] == np.float32(-0.7 * ln10)
    with pytest.raises(ValueError, match="unk_logp"):
        WordNGramLM.from_arpa(R.ARPA_BOS, R.SYMBOLS).compile()
    lm = WordNGramLM.from_arpa(R.ARPA_BOS, R.SYMBOLS, unk_logp=-7.5).compile()
    assert lm.ngrams[0][(UNK,)] == (-7.5, 0.0) and R.mirror_ngram(lm, [0])[0] == (np.float32(-7.5), np.float32(0.0))
    emu, cat = tuple(R.spell("emu")), tuple(R.spell("cat"))
    assert lm.log_prob((BOS,), emu) == -0.4 * ln10 + -7.5 and lm.log_prob((BOS, emu), cat) == -0.9 * ln10       # (<unk>) has no weight
    for word in ((10 ** 12, 5), (-5,), (29, 30), (2 ** 40 + 3,)):               # ids outside the symbol range: unknown, never an index
        assert lm.token(word) == UNK and R.mirror_word_id(lm, word)[0] == 0
    with pytest.raises(RuntimeError, match="compile"):
        WordNGramLM.from_arpa(R.ARPA_BOS, R.SYMBOLS).to("cpu")


def test_the_oracle_scores_a_sentence_by_hand():
    lm, (ids, lens, scores) = R.flip_case()
    ln10 = math.log(10.0)
    ref = R.oracle(lm, ids, lens, scores, lm_weight=0.5, word_bonus=0.25)
    right = (-0.25 - 0.5 - 0.65) * ln10 + (-0.8) * ln10                                      # <s> the, the cat, cat sat, then sat -> </s> backs off
    wrong = -0.25 * ln10 + (-0.3 * ln10 - 7.5) + (-1.4 * ln10) + (-0.8 * ln10)               # the -> <unk> backs off, <unk> -> sat, sat -> </s>
    assert ref["order"].tolist() == [[1, 0]] and ref["n_words"].tolist() == [[3, 3]] and ref["n_oov"].tolist() == [[0, 1]]
    assert ref["word_lm_scores"][0] == pytest.approx([right, wrong], rel=1e-14)
    assert ref["scores"][0] == pytest.approx([-10.25 + 0.5 * right + 0.75, -10.0 + 0.5 * wrong + 0.75], rel=1e-14)
    assert R.oracle(lm, ids, lens, scores, lm_weight=0.0)["order"].tolist() == [[0, 1]]
    assert R.split_words([1, 1, 5, 6, 1, 1, 7, 1, 9], 8, 1) == [(5, 6), (7,)] and R.split_words([1, 1], 2, 1) == [] == R.split_words([5], 0, 1)


def test_case_list_is_well_separated():
    """adjacent keys of an utterance differ by more than four times the bound, or are exact ties of a duplicated hypothesis with an equal
    first-pass score: then a device within the bound must give the oracle's order, with no case left out"""
    names, ties = set(), 0
    for name, lm, ids, lens, scores, kw in R.case_list():
        assert name not in names and ids.dtype == np.int64 and lens.dtype == np.int32 and scores.dtype == np.float32
        names.add(name)
        ref = R.oracle(lm, ids, lens, scores, **kw)
        assert R.well_separated(ref, ids, lens, scores) == [], name
        present = np.isfinite(ref["scores"])
        ties += int(np.sum((ref["scores"][:, 1:] == ref["scores"][:, :-1]) & present[:, 1:]))
        assert np.all(np.isfinite(ref["word_lm_scores"])) and np.all(ref["bound_lm"][present] < 1e-3)
    assert ties >= 2 and len(names) >= 15
    lm, (ids, lens, scores) = R.flip_case()
    for w in (0.5, 0.0):
        assert R.well_separated(R.oracle(lm, ids, lens, scores, lm_weight=w), ids, lens, scores) == []


def test_pipelines_refuse_a_word_model_without_a_beam():
    from voice100_amd.infer import ASRPipeline, LongASRPipeline
    lm = WordNGramLM.from_arpa(R.ARPA_UNK, R.SYMBOLS).compile()
    for make in (lambda **kw: ASRPipeline(None, **kw), lambda **kw: LongASRPipeline(None, **kw)):
        with pytest.raises(RuntimeError) as word:
            make(word_lm=lm)
        with pytest.raises(RuntimeError) as char:
            make(lm=object())
        assert str(word.value) == str(char.value) and "beam_size" in str(word.value)
        p = make(word_lm=lm, beam_size=8)
        p = getattr(p, "asr", p)
        assert p.rescore_size == 8 and p.word_lm is lm and p.word_lm_weight == 0.5 and p.word_bonus == 0.0 and p.sep == 1
        assert getattr(make(beam_size=8), "asr", make(beam_size=8)).word_lm is None
    with pytest.raises(RuntimeError, match="rescore_size"):
        ASRPipeline(None, beam_size=8, word_lm=lm, rescore_size=9)
    with pytest.raises(RuntimeError, match="rescore_size"):
        ASRPipeline(None, beam_size=8, nbest=4, word_lm=lm, rescore_size=2)


def test_rescore_nbest_refuses_cpu_tensors_and_uncompiled_models():
    from voice100_amd.decode import rescore_nbest
    lm, (ids, lens, scores) = R.flip_case()
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        rescore_nbest(torch.from_numpy(ids), torch.from_numpy(lens), torch.from_numpy(scores), lm)
