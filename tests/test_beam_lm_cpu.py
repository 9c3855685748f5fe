"""CPU-side checks of the fused CTC prefix beam search (K25): the ARPA reader on a hand-written file, the estimator's normalisation and
its round trip through ARPA text, the compiled automaton against the back-off walk and a brute force over all histories, the oracle of
tests/_beam_lm_ref.py against a brute-force sum over all alignments, the share of the GPU test's cases that the forking oracle leaves
undecided, the library's prototype and host-side validation, and the wrappers' refusals without a GPU."""
import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

from _beam_lm_ref import (GPU_SHAPES, SETTINGS, AutomatonLM, BackoffLM, accept, beam_search, beam_search_fork, fit_lm, random_automaton,
                          seeded_case, shape_params)
from _beam_ref import MAX_LEAVES, REL, brute_force, log_softmax
from voice100_amd.lm import NGramLM

LN10 = math.log(10.0)
SYMBOLS = ["_", "a", "b", "c"]                           # id 0 is the blank
ARPA = """
\\data\\
ngram 1=5
ngram 2=4
ngram 3=2

\\1-grams:
-99\t<s>\t-0.5
-0.7\t</s>
-0.4\ta\t-0.3
-0.6\tb\t-0.2
-1.0\tc

\\2-grams:
-0.2\t<s> a\t-0.1
-0.5\ta b\t-0.4
-0.3\tb a
-0.9\ta </s>

\\3-grams:
-0.1\t<s> a b
-0.25\ta b a

\\end\\
"""
A, B_, C, BOS, EOS = 1, 2, 3, 4, 5


def test_arpa_reader_values_and_backoff():
    lm = NGramLM.from_arpa(ARPA, SYMBOLS)
    assert lm.order == 3 and lm.vocab_size == 4 and lm.has_bos and lm.has_eos and (lm.bos, lm.eos) == (BOS, EOS)
    assert [len(t) for t in lm.ngrams] == [5, 4, 2]
    assert lm.ngrams[0][(A,)] == (-0.4 * LN10, -0.3 * LN10) and lm.ngrams[0][(C,)] == (-1.0 * LN10, 0.0)
    assert lm.ngrams[1][(A, B_)] == (-0.5 * LN10, -0.4 * LN10) and lm.ngrams[2][(A, B_, A)] == (-0.25 * LN10, 0.0)
    close = lambda got, log10: abs(got - log10 * LN10) < 1e-12     # noqa: E731
    assert lm.start_history() == (BOS,)
    assert close(lm.log_prob((BOS,), A), -0.2)                               # listed bigram
    assert close(lm.log_prob((BOS, A), B_), -0.1)                            # listed trigram
    assert close(lm.log_prob((BOS, A), C), -0.1 + -0.3 + -1.0)               # bow(<s> a) + bow(a) + p(c)
    assert close(lm.log_prob((BOS, A, B_), A), -0.25)                        # the history is cut to the last two tokens
    assert close(lm.log_prob((A, B_), C), -0.4 + -0.2 + -1.0)
    assert close(lm.log_prob((C, C), A), -0.4)                               # unlisted contexts cost nothing
    assert close(lm.log_prob((B_, A), B_), -0.5)                             # (b a) has no back-off weight written: 0; then (a b)
    assert close(lm.log_prob_eos((BOS, A)), -0.1 + -0.9) and close(lm.log_prob_eos((C,)), -0.7)
    look = BackoffLM(lm.ngrams, 3, 4)                                        # the oracle's own walk agrees
    for hist in [(), (A,), (A, B_), (C, A, B_), (B_, B_, B_)]:
        for c in (A, B_, C):
            assert abs(look.row(hist)[c] - lm.log_prob((BOS,) + hist, c)) < 1e-12
        assert abs(look.final(hist) - lm.log_prob_eos((BOS,) + hist)) < 1e-12


def test_arpa_reader_unknown_symbols(tmp_path):
    with pytest.raises(ValueError, match="'d'"):
        NGramLM.from_arpa(ARPA, SYMBOLS + ["d"])
    lm = NGramLM.from_arpa(ARPA, SYMBOLS + ["d"], unk_logp=-5.0)
    assert lm.ngrams[0][(4,)] == (-5.0, 0.0) and lm.bos == 5
    with_unk = ARPA.replace("ngram 1=5", "ngram 1=6").replace("-1.0\tc\n", "-1.0\tc\n-2.0\t<unk>\n")
    lm = NGramLM.from_arpa(with_unk, SYMBOLS + ["d"], unk_logp=-5.0)         # <unk> wins over unk_logp
    assert lm.ngrams[0][(4,)] == (-2.0 * LN10, 0.0) and (A,) in lm.ngrams[0] and len(lm.ngrams[0]) == 6
    no_marks = "\\data\\\nngram 1=2\n\n\\1-grams:\n-0.3 a\n-0.3 b\n\n\\end\\\n"
    lm = NGramLM.from_arpa(no_marks, ["_", "a", "b"])
    assert not lm.has_bos and not lm.has_eos and lm.start_history() == () and lm.log_prob_eos(()) == 0.0
    assert NGramLM.from_arpa(no_marks, ["a", "_", "b"], blank=1).ngrams[0].keys() == {(0,), (2,)}
    path = tmp_path / "lm.arpa"                          # a path is read like the text
    path.write_text(ARPA)
    assert NGramLM.from_arpa(str(path), SYMBOLS).ngrams == NGramLM.from_arpa(ARPA, SYMBOLS).ngrams
    assert NGramLM.from_arpa(path, SYMBOLS).order == 3


@pytest.mark.parametrize("old,new,line,what", [
    ("ngram 2=4", "ngram 2=5", 20, "announces 5"),                           # count mismatch, reported where the section ends
    ("-0.5\ta b\t-0.4", "-0.5\tc b\t-0.4", 22, "context"),                    # the trigram a b a has lost its context
    ("-0.25\ta b a", "-0.25\tc c a", 22, "context"),
    ("-0.3\tb a", "-0.3\tb a x y", 17, "tokens"),
    ("-0.3\tb a", "zero\tb a", 17, "not a number"),
    ("-0.3\tb a", "0.3\tb a", 17, "log probability"),
    ("\\2-grams:", "\\3-grams:", 14, "section"),
    ("\\end\\", "", 25, "missing"),
    ("\\data\\", "\\dat\\", 2, "expected"),
    ("ngram 3=2", "ngram 4=2", 5, "order"),
    ("-0.3\tb a", "-0.3\tb a\n-0.3\tb a", 18, "twice"),
])
def test_arpa_reader_malformed(old, new, line, what):
    assert old in ARPA
    with pytest.raises(ValueError, match=f"line {line}: .*{what}"):
        NGramLM.from_arpa(ARPA.replace(old, new), SYMBOLS)


def test_arpa_reader_order_limit():
    text = "\\data\\\n" + "".join(f"ngram {n}=1\n" for n in range(1, 10))
    with pytest.raises(ValueError, match="line 10: .*limit of 8"):
        NGramLM.from_arpa(text, SYMBOLS)


def _sequences(V, blank, seed, count=40):
    rng = np.random.default_rng(seed)
    labels = [c for c in range(V) if c != blank]
    return [[labels[i] for i in rng.integers(0, len(labels), int(rng.integers(0, 12)))] for _ in range(count)]


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_fit_distributions_sum_to_one_and_survive_arpa(order):
    V, blank = 6, 2
    lm = NGramLM.fit(_sequences(V, blank, 10 + order), V, order, blank=blank)
    assert lm.order == order and lm.has_bos and lm.has_eos
    labels = [c for c in range(V) if c != blank]
    contexts = {()} | {g for t in lm.ngrams[:order - 1] for g in t if g[-1] != lm.eos}
    contexts |= {(c, d) for c in labels for d in labels}                    # and contexts the model has never seen
    for h in contexts:
        total = sum(math.exp(lm.log_prob(h, c)) for c in labels) + math.exp(lm.log_prob_eos(h))
        assert abs(total - 1.0) <= 1e-12, (h, total)
    symbols = [f"s{i}" for i in range(V)]
    back = NGramLM.from_arpa(lm.to_arpa(symbols), symbols, blank=blank)
    assert back.order == order and [t.keys() for t in back.ngrams] == [t.keys() for t in lm.ngrams]
    for h in contexts:
        for c in labels:
            assert abs(back.log_prob(h, c) - lm.log_prob(h, c)) <= 1e-6
        assert abs(back.log_prob_eos(h) - lm.log_prob_eos(h)) <= 1e-6
    with pytest.raises(ValueError):
        NGramLM.fit([[blank]], V, order, blank=blank)
    with pytest.raises(ValueError):
        NGramLM.fit([[1]], V, 9)


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_compile_against_the_backoff_walk_by_brute_force(order):
    V, blank = 4, 0
    lm = NGramLM.fit(_sequences(V, blank, 20 + order, 12), V, order).compile()
    look = BackoffLM(lm.ngrams, order, V)
    S = lm.num_states
    assert lm.logp.shape == (S, V) and lm.next.shape == (S, V) and lm.final.shape == (S,)
    assert (lm.logp.dtype, lm.next.dtype, lm.final.dtype) == (torch.float32, torch.int32, torch.float32)
    assert lm.states[0] == () and lm.states[lm.start] == ((lm.bos,) if order > 1 else ()) and len(set(lm.states)) == S
    assert S == 1 + sum(1 for t in lm.ngrams[:order - 1] for g in t if g[-1] != lm.eos)
    index = {s: i for i, s in enumerate(lm.states)}
    logp, nxt, fin = lm.logp.numpy(), lm.next.numpy(), lm.final.numpy()
    for i, s in enumerate(lm.states):                    # every state and label: the walk over the tables
        for c in range(1, V):
            assert abs(logp[i, c] - lm.log_prob(s, c)) <= 1e-6
            full = s + (c,)
            want = next(index[full[k:]] for k in range(len(full) + 1) if len(full[k:]) < order and full[k:] in index)
            assert nxt[i, c] == want, (s, c)
        assert abs(fin[i] - lm.log_prob_eos(s)) <= 1e-6 and logp[i, blank] == 0.0 and nxt[i, blank] == i
    walker = AutomatonLM(logp, nxt, fin, lm.start)       # every history up to length N: the automaton IS the back-off model
    for n in range(order + 1):
        for hist in itertools.product(range(1, V), repeat=n):
            assert np.abs(walker.row(hist)[1:] - look.row(hist)[1:]).max() <= 1e-6
            assert abs(walker.final(hist) - look.final(hist)) <= 1e-6
            full = (lm.bos,) + hist
            assert lm.states[walker._state(hist)] == next(full[k:] for k in range(len(full) + 1)
                                                          if len(full[k:]) < order and full[k:] in index)
    with pytest.raises(RuntimeError):
        NGramLM.fit([[1, 2]], V, 2).to("cpu")            # not compiled
    assert lm.to("cpu") is lm


def test_compile_a_model_without_sentence_marks():
    lm = NGramLM.from_arpa("\\data\\\nngram 1=2\nngram 2=1\n\n\\1-grams:\n-0.2 a -0.1\n-0.5 b\n\n\\2-grams:\n-0.05 a a\n\n\\end\\\n",
                           ["_", "a", "b"]).compile()
    assert lm.start == 0 and lm.states == [(), (1,), (2,)] and lm.final.tolist() == [0.0, 0.0, 0.0]
    assert np.allclose(lm.logp.numpy(), np.array([[0, -0.2, -0.5], [0, -0.05, -0.6], [0, -0.2, -0.5]]) * LN10, atol=1e-6)
    assert lm.next.tolist() == [[0, 1, 2], [1, 1, 2], [2, 1, 2]]


@pytest.mark.parametrize("T,V", [(5, 3), (6, 3), (4, 3)])
def test_oracle_is_the_brute_force_sum_plus_the_lm_term(T, V):
    lm_fit, look_fit = fit_lm(V, 3)
    tables = random_automaton(5, V, 3)
    for look in (look_fit, AutomatonLM(*tables)):
        for alpha, beta, _ in SETTINGS:
            x = (np.random.default_rng(100 * T + V).standard_normal((T, V)) * 2).astype(np.float32)
            exact = brute_force(log_softmax(x))
            final = beam_search(x, 64, look, alpha, beta)                    # W holds every prefix: nothing is pruned
            assert {p for p, _, _, _ in final} == set(exact)
            for p, key, ctc, lm in final:
                want_lm = sum(look.row(p[:i])[p[i]] for i in range(len(p))) + look.final(p)
                assert abs(ctc - exact[p]) <= 1e-12 and abs(lm - want_lm) <= 1e-12
                assert abs(key - (exact[p] + alpha * want_lm + beta * len(p))) <= 1e-12
            assert [e[1] for e in final] == sorted((e[1] for e in final), reverse=True)
            leaves = beam_search_fork(x, 64, look, alpha, beta)
            assert len(leaves) == 1 and leaves[0] == final
            cols = [[e[i] for e in final] for i in range(4)]
            assert accept(leaves, *cols) == (True, 0.0)
            assert not accept(leaves, cols[0], cols[1], [c + 1e-2 for c in cols[2]], cols[3])[0]
            assert not accept(leaves, cols[0], cols[1], cols[2], [v - 1e-2 for v in cols[3]])[0]
            no_eos = beam_search(x, 64, look, alpha, beta, use_eos=False)
            assert all(abs(dict((e[0], e[3]) for e in no_eos)[p] + look.final(p) - lm) <= 1e-12 for p, _, _, lm in final)


def test_oracle_with_a_neutral_lm_is_the_plain_oracle():
    import _beam_ref
    x = (np.random.default_rng(4).standard_normal((30, 9)) * 3).astype(np.float32)
    look = AutomatonLM(*random_automaton(7, 9, 1))
    plain = _beam_ref.beam_search(x, 5)
    fused = beam_search(x, 5, look, 0.0, 0.0, use_eos=False)
    assert [(p, k) for p, k, _, _ in fused] == plain and all(k == c for _, k, c, _ in fused)
    assert [p for p, *_ in beam_search(x, 5, look, 2.0, -0.5)] != [p for p, _ in plain]       # and a real one changes the result


@pytest.mark.parametrize("index", range(len(GPU_SHAPES)), ids=["T%d-V%d-W%d" % s for s in GPU_SHAPES])
def test_gpu_cases_are_decided(index):
    """At most 10 % of every cell of the GPU parity test may be undecided (more than MAX_LEAVES leaves)."""
    T, V, W = GPU_SHAPES[index]
    _, nbest, cases = shape_params(T, V, W)
    for setting in range(len(SETTINGS)):
        for kind in ("automaton", "fit"):
            x, _, leaves = seeded_case(index, setting, kind)
            assert x.shape == (cases, T, V) and x.dtype == np.float32
            undecided = sum(leaf is None for leaf in leaves)
            assert undecided <= 0.1 * cases, (GPU_SHAPES[index], SETTINGS[setting], kind, undecided)
            assert all(leaf is None or 1 <= len(leaf) <= MAX_LEAVES for leaf in leaves)
    assert REL == 2e-5


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


NAMES = ["logits", "lens", "ws", "ids", "ids_len", "scores", "lm_logp", "lm_next", "lm_final", "S", "start_state", "alpha", "beta",
         "use_eos", "ctc_scores", "lm_scores", "B", "T", "V", "W", "nbest", "blank", "stream"]


def test_library_exports_and_prototype(lib):
    from voice100_amd import _native as N
    protos = N.parse_header()
    assert hasattr(lib, "v100_ctc_beam_search_lm") and lib.v100_ctc_beam_search_lm.restype is ctypes.c_int
    assert [n for _, n in protos["v100_ctc_beam_search_lm"]] == NAMES
    p, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert [t for t, _ in protos["v100_ctc_beam_search_lm"]] == [p] * 9 + [i, i, f, f, i, p, p] + [i] * 6 + [p]
    assert len(protos["v100_ctc_beam_search"]) == 13     # the plain entry keeps its signature


def test_host_side_validation(lib):
    one = ctypes.c_void_p(16)                            # never dereferenced: every call below returns before any device call
    fn = lib.v100_ctc_beam_search_lm

    def call(ptrs=None, S=5, start=0, alpha=0.5, beta=0.0, shape=(2, 16, 29, 8, 1, 0)):
        a = dict.fromkeys([n for n in NAMES if n in ("logits", "lens", "ws", "ids", "ids_len", "scores", "lm_logp", "lm_next", "lm_final",
                                                      "ctc_scores", "lm_scores")], one)
        a.update(ptrs or {})
        return fn(a["logits"], a["lens"], a["ws"], a["ids"], a["ids_len"], a["scores"], a["lm_logp"], a["lm_next"], a["lm_final"], S, start,
                  alpha, beta, 1, a["ctc_scores"], a["lm_scores"], *shape, None)

    for name in ("logits", "ws", "ids", "ids_len", "scores", "lm_logp", "lm_next", "lm_final", "ctc_scores", "lm_scores"):
        assert call({name: None}) == 3, name             # lens may be NULL, the others may not
    assert call({"logits": None}, S=0) == 3              # a NULL pointer is reported before the shape
    for shape in ((0, 16, 29, 8, 1, 0), (2, 0, 29, 8, 1, 0), (2, 4097, 29, 8, 1, 0), (2, 16, 1, 8, 1, 0), (2, 16, 129, 8, 1, 0),
                  (2, 16, 29, 0, 1, 0), (2, 16, 29, 65, 1, 0), (2, 16, 29, 8, 0, 0), (2, 16, 29, 8, 9, 0), (2, 16, 29, 8, 1, -1),
                  (2, 16, 29, 8, 1, 29)):
        assert call(shape=shape) == 1, shape
    for kw in ({"S": 0}, {"S": -1}, {"start": 5}, {"start": -1}, {"S": (1 << 28) // 29 + 1}, {"alpha": math.inf}, {"alpha": math.nan},
               {"beta": -math.inf}, {"beta": math.nan}):
        assert call(**kw) == 1, kw


def test_wrappers_refuse_without_a_gpu():
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.decode import ctc_beam_search
    from voice100_amd.infer import ASRPipeline
    lm = NGramLM.from_tables(*random_automaton(3, 29, 0)).compile()
    assert lm.num_states == 3 and lm.start == 0
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ctc_beam_search(torch.zeros(2, 8, 29), lm=lm)
    model = AudioToTextCTC(64, 32, 29, 32).eval()
    with pytest.raises(RuntimeError, match="beam_size"):
        ASRPipeline(model, lm=lm)
    pipe = ASRPipeline(model, beam_size=4, lm=lm, lm_weight=0.7, length_bonus=0.1)
    assert (pipe.lm, pipe.lm_weight, pipe.length_bonus) == (lm, 0.7, 0.1)
    with pytest.raises(RuntimeError):
        pipe.nbest(torch.zeros(2, 64, 64))
    assert ASRPipeline(model).lm is None and ASRPipeline(model, beam_size=4).lm is None
    with pytest.raises(ValueError):
        NGramLM.from_tables(np.zeros((2, 3)), np.zeros((2, 4)), np.zeros(2))
