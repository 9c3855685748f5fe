"""The float64 oracle of decode.rescore_nbest (K34), a numpy mirror of the compiled tables' lookups, and the case list.

The oracle never touches the hash tables: the words come from a plain Python split, the probabilities from WordNGramLM.log_prob over the
dictionaries, the key and a stable sort from Python.  The mirror restates what csrc/rescore.hip does with a table (hash, probe at most
one lap, verify) and serves tests/test_rescore_cpu.py's check of compile() alone.

THE ERROR BOUND, derived, not tuned.  The tables hold the float32 roundings of the float64 values (relative error 2^-24 each); the
device adds them in fp64 (2^-53 per addition: nothing next to 2^-24) and stores the sum as fp32 (another 2^-24 of the value).  With
A = the sum of |log p| and |back-off weight| over the terms a hypothesis uses, word_lm_scores is therefore within
2^-24 (A + |value|) of the oracle; the bound asked for is twice that, BOUND_LM = 2^-23 (A + |value|).  scores = first + lm_weight * lm +
word_bonus * words in fp64 from an exact fp32 `first` and an exact integer, stored as fp32: its error is 2^-24 (|lm_weight| A + |value|),
and the bound is the same form over its three terms, BOUND_SCORE = 2^-23 (|first| + |lm_weight| A + |word_bonus| words + |value|)."""
import math

import numpy as np

from voice100_amd.lm import MAX_ORDER, WordNGramLM

EPS = 2.0 ** -23
SEP = 1


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------
def split_words(row, n, sep):
    """The words of row[:n]: maximal runs of ids != sep, as tuples of Python ints."""
    out, cur = [], []
    for x in row[:n]:
        x = int(x)
        if x == sep:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(x)
    if cur:
        out.append(tuple(cur))
    return out


def walk_abs(lm, history, tok):
    """The sum of |log p| and |back-off weight| over the terms that the back-off walk for tok after history uses (tokens, not words)."""
    ctx = tuple(history)[-(lm.order - 1):] if lm.order > 1 else ()
    a = 0.0
    while True:
        hit = lm.ngrams[len(ctx)].get(ctx + (tok,))
        if hit is not None:
            return a + abs(hit[0])
        if not ctx:
            return a
        own = lm.ngrams[len(ctx) - 1].get(ctx)
        if own is not None:
            a += abs(own[1])
        ctx = ctx[1:]


def score_hypothesis(lm, row, n, sep, use_eos):
    """(log p of the word model, A, words, unknown words) of one hypothesis, float64."""
    words = split_words(row, n, sep)
    hist = list(lm.start_history())
    total, a = 0.0, 0.0
    for w in words:
        total += lm.log_prob(hist, w)
        a += walk_abs(lm, [lm.token(h) for h in hist], lm.token(w))
        hist.append(w)
    if use_eos and lm.has_eos:
        total += lm.log_prob_eos(hist)
        a += walk_abs(lm, [lm.token(h) for h in hist], lm.EOS)
    return total, a, len(words), sum(lm.token(w) == lm.UNK for w in words)


def oracle(lm, ids, lens, scores, lm_weight=0.5, word_bonus=0.0, sep=SEP, use_eos=True):
    """ids [B, nbest, T], lens, scores as numpy arrays -> dict of [B, nbest] arrays by rank: order (int), scores, word_lm_scores,
    bound_score, bound_lm (float64), n_words, n_oov (int); absent hypotheses (first-pass score -inf) last, in their order."""
    B, nbest, T = ids.shape
    out = {k: np.zeros((B, nbest), dtype=np.float64) for k in ("scores", "word_lm_scores", "bound_score", "bound_lm")}
    out.update({k: np.zeros((B, nbest), dtype=np.int64) for k in ("order", "n_words", "n_oov")})
    for b in range(B):
        rows = []
        for j in range(nbest):
            f = float(scores[b, j])
            if not f > -math.inf:
                rows.append((1, 0.0, j, -math.inf, 0.0, 0.0, 0.0, 0, 0))
                continue
            n = min(max(int(lens[b, j]), 0), T)
            lp, a, nw, oov = score_hypothesis(lm, ids[b, j], n, sep, use_eos)
            key = f + lm_weight * lp + word_bonus * nw
            rows.append((0, -key, j, key, lp, EPS * (abs(f) + abs(lm_weight) * a + abs(word_bonus) * nw + abs(key)), EPS * (a + abs(lp)), nw, oov))
        rows.sort(key=lambda r: r[:3])                   # present first, a greater key first, the first-pass index last
        for r, row in enumerate(rows):
            out["order"][b, r], out["scores"][b, r], out["word_lm_scores"][b, r] = row[2], row[3], row[4]
            out["bound_score"][b, r], out["bound_lm"][b, r], out["n_words"][b, r], out["n_oov"][b, r] = row[5], row[6], row[7], row[8]
    return out


def well_separated(ref, ids, lens, scores):
    """The condition on the inputs that makes the ranking comparison exact: adjacent keys of an utterance differ by more than four times
    the bound, or are exact ties of a duplicated hypothesis with an equal first-pass score.  Returns the offending (b, r) pairs."""
    bad = []
    B, nbest = ref["order"].shape
    for b in range(B):
        for r in range(nbest - 1):
            i, j = int(ref["order"][b, r]), int(ref["order"][b, r + 1])
            if not scores[b, j] > -math.inf:
                break
            gap = ref["scores"][b, r] - ref["scores"][b, r + 1]
            if gap > 4.0 * max(ref["bound_score"][b, r], ref["bound_score"][b, r + 1]):
                continue
            ni, nj = int(lens[b, i]), int(lens[b, j])
            if not (gap == 0.0 and scores[b, i] == scores[b, j] and ni == nj and np.array_equal(ids[b, i, :ni], ids[b, j, :nj])):
                bad.append((b, r))
    return bad


# ---- the mirror of the table lookups (for testing compile() alone) ----------------------------------------------------------------------
_M64 = (1 << 64) - 1


def table_hash(count, elements):
    h = (count * 0xD6E8FEB86659FD93) & _M64
    for v in elements:
        h = ((h ^ (int(v) & _M64)) * 0x9E3779B97F4A7C15) & _M64
        h ^= h >> 29
    return (h ^ (h >> 32)) & 0xFFFFFFFF


def mirror_word_id(lm, word):
    """(word id, probes) as the kernel finds it in lm.word_table / lm.pool: 0 (<unk>) after an empty slot or one lap."""
    tab, pool = lm.word_table.numpy(), lm.pool.numpy()
    cap = tab.shape[0]
    slot = table_hash(len(word), word) & (cap - 1)
    for probe in range(cap):
        wid, off, n = (int(v) for v in tab[slot, :3])
        if wid < 0:
            return 0, probe + 1
        if n == len(word) and 0 <= off <= lm.pool_len - n and tuple(int(v) for v in pool[off:off + n]) == tuple(word):
            return wid, probe + 1
        slot = (slot + 1) & (cap - 1)
    return 0, cap


def mirror_ngram(lm, key):
    """((log p, back-off weight) as float32, probes) of the n-gram of word ids `key` in lm.ngram_table, or (None, probes)."""
    n = len(key)
    ng, meta = lm.ngram_table.numpy(), lm.meta
    off, cap = int(meta[n - 1]), int(meta[lm.order + n - 1])
    tab = ng[off:off + cap * (n + 2)].reshape(cap, n + 2)
    slot = table_hash(n, key) & (cap - 1)
    for probe in range(cap):
        if tab[slot, 0] < 0:
            return None, probe + 1
        if tuple(int(v) for v in tab[slot, :n]) == tuple(key):
            v = tab[slot, n:].view(np.float32)
            return (v[0], v[1]), probe + 1
        slot = (slot + 1) & (cap - 1)
    return None, cap


# ---- models ---------------------------------------------------------------------------------------------------------------------------
SYMBOLS = ["", " "] + list("abcdefghijklmnopqrstuvwxyz'")          # id -> character: blank 0, space 1, then 27 letters (V = 29)
LONG_WORD = tuple(2 + (i * 7) % 27 for i in range(70))               # a vocabulary word of more than 64 labels


def lexicon(rng, size, longest=6):
    words = set()
    while len(words) < size:
        words.add(tuple(int(x) for x in rng.integers(2, 29, size=int(rng.integers(1, longest + 1)))))
    return sorted(words)


def sentences(rng, lex, count, longest=7):
    return [[lex[int(i)] for i in rng.integers(0, len(lex), size=int(rng.integers(1, longest + 1)))] for _ in range(count)]


def join(words, sep=SEP):
    out = []
    for k, w in enumerate(words):
        out += ([sep] if k else []) + list(w)
    return out


def fit_model(seed, order, size=24, count=60, extra=(), unk_logp=-9.0, table_bits=None):
    """(compiled model, its lexicon): WordNGramLM.fit on `count` random sentences over a random lexicon (plus the `extra` words)."""
    rng = np.random.default_rng(seed)
    lex = sorted(set(lexicon(rng, size)) | set(extra))
    lm = WordNGramLM.fit([join(s) for s in sentences(rng, lex, count)] + [join([w]) for w in extra], SEP, order, unk_logp=unk_logp)
    return lm.compile(table_bits), lex


ARPA_UNK = """\\data\\
ngram 1=6
ngram 2=6
ngram 3=2

\\1-grams:
-1.2\t<unk>\t-0.31
-0.9\tthe\t-0.25
-1.1\tcat\t0.125
-1.3\tsat\t-0.2
-1.0\ton\t-0.15
-2.0\tit's

\\2-grams:
-0.4\tthe cat\t-0.11
-0.7\tthe <unk>\t-0.05
-0.6\tcat sat
-0.5\t<unk> sat\t-0.21
-0.8\tsat on
-0.3\ton the

\\3-grams:
-0.2\tthe cat sat
-0.35\tthe <unk> sat

\\end\\
"""                                                      # lists <unk> (and n-grams that name it); neither <s> nor </s>; a positive back-off

ARPA_BOS = """\\data\\
ngram 1=5
ngram 2=4

\\1-grams:
-99\t<s>\t-0.4
-0.8\t</s>
-0.7\tthe\t-0.3
-0.9\tcat\t-0.2
-1.4\tsat

\\2-grams:
-0.25\t<s> the
-0.5\tthe cat
-0.45\tcat </s>
-0.65\tcat sat

\\end\\
"""                                                      # <s> and </s>, no <unk>: compile() installs unk_logp


def spell(text):
    """A text as ids through SYMBOLS."""
    idx = {s: i for i, s in enumerate(SYMBOLS) if i}
    return [idx[c] for c in text]


def arpa_model(text, unk_logp=None, table_bits=None):
    return WordNGramLM.from_arpa(text, SYMBOLS, sep=SEP, blank=0, unk_logp=unk_logp).compile(table_bits)


# ---- the case list ----------------------------------------------------------------------------------------------------------------------
def pack(rows, scores, T=None, rng=None, lens=None):
    """rows [B][nbest] of id lists (None: an absent hypothesis) -> (ids, lens, scores); what lies beyond a length is junk, not padding:
    nothing there may be read."""
    B, nbest = len(rows), len(rows[0])
    T = T or max([1] + [len(r) for u in rows for r in u if r is not None])
    rng = rng or np.random.default_rng(7)
    ids = rng.integers(2, 29, size=(B, nbest, T)).astype(np.int64)
    ln = np.zeros((B, nbest), dtype=np.int32)
    sc = np.array(scores, dtype=np.float32).reshape(B, nbest)
    for b in range(B):
        for j, r in enumerate(rows[b]):
            if r is None:
                sc[b, j] = -np.inf
                ids[b, j] = 0
                continue
            ids[b, j, :len(r)] = r
            ln[b, j] = len(r)
    if lens is not None:
        ln = np.array(lens, dtype=np.int32).reshape(B, nbest)
    return ids, ln, sc


def first_scores(rng, B, nbest):
    """Falling first-pass scores, as a beam search gives them, a few tenths apart."""
    return -np.cumsum(rng.uniform(0.2, 0.9, size=(B, nbest)), axis=1) - rng.uniform(5, 40, size=(B, 1))


def random_rows(rng, lex, B, nbest, longest=7, oov=0.15):
    rows = []
    for _ in range(B):
        u = []
        for _ in range(nbest):
            words = [tuple(int(x) for x in rng.integers(2, 29, size=int(rng.integers(1, 5)))) if rng.random() < oov else lex[int(rng.integers(0, len(lex)))]
                     for _ in range(int(rng.integers(0, longest + 1)))]
            u.append(join(words))
        rows.append(u)
    return rows


_CASES = None


def case_list():
    """[(name, model, ids, lens, scores, keyword arguments of rescore_nbest)], built once; every case is small."""
    global _CASES
    if _CASES is not None:
        return _CASES
    cases = []

    def add(name, lm, packed, **kw):
        cases.append((name, lm, packed[0], packed[1], packed[2], kw))

    one = [(5,), (6,), (7,)]                              # single-label words: 2 k - 1 labels hold k words
    m3, lex3 = fit_model(11, 3, extra=(LONG_WORD,) + tuple(one))
    m1, lex1 = fit_model(12, 1)
    m8, lex8 = fit_model(13, MAX_ORDER, size=6, count=80)
    m3full, _ = fit_model(11, 3, extra=(LONG_WORD,) + tuple(one), table_bits=0)
    unk, bos = arpa_model(ARPA_UNK), arpa_model(ARPA_BOS, unk_logp=-7.5)
    rng = np.random.default_rng(2024)

    add("B = 1, nbest = 1", m3, pack([[join(lex3[:3])]], [-12.5]))
    rows = random_rows(rng, lex3, 2, 64)
    rows[1][54:] = [None] * 10                            # absent hypotheses at the end of a row
    add("nbest = 64 on 16 waves, absent tail", m3, pack(rows, first_scores(rng, 2, 64), rng=rng), lm_weight=0.7, word_bonus=0.3)
    a, b_, c = lex3[0], lex3[1], lex3[2]
    add("empty, separators only, leading / trailing / doubled separators", m3,
        pack([[[], [SEP], [SEP, SEP, SEP], [SEP] + join([a, b_]), join([a, b_]) + [SEP], list(a) + [SEP, SEP] + list(b_),
               [SEP, SEP] + join([a, b_, c]) + [SEP, SEP], join([a, b_, c])]], first_scores(rng, 1, 8), rng=rng), lm_weight=0.4, word_bonus=-0.2)
    w62, w3 = tuple([9] * 62), (10, 11, 12)
    add("63, 64 and 65 labels; a word across positions 63 / 64; words of more than 64 labels", m3,
        pack([[join([one[k % 3] for k in range(32)]), join([one[k % 3] for k in range(32)]) + [SEP], join([one[k % 3] for k in range(33)]),
               join([tuple([8] * 61), w3, a]), join([w62, w3]), join([a, LONG_WORD, b_]), join([LONG_WORD[:69] + (3,), c]),
               join([tuple([4] * 64), a]), join([a, tuple([4] * 63)])]], first_scores(rng, 1, 9), rng=rng))
    add("65 and 130 words: the lanes loop", m3,
        pack([[join([lex3[int(i)] if len(lex3[int(i)]) < 3 else one[int(i) % 3] for i in rng.integers(0, len(lex3), size=65)]),
               join([one[int(i)] for i in rng.integers(0, 3, size=130)]), join([one[int(i)] for i in rng.integers(0, 3, size=64)])]],
             first_scores(rng, 1, 3), rng=rng), word_bonus=0.05)
    add("order 1", m1, pack(random_rows(rng, lex1, 2, 5), first_scores(rng, 2, 5), rng=rng))
    add("order MAX_ORDER", m8, pack(random_rows(rng, lex8, 2, 7, longest=12, oov=0.05), first_scores(rng, 2, 7), rng=rng), lm_weight=0.9)
    add("sentences shorter than the order, with <s>", m8, pack([[join(lex8[:1]), join(lex8[1:3]), [], join(lex8[2:5])]],
                                                               first_scores(rng, 1, 4), rng=rng))
    add("sentences shorter than the order, without <s>; <unk> listed", unk,
        pack([[spell("cat"), spell("the cat"), spell("the dog sat"), spell("dog"), spell("it's on the cat sat"), spell("the cat sat on the dog sat on")]],
             first_scores(rng, 1, 6), rng=rng), lm_weight=1.3)
    add("a model without </s>, use_eos as it comes", unk, pack([[spell("the cat sat"), spell("on the zebra")]], [-3.0, -3.5]), use_eos=True)
    add("use_eos=False on a model with </s>", bos, pack([[spell("the cat"), spell("the cat sat"), spell("cat the")]], [-4.0, -4.25, -5.5]),
        use_eos=False)
    add("<unk> from unk_logp; unlisted contexts", bos, pack([[spell("the cat"), spell("the emu sat"), spell("emu emu"), spell("sat sat cat")]],
                                                            first_scores(rng, 1, 4), rng=rng), lm_weight=0.8)
    wild = [[3, 4, SEP, 10 ** 12, 5, SEP, 6], [-5, SEP, 29, 30], [2 ** 40 + 3, 2 ** 40 + 4], list(a) + [SEP, -(2 ** 62), SEP] + list(b_)]
    add("ids outside the symbol range", m3, pack([wild], first_scores(rng, 1, 4), rng=rng))
    add("table_bits = 0: long probe chains that wrap", m3full, pack(random_rows(rng, lex3, 2, 9, oov=0.3), first_scores(rng, 2, 9), rng=rng),
        lm_weight=0.6)
    dup = random_rows(rng, lex3, 1, 6)
    dup[0][3], dup[0][4] = list(dup[0][1]), list(dup[0][0])
    sc = first_scores(rng, 1, 6)
    sc[0, 3], sc[0, 4] = sc[0, 1], sc[0, 0]
    add("exact ties: duplicated hypotheses with equal first-pass scores", m3, pack(dup, sc, rng=rng))
    rows = random_rows(rng, lex3, 1, 4)
    T = max(len(r) for r in rows[0]) + 3
    ln = [[len(rows[0][0]), T + 9, -4, len(rows[0][3])]]  # lengths beyond the row and below zero are clamped
    add("lengths outside [0, T]", m3, pack(rows, first_scores(rng, 1, 4), T=T, rng=rng, lens=ln))
    add("a negative weight", m3, pack(random_rows(rng, lex3, 1, 6), first_scores(rng, 1, 6), rng=rng), lm_weight=-0.5, word_bonus=1.0)
    _CASES = cases
    return cases


def flip_case():
    """Two hypotheses that differ in one word; the wrong one is slightly ahead in the first pass, only the right word is in the model."""
    lm = arpa_model(ARPA_BOS, unk_logp=-7.5)
    return lm, pack([[spell("the cot sat"), spell("the cat sat")]], [-10.0, -10.25])
