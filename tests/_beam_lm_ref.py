"""Host oracle for the fused CTC prefix beam search (K25), written from the definition, in float64.

The CTC side is the recursion of tests/_beam_ref.py: the beam maps a label prefix to (pb, pnb), stays and extensions merge per prefix,
probability zero is dropped.  What changes is the ranking: a candidate prefix p is ranked by
    key(p) = logaddexp(pb, pnb) + alpha * lm(p) + beta * len(p),      lm(p) = sum_i log P(p[i] | p[:i])
and the W highest keys are the next beam.  After the last frame, with use_eos, alpha * log P(</s> | p) is added and the beam is sorted.
lm(p) is a function of the prefix alone, so merging is as exact as without an LM.

The LM comes as a LOOKUP over the full id history, not as the compiled automaton the device reads:
    BackoffLM(ngrams, order, V)   walks ARPA tables {n-gram: (logp, bow)} per order: the listed value of the longest history that has
                                  one, plus the back-off weights of the longer histories on the way.  NGramLM.compile() is therefore
                                  tested by this oracle, not trusted by it;
    AutomatonLM(logp, next, ...)  walks an arbitrary deterministic automaton from its start state along the history (the tests'
                                  random tables, which no n-gram model stands behind).

beam_search is the plain recursion, beam_search_fork follows every way of breaking a near-tie of KEYS at the beam's edge exactly as
_beam_ref.beam_search_fork does for totals (thr = rel * max(1, |key of rank W|)); a leaf is the sorted final beam
[(prefix, key, ctc, lm)].  accept() is _beam_ref.accept's rule on the keys, and also wants ctc and lm of every rank within TOL.
REL stays 2e-5: the device's own worst relative score error is recorded in profiles/beam_lm_bench.json and REL must be >= 8 x it."""
import functools
import itertools
import math

import numpy as np

from _beam_ref import MAX_LEAVES, REL, SHAPES, TOL, log_softmax

SETTINGS = [(0.5, 0.0, 37), (1.0, 1.5, 1), (2.0, -0.5, 200)]            # (alpha, beta, states of the random automaton)
# (T, V, W) of the GPU parity test; scale, nbest and the number of cases are _beam_ref.SHAPES' for the same (T, V, W), but 16 cases
# at (64, 29, 16): with 8, one undecided case would be 12.5 %
GPU_SHAPES = [(24, 8, 4), (33, 29, 8), (64, 29, 16), (20, 71, 16), (48, 29, 1), (31, 65, 17), (16, 128, 64), (300, 8, 4), (24, 3, 5),
              (1, 29, 8), (2, 29, 8)]


def shape_params(T, V, W):
    scale, nbest, cases = next(s[3:] for s in SHAPES if s[:3] == (T, V, W))
    return scale, nbest, 16 if (T, V, W) == (64, 29, 16) else cases


def seeded_logits(T, V, W):
    scale, _, cases = shape_params(T, V, W)
    rng = np.random.default_rng(1000 * T + 10 * V + W + 7)
    return (rng.standard_normal((cases, T, V)) * scale).astype(np.float32)


def random_automaton(S, V, seed, blank=0):
    """(logp [S, V] float32, next [S, V] int32, final [S] float32): every state's distribution over the non-blank labels and the end
    of the sentence sums to 1; the successors are arbitrary."""
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((S, V + 1)) * 2.0          # column V: the end of the sentence
    raw[:, blank] = -np.inf
    lp = log_softmax(raw)
    logp = lp[:, :V].copy()
    logp[:, blank] = 0.0
    nxt = rng.integers(0, S, (S, V)).astype(np.int32)
    nxt[:, blank] = np.arange(S)
    return logp.astype(np.float32), nxt, lp[:, V].astype(np.float32)


class BackoffLM:
    """P(c | history) by the ARPA rule on tables ngrams[n - 1] = {n-gram of tokens: (logp, bow)}; tokens are label ids, V for <s> and
    V + 1 for </s>."""

    def __init__(self, ngrams, order, V):
        self.ngrams, self.order, self.V = ngrams, order, V
        self.bos, self.eos = V, V + 1
        self.has_bos, self.has_eos = (V,) in ngrams[0], (V + 1,) in ngrams[0]

    def _p(self, prefix, tok):
        hist = ((self.bos,) if self.has_bos else ()) + tuple(prefix)
        hist = hist[-(self.order - 1):] if self.order > 1 else ()        # the last N - 1 tokens (all of them where there are fewer)
        total = 0.0
        for start in range(len(hist) + 1):               # from the longest history to none
            ctx = hist[start:]
            hit = self.ngrams[len(ctx)].get(ctx + (tok,))
            if hit is not None:
                return total + hit[0]
            if ctx and ctx in self.ngrams[len(ctx) - 1]:
                total += self.ngrams[len(ctx) - 1][ctx][1]
        return -math.inf

    def row(self, prefix):
        return np.array([self._p(prefix, c) for c in range(self.V)], dtype=np.float64)

    def final(self, prefix):
        return self._p(prefix, self.eos) if self.has_eos else 0.0


class AutomatonLM:
    def __init__(self, logp, nxt, final, start=0):
        self.logp, self.nxt, self.fin, self.start = np.asarray(logp, np.float64), np.asarray(nxt), np.asarray(final, np.float64), start
        self.states = {(): start}                        # the state after each prefix asked for so far

    def _state(self, prefix):
        s = self.states.get(prefix)
        if s is None:
            s = self.states[prefix] = int(self.nxt[self._state(prefix[:-1]), prefix[-1]])
        return s

    def row(self, prefix):
        return self.logp[self._state(prefix)]

    def final(self, prefix):
        return float(self.fin[self._state(prefix)])


class _Scorer:
    """lm(p) and the row log P(. | p) per prefix, each computed once."""

    def __init__(self, lm):
        self.lm, self.sums, self.rows = lm, {(): 0.0}, {}

    def row(self, p):
        r = self.rows.get(p)
        if r is None:
            r = self.rows[p] = self.lm.row(p)
        return r

    def lm_sum(self, p):
        v = self.sums.get(p)
        if v is None:
            v = self.sums[p] = self.lm_sum(p[:-1]) + float(self.row(p[:-1])[p[-1]])
        return v


def _frame(beam, lp, blank, sc, alpha, beta):
    """beam [(prefix, pb, pnb)] and one frame -> (order, key, make): the candidates of probability > 0 by falling key (stable; the
    stays first, then entry-major extensions: the device's candidate order up to the stays' places), their keys, and
    make(indices) -> the beam of those candidates."""
    nb, V = len(beam), len(lp)
    index = {p: i for i, (p, _, _) in enumerate(beam)}
    pb = np.array([e[1] for e in beam], dtype=np.float64)
    pnb = np.array([e[2] for e in beam], dtype=np.float64)
    last = np.array([e[0][-1] if e[0] else -1 for e in beam], dtype=np.int64)
    lms = np.array([sc.lm_sum(e[0]) for e in beam], dtype=np.float64)
    lens = np.array([len(e[0]) for e in beam], dtype=np.float64)
    rows = np.stack([sc.row(e[0]) for e in beam])
    with np.errstate(all="ignore"):
        tot = np.logaddexp(pb, pnb)
        spb = tot + lp[blank]
        spnb = np.where(last >= 0, pnb + lp[np.maximum(last, 0)], -np.inf)
        ext = tot[:, None] + lp[None, :]
        has = np.nonzero(last >= 0)[0]
        ext[has, last[has]] = pb[has] + lp[last[has]]
        ext[:, blank] = -np.inf
        for i, (q, _, _) in enumerate(beam):             # q = parent + (c,) with the parent in the beam: that extension IS q
            if q and q[:-1] in index:
                k, c = index[q[:-1]], q[-1]
                spnb[i] = np.logaddexp(spnb[i], ext[k, c])
                ext[k, c] = -np.inf
        stay = np.logaddexp(spb, spnb)
        ctc = np.concatenate([stay, ext.ravel()])
        key = np.concatenate([stay + alpha * lms + beta * lens,
                              (ext + alpha * (lms[:, None] + rows) + beta * (lens[:, None] + 1.0)).ravel()])
        key[~(ctc > -np.inf)] = -np.inf                  # probability zero stays no candidate, whatever the LM says
    valid = np.nonzero(key > -np.inf)[0]
    order = valid[np.argsort(-key[valid], kind="stable")]

    def make(indices):
        out = []
        for i in indices:
            i = int(i)
            if i < nb:
                out.append((beam[i][0], spb[i], spnb[i]))
            else:
                k, c = divmod(i - nb, V)
                out.append((beam[k][0] + (c,), -np.inf, ctc[i]))
        return out
    return order, key, make


def _final(beam, sc, alpha, beta, use_eos):
    out = []
    with np.errstate(all="ignore"):
        for p, a, b in beam:
            ctc = float(np.logaddexp(a, b))
            lm = sc.lm_sum(p) + (sc.lm.final(p) if use_eos else 0.0)
            out.append((p, ctc + alpha * lm + beta * len(p), ctc, lm))
    out.sort(key=lambda e: -e[1])                        # stable: ties keep beam order
    return out


def beam_search(x, W, lm, alpha, beta, blank=0, use_eos=True):
    """The plain recursion on logits x [n, V]: the final beam [(prefix, key, ctc, lm)], best first."""
    lps = log_softmax(x) if len(x) else np.zeros((0, 1))
    sc = _Scorer(lm)
    beam = [((), 0.0, -np.inf)]
    for lp in lps:
        order, _, make = _frame(beam, lp, blank, sc, alpha, beta)
        beam = make(order[:W])
    return _final(beam, sc, alpha, beta, use_eos)


class _Undecided(Exception):
    pass


def beam_search_fork(x, W, lm, alpha, beta, blank=0, use_eos=True, rel=REL, max_leaves=MAX_LEAVES):
    """Every final beam that a search with near-ties of keys broken either way can end in; None = undecided (too many)."""
    lps = log_softmax(x) if len(x) else np.zeros((0, 1))
    sc = _Scorer(lm)
    leaves = []

    def run(beam, t):
        while t < len(lps):
            order, key, make = _frame(beam, lps[t], blank, sc, alpha, beta)
            t += 1
            if len(order) <= W:
                beam = make(order)
                continue
            s = key[order]
            thr = rel * max(1.0, abs(s[W - 1]))
            keep = order[s > s[W] + thr]
            mid = order[(s <= s[W] + thr) & (s >= s[W - 1] - thr)]
            need = W - len(keep)
            if need == 0:
                beam = make(keep)
                continue
            if math.comb(len(mid), need) > max_leaves:
                raise _Undecided
            for combo in itertools.combinations(mid, need):
                run(make(list(keep) + list(combo)), t)
            return
        leaves.append(_final(beam, sc, alpha, beta, use_eos))
        if len(leaves) > max_leaves:
            raise _Undecided

    try:
        run([((), 0.0, -np.inf)], 0)
    except _Undecided:
        return None
    return leaves


def accept(leaves, hyps, scores, ctc_scores, lm_scores, rel=REL, tol=TOL):
    """_beam_ref.accept's rule on the fused scores (count, every score within tol * max(1, |score|) of the leaf's at the same rank, ids
    equal rank by rank up to the leaf's first near-tie), and ctc_scores / lm_scores within tol * max(1, |value|) of the leaf's at
    every rank.  Returns (accepted, the worst relative difference of the three scores against the best-matching leaf)."""
    best_err = math.inf
    for leaf in leaves:
        m = min(len(leaf), len(hyps))
        if any(scores[r] != -math.inf for r in range(m, len(hyps))) or any(len(hyps[r]) for r in range(m, len(hyps))):
            continue
        if any(not math.isfinite(scores[r]) for r in range(m)):
            continue
        cut = m
        for r in range(len(leaf) - 1):
            if leaf[r][1] - leaf[r + 1][1] < rel * max(1.0, abs(leaf[r][1])):
                cut = min(cut, r)
                break
        if any(tuple(hyps[r]) != leaf[r][0] for r in range(cut)):
            continue
        err = 0.0
        for r in range(m):
            # beyond the cut the ids may be another near-tied prefix' whose parts differ: there only the key is compared
            parts = [(scores[r], leaf[r][1])] + ([(ctc_scores[r], leaf[r][2]), (lm_scores[r], leaf[r][3])] if r < cut else [])
            err = max([err] + [abs(g - w) / max(1.0, abs(w)) for g, w in parts])
        best_err = min(best_err, err)
    return best_err <= tol, best_err


@functools.lru_cache(maxsize=None)
def fit_lm(V, order=3, blank=0, seed=0):
    """A `fit` model on seeded sequences with some structure (a random first-order chain), for the tests that want a real n-gram
    model: (NGramLM, BackoffLM over its tables)."""
    from voice100_amd.lm import NGramLM
    rng = np.random.default_rng(77 + V + 1000 * seed + blank)
    labels = np.array([c for c in range(V) if c != blank])
    trans = rng.dirichlet(np.full(len(labels), 0.3), size=len(labels))
    seqs = []
    for _ in range(60):
        s = [int(rng.integers(len(labels)))]
        for _ in range(int(rng.integers(3, 40))):
            s.append(int(rng.choice(len(labels), p=trans[s[-1]])))
        seqs.append([int(labels[i]) for i in s])
    lm = NGramLM.fit(seqs, V, order, blank=blank)
    return lm, BackoffLM(lm.ngrams, lm.order, V)


@functools.lru_cache(maxsize=None)
def seeded_case(shape_index, setting_index, kind):
    """One cell of the GPU parity test, computed once per process: kind "automaton" (random tables of the setting's S states) or "fit"
    (an order-3 fit model).  Returns (logits [cases, T, V] float32, the LM as the device takes it: (logp, next, final, start) numpy
    tables for "automaton", the NGramLM for "fit"; [leaves or None per case])."""
    T, V, W = GPU_SHAPES[shape_index]
    alpha, beta, S = SETTINGS[setting_index]
    x = seeded_logits(T, V, W)
    if kind == "automaton":
        tables = random_automaton(S, V, 31 * S + V)
        dev, look = tables + (0,), AutomatonLM(*tables)
    else:
        dev, look = fit_lm(V)
    return x, dev, [beam_search_fork(x[i], W, look, alpha, beta) for i in range(x.shape[0])]
