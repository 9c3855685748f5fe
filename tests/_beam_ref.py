"""Host oracle for the CTC prefix beam search tests (K24), written from the definition, not from the code under test, in float64:

    lp[t] = log_softmax(x[t]); the beam maps a label prefix (a tuple of ids) to (pb, pnb), the log probability of all alignments of the
    frames so far that collapse to the prefix and end in blank / in a label; start {(): (0, -inf)}.  Per frame, for every prefix p with
    last label e and tot = logaddexp(pb, pnb):
        stay    p:        pb' (+)= tot + lp[blank];  pnb' (+)= pnb + lp[e]  (p non-empty)
        extend  p + (c,): pnb' (+)= (pb if c == e else tot) + lp[c]         (every c != blank)
    contributions to the same prefix merge; probability zero is dropped; the W highest totals are the next beam.

Prefixes are identified through a dictionary keyed by the id tuples.  An extension can only coincide with a prefix that is itself in the
beam (two different beam entries never extend to the same prefix), so per frame the dictionary is asked once per beam entry whether its
parent is in the beam, and the scores are numpy rows.

beam_search is the plain recursion.  beam_search_fork follows every way of breaking a near-tie at the beam's edge: with
thr = rel * max(1, |score of rank W|), candidates above (rank W+1) + thr are kept, candidates below (rank W) - thr are dropped, and every
way of filling the remaining places from those in between is followed to the end; each leaf is a sorted final beam.  More than
MAX_LEAVES leaves: the case is undecided (None).  accept() says whether a device result equals some leaf.

REL = 2e-5: a numpy float32 run of the same recursion differs from the float64 one by <= 3.3e-7 relative at T <= 100 (host
measurement), 2e-5 is 60 x that; the device's own worst relative score difference over the seeded cases is recorded in
profiles/beam_bench.json (score_rel_err_max) and REL must be at least 8 x that figure.

ctc_loglik is the exact CTC log-likelihood of a label sequence (forward recursion); brute_force sums all V^T alignments."""
import functools
import itertools
import math

import numpy as np

REL = 2e-5
MAX_LEAVES = 64
TOL = 1e-4                                               # the project's bound on reported scores: TOL * max(1, |score|)

# (T, V, W, scale, nbest, cases): logits standard_normal((cases, T, V)) * scale in float32 from default_rng(1000 T + 10 V + W)
SHAPES = [(24, 8, 4, 3, 4, 16), (33, 29, 8, 3, 4, 16), (64, 29, 16, 3, 4, 8), (20, 71, 16, 4, 4, 8), (40, 29, 3, 3, 3, 16),
          (48, 29, 1, 3, 1, 16), (31, 65, 17, 3, 4, 6), (16, 128, 64, 3, 4, 2), (24, 64, 64, 3, 4, 2), (300, 8, 4, 3, 4, 4),
          (40, 2, 8, 2, 4, 8), (24, 3, 5, 2, 4, 8), (12, 3, 64, 1, 4, 4), (1, 29, 8, 3, 4, 8), (2, 29, 8, 3, 8, 8)]


def seeded_logits(T, V, W, scale, cases):
    rng = np.random.default_rng(1000 * T + 10 * V + W)
    return (rng.standard_normal((cases, T, V)) * scale).astype(np.float32)


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def _frame(beam, lp, blank):
    """beam [(prefix, pb, pnb)] and one frame -> (order, tot, make): the candidates of probability > 0 by falling total (stable),
    their totals, and make(indices) -> the beam of those candidates."""
    nb, V = len(beam), len(lp)
    index = {p: i for i, (p, _, _) in enumerate(beam)}
    pb = np.array([e[1] for e in beam], dtype=np.float64)
    pnb = np.array([e[2] for e in beam], dtype=np.float64)
    last = np.array([e[0][-1] if e[0] else -1 for e in beam], dtype=np.int64)
    with np.errstate(all="ignore"):
        tot = np.logaddexp(pb, pnb)
        spb = tot + lp[blank]
        spnb = np.where(last >= 0, pnb + lp[np.maximum(last, 0)], -np.inf)
        ext = tot[:, None] + lp[None, :]
        rows = np.nonzero(last >= 0)[0]
        ext[rows, last[rows]] = pb[rows] + lp[last[rows]]
        ext[:, blank] = -np.inf
        for i, (q, _, _) in enumerate(beam):             # q = parent + (c,) with the parent in the beam: that extension IS q
            if q and q[:-1] in index:
                k, c = index[q[:-1]], q[-1]
                spnb[i] = np.logaddexp(spnb[i], ext[k, c])
                ext[k, c] = -np.inf
        alltot = np.concatenate([np.logaddexp(spb, spnb), ext.ravel()])
    valid = np.nonzero(alltot > -np.inf)[0]
    order = valid[np.argsort(-alltot[valid], kind="stable")]

    def make(indices):
        out = []
        for i in indices:
            i = int(i)
            if i < nb:
                out.append((beam[i][0], spb[i], spnb[i]))
            else:
                k, c = divmod(i - nb, V)
                out.append((beam[k][0] + (c,), -np.inf, alltot[i]))
        return out
    return order, alltot, make


def _final(beam):
    with np.errstate(all="ignore"):
        out = [(p, float(np.logaddexp(a, b))) for p, a, b in beam]
    out.sort(key=lambda e: -e[1])                        # stable: ties keep beam order
    return out


def beam_search(x, W, blank=0):
    """The plain recursion on logits x [n, V]: the final beam [(prefix, total)], best first."""
    lps = log_softmax(x) if len(x) else np.zeros((0, 1))
    beam = [((), 0.0, -np.inf)]
    for lp in lps:
        order, _, make = _frame(beam, lp, blank)
        beam = make(order[:W])
    return _final(beam)


class _Undecided(Exception):
    pass


def beam_search_fork(x, W, blank=0, rel=REL, max_leaves=MAX_LEAVES):
    """Every final beam that a search with ties broken either way within rel can end in; None = undecided (too many)."""
    lps = log_softmax(x) if len(x) else np.zeros((0, 1))
    leaves = []

    def run(beam, t):
        while t < len(lps):
            order, tot, make = _frame(beam, lps[t], blank)
            t += 1
            if len(order) <= W:
                beam = make(order)
                continue
            s = tot[order]
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
        leaves.append(_final(beam))
        if len(leaves) > max_leaves:
            raise _Undecided

    try:
        run([((), 0.0, -np.inf)], 0)
    except _Undecided:
        return None
    return leaves


def accept(leaves, hyps, scores, rel=REL, tol=TOL):
    """hyps: the device's hypotheses (tuples of ids), best first, scores: theirs; -inf marks "no hypothesis".  True iff for some leaf
    the count is right, every score is within tol * max(1, |score|) of the leaf's at the same rank, and the ids equal the leaf's rank
    by rank up to the leaf's first pair of adjacent scores closer than rel * max(1, |score|).  Also returns the worst relative score
    difference against the best-matching leaf."""
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
        err = max([abs(scores[r] - leaf[r][1]) / max(1.0, abs(leaf[r][1])) for r in range(m)], default=0.0)
        best_err = min(best_err, err)
    return best_err <= tol, best_err


def ctc_loglik(lp, labels, blank=0):
    """log p(labels | frames) of the CTC model: the forward recursion over the blank-extended labels, float64."""
    lp = np.asarray(lp, dtype=np.float64)
    ext = [blank]
    for c in labels:
        ext += [int(c), blank]
    S = len(ext)
    if len(lp) == 0:
        return 0.0 if not labels else -math.inf
    ext = np.array(ext, dtype=np.int64)
    skip = np.zeros(S, dtype=bool)                       # s - 2 -> s: between two different labels
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    a = np.full(S, -np.inf)
    a[0] = lp[0][blank]
    if S > 1:
        a[1] = lp[0][ext[1]]
    with np.errstate(all="ignore"):
        for t in range(1, len(lp)):
            one = np.concatenate([[-np.inf], a[:-1]])
            two = np.where(skip, np.concatenate([[-np.inf, -np.inf], a[:-2]]), -np.inf)
            a = np.logaddexp(np.logaddexp(a, one), two) + lp[t][ext]
        return float(np.logaddexp(a[S - 1], a[S - 2]) if S > 1 else a[0])


def brute_force(lp, blank=0):
    """{prefix: log probability} summed over all V^T alignments (tiny T and V only)."""
    lp = np.asarray(lp, dtype=np.float64)
    T, V = lp.shape
    acc = {}
    for path in itertools.product(range(V), repeat=T):
        out, prev = [], None
        for c in path:
            if c != prev and c != blank:
                out.append(c)
            prev = c
        acc.setdefault(tuple(out), []).append(sum(lp[t][c] for t, c in enumerate(path)))
    with np.errstate(all="ignore"):
        return {p: float(np.logaddexp.reduce(v)) for p, v in acc.items()}


@functools.lru_cache(maxsize=None)
def seeded_case(shape_index, blank=0):
    """(logits [cases, T, V] float32, [leaves or None per case]) of one seeded shape: computed once per process."""
    T, V, W, scale, _, cases = SHAPES[shape_index]
    x = seeded_logits(T, V, W, scale, cases)
    return x, [beam_search_fork(x[i], W, blank) for i in range(cases)]
