"""Float64 numpy oracle of decode.ctc_segment (K26): the posterior over the CTC alignments of a GIVEN transcript, reduced per label
and per word.  It follows the definitions, not the kernel: plain log-domain alpha / beta lattices over the whole utterance, the
onset and last-frame distributions written out, cumulative sums from the front.

For every boundary it also returns the margin min(|cdf(t*) - 1/2|, |cdf(t* - 1) - 1/2|), so a test can tell a decided median from a
near-tie that fp32 may put on either side.  tests/test_ctc_segment_cpu.py checks this file against an enumeration of all alignments
and against torch's ctc_loss."""
import numpy as np

NEG = -np.inf


def log_softmax(x):
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.max(x, axis=-1, keepdims=True)
        return x - (m + np.log(np.sum(np.exp(x - m), axis=-1, keepdims=True)))


def _shift(a, k):
    """a moved by k places (k > 0: towards higher states), -inf shifted in."""
    out = np.full(a.shape, NEG)
    if k > 0:
        out[k:] = a[:len(a) - k] if len(a) > k else []
    else:
        out[:len(a) + k if len(a) > -k else 0] = a[-k:]
    return out


def word_spans(labels, sep):
    """[(first, count)] of the maximal runs of labels != sep (K23's rule)."""
    out, i, n = [], 0, len(labels)
    while i < n:
        if labels[i] == sep:
            i += 1
            continue
        j = i
        while j < n and labels[j] != sep:
            j += 1
        out.append((i, j - i))
        i = j
    return out


def _median(pmf):
    """(first t with cdf(t) >= 1/2, margin, cdf) of one distribution over frames."""
    cdf = np.cumsum(pmf)
    hit = np.nonzero(cdf >= 0.5)[0]
    t = int(hit[0]) if hit.size else len(cdf) - 1
    before = cdf[t - 1] if t > 0 else 0.0
    return t, float(min(abs(cdf[t] - 0.5), abs(before - 0.5))), cdf


def segment_one(logits, labels, blank=0, sep=1):
    """One utterance: logits [T, V], labels a sequence of L ints.  Returns a dict: log_prob, feasible, and per label start, end,
    duration, log_confidence, start_margin, end_margin, onset_cdf / last_cdf [T, L]; per word (sep not None) word_first, word_count,
    word_start, word_end, word_log_confidence."""
    x = np.asarray(logits, np.float64)
    T, V = x.shape
    labels = [int(c) for c in labels]
    L = len(labels)
    S = 2 * L + 1
    res = {"feasible": False, "log_prob": NEG, "start": np.zeros(L, np.int64), "end": np.zeros(L, np.int64),
           "duration": np.zeros(L), "log_confidence": np.full(L, NEG), "start_margin": np.full(L, 0.5), "end_margin": np.full(L, 0.5),
           "onset_cdf": np.zeros((T, L)), "last_cdf": np.zeros((T, L)), "numerator": np.zeros(L)}

    def finish():
        if sep is not None:
            spans = word_spans(labels, sep)
            res["word_first"] = np.array([f for f, _ in spans], np.int64)
            res["word_count"] = np.array([c for _, c in spans], np.int64)
            res["word_start"] = np.array([res["start"][f] for f, _ in spans], np.int64)
            res["word_end"] = np.array([res["end"][f + c - 1] for f, c in spans], np.int64)
            res["word_start_margin"] = np.array([res["start_margin"][f] for f, _ in spans])
            res["word_end_margin"] = np.array([res["end_margin"][f + c - 1] for f, c in spans])
            wl = []
            for f, c in spans:
                d = res["duration"][f:f + c].sum()
                wl.append(res["numerator"][f:f + c].sum() / d if res["feasible"] and d > 0 else NEG)
            res["word_log_confidence"] = np.array(wl, np.float64)
        return res

    if T == 0:
        if L == 0:
            res["feasible"], res["log_prob"] = True, 0.0
        return finish()
    if any(c == blank or c < 0 or c >= V for c in labels):
        return finish()
    lp = log_softmax(x)
    z = np.full(S, blank, np.int64)
    z[1::2] = labels
    em = lp[:, z]                                        # [T, S]
    skip = np.zeros(S, bool)                             # the +2 transition INTO s
    for s in range(3, S, 2):
        skip[s] = z[s] != z[s - 2]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        alpha = np.full((T, S), NEG)
        enter = np.full((T, S), NEG)                     # log e_t(s)
        alpha[0, 0] = em[0, 0]
        enter[0, 0] = 0.0
        if S > 1:
            alpha[0, 1] = em[0, 1]
            enter[0, 1] = 0.0
        for t in range(1, T):
            a = alpha[t - 1]
            enter[t] = np.logaddexp(_shift(a, 1), np.where(skip, _shift(a, 2), NEG))
            alpha[t] = em[t] + np.logaddexp(a, enter[t])
        logp = np.logaddexp(alpha[T - 1, S - 1], alpha[T - 1, S - 2]) if S > 1 else alpha[T - 1, S - 1]
        if not np.isfinite(logp):
            if np.isnan(logp):
                res["log_prob"] = np.nan
            return finish()
        beta = np.full((T, S), NEG)
        leave = np.full((T, S), NEG)                     # log o_t(s)
        beta[T - 1, S - 1] = leave[T - 1, S - 1] = 0.0
        if S > 1:
            beta[T - 1, S - 2] = leave[T - 1, S - 2] = 0.0
        skip_out = np.zeros(S, bool)                         # the +2 transition OUT of s
        skip_out[:max(S - 2, 0)] = skip[2:]
        for t in range(T - 2, -1, -1):
            bt = em[t + 1] + beta[t + 1]
            leave[t] = np.logaddexp(_shift(bt, -1), np.where(skip_out, _shift(bt, -2), NEG))
            beta[t] = np.logaddexp(bt, leave[t])
        gamma = np.exp(alpha + beta - logp)
        onset = np.exp(enter + em + beta - logp)
        last = np.exp(alpha + leave - logp)
        gamma, onset, last = (np.where(np.isnan(v), 0.0, v) for v in (gamma, onset, last))
    res["feasible"], res["log_prob"] = True, float(logp)
    for i in range(L):
        s = 2 * i + 1
        g = gamma[:, s]
        res["duration"][i] = g.sum()
        res["numerator"][i] = (g * np.where(g > 0, em[:, s], 0.0)).sum()         # 0 * -inf is 0: a frame never spent there
        res["log_confidence"][i] = res["numerator"][i] / res["duration"][i]
        t0, m0, c0 = _median(onset[:, s])
        t1, m1, c1 = _median(last[:, s])
        res["start"][i], res["start_margin"][i], res["onset_cdf"][:, i] = t0, m0, c0
        res["end"][i], res["end_margin"][i], res["last_cdf"][:, i] = t1 + 1, m1, c1
    return finish()


def segment_batch(logits, lengths, labels, label_lengths, blank=0, sep=1):
    """The padded batch as decode.ctc_segment returns it (numpy, float64 / int64), plus start_margin / end_margin [B, Lmax] and
    word_start_margin / word_end_margin [B, NW]; 0 beyond the row's labels / words (margins there: inf)."""
    x = np.asarray(logits)
    B, T, V = x.shape
    labels = np.asarray(labels).reshape(B, -1)
    Lmax = labels.shape[1]
    NW = (Lmax + 1) // 2
    out = {"log_prob": np.zeros(B), "start": np.zeros((B, Lmax), np.int64), "end": np.zeros((B, Lmax), np.int64),
           "duration": np.zeros((B, Lmax)), "log_confidence": np.zeros((B, Lmax)), "start_margin": np.full((B, Lmax), np.inf),
           "end_margin": np.full((B, Lmax), np.inf), "feasible": np.zeros(B, bool)}
    if sep is not None:
        out.update({"word_first": np.zeros((B, NW), np.int64), "word_count": np.zeros((B, NW), np.int64),
                    "word_start": np.zeros((B, NW), np.int64), "word_end": np.zeros((B, NW), np.int64),
                    "word_log_confidence": np.zeros((B, NW)), "n_words": np.zeros(B, np.int64),
                    "word_start_margin": np.full((B, NW), np.inf), "word_end_margin": np.full((B, NW), np.inf)})
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        L = Lmax if label_lengths is None else min(max(int(label_lengths[b]), 0), Lmax)
        r = segment_one(x[b, :n], labels[b, :L], blank, sep)
        out["log_prob"][b], out["feasible"][b] = r["log_prob"], r["feasible"]
        for k in ("start", "end", "duration", "log_confidence", "start_margin", "end_margin"):
            out[k][b, :L] = r[k]
        if sep is not None:
            nw = len(r["word_first"])
            out["n_words"][b] = nw
            for k in ("word_first", "word_count", "word_start", "word_end", "word_log_confidence", "word_start_margin",
                      "word_end_margin"):
                out[k][b, :nw] = r[k]
    return out


def planted(rng, L, V, blank=0, sep=None, peak=20.0):
    """A transcript of L labels, an alignment (1-3 frames per label, 0-2 blanks between labels and at the ends, at least one where a
    label repeats) and logits with `peak` nats on the planted class of each frame.  Returns (logits [T, V], labels, starts, ends)."""
    labels, frames, starts, ends = [], [], [], []
    choices = [c for c in range(V) if c != blank]
    frames += [blank] * int(rng.integers(0, 3))
    for i in range(L):
        c = int(rng.choice(choices)) if not labels or rng.random() > 0.25 else labels[-1]
        if i > 0:
            frames += [blank] * int(rng.integers(1 if c == labels[-1] else 0, 3))
        labels.append(c)
        starts.append(len(frames))
        frames += [c] * int(rng.integers(1, 4))
        ends.append(len(frames))
    frames += [blank] * int(rng.integers(0, 3))
    x = np.zeros((len(frames), V), np.float32)
    x[np.arange(len(frames)), frames] = peak
    return x, labels, starts, ends


# ---- the parity cases shared by tests/test_gpu_ctc_segment.py and tools/bench_ctc_segment.py (which measures the errors the test's
# tolerances are derived from): seeded standard_normal logits at three scales, one batch row per scale.
BASE_GRID = ((1, 1), (2, 1), (17, 5), (63, 20), (64, 20), (65, 32), (129, 40), (300, 100), (300, 37))
# S = 255 / 257 and 1023 / 1025 states; and 256 / 257, 512 / 513, 1024 / 1025 PAIRS of states (a blank and its label; pair L is the
# last blank): one pair more per thread of the kernel, its 1 / 2 / 4 / 8 pairs-a-thread variants
SEAMS = ((260, 127), (260, 128), (520, 255), (520, 256), (1030, 511), (1030, 512), (1100, 1023), (1100, 1024))
CLASSES = (2, 29, 71, 128)
SCALES = (0.1, 3.0, 10.0)
PARITY = [(T, L, V) for T, L in BASE_GRID for V in CLASSES] + [(T, L, 29) for T, L in SEAMS]


def parity_case(T, L, V):
    """(logits [3, T, V] fp32, labels [3, L] int64): row r has scale SCALES[r]; labels in [1, V), so V = 2 repeats one label."""
    rng = np.random.default_rng(100000 * T + 100 * L + V)
    x = np.stack([rng.standard_normal((T, V)) * s for s in SCALES]).astype(np.float32)
    labels = rng.integers(1, V, (len(SCALES), L)).astype(np.int64)
    return x, labels


PLANTED = ((1, 2), (8, 5), (20, 29), (60, 29), (130, 71))           # (L, V) of the planted-alignment cases


def planted_case(L, V):
    """(logits [1, T, V], labels [1, L], starts, ends) of one seeded planted alignment."""
    x, labels, starts, ends = planted(np.random.default_rng(1000 * L + V), L, V)
    return x[None], np.array([labels], np.int64), starts, ends


def compare(got, ref, decided_margin):
    """Device results `got` (a dict of numpy arrays, the fields of decode.CTCSegments) against segment_batch's `ref`.  Returns
    {"log_prob_rel", "duration_abs", "log_confidence_abs"}: the largest errors over the feasible rows' labels and words;
    "boundaries", "undecided": how many integer outputs there are and how many have an oracle margin <= decided_margin;
    "wrong": the decided ones that differ."""
    feas = ref["feasible"]
    out = {"log_prob_rel": 0.0, "duration_abs": 0.0, "log_confidence_abs": 0.0, "boundaries": 0, "undecided": 0, "wrong": 0}
    if feas.any():
        lp, rp = got["log_prob"][feas].astype(np.float64), ref["log_prob"][feas]
        out["log_prob_rel"] = float(np.max(np.abs(lp - rp) / np.maximum(1.0, np.abs(rp))))
        out["duration_abs"] = float(np.max(np.abs(got["duration"][feas] - ref["duration"][feas]), initial=0.0))
        pairs = [("log_confidence", "duration")] + ([("word_log_confidence", "word_count")] if "word_first" in ref else [])
        for k, live in pairs:
            m = ref[live][feas] > 0
            out["log_confidence_abs"] = max(out["log_confidence_abs"],
                                            float(np.max(np.abs(got[k][feas][m] - ref[k][feas][m]), initial=0.0)))
    keys = [("start", "start_margin"), ("end", "end_margin")]
    if "word_first" in ref:
        keys += [("word_start", "word_start_margin"), ("word_end", "word_end_margin")]
    for k, mk in keys:
        live = np.isfinite(ref[mk]) & feas[:, None]
        decided = live & (ref[mk] > decided_margin)
        out["boundaries"] += int(live.sum())
        out["undecided"] += int(live.sum() - decided.sum())
        out["wrong"] += int((got[k][decided] != ref[k][decided]).sum())
    return out
