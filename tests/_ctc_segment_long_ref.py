"""Float64 numpy oracle of decode.ctc_segment_long (K33): K26's posterior over the CTC alignments of a GIVEN transcript, restricted
to the alignments that stay inside a corridor.  Frames come in blocks of B16; lo[k] is the first live state of block k = t >> 4 and
`band` = W the number of live states: alpha_t(s), beta_t(s) and with them the enter and leave terms are zero wherever
not lo[t >> 4] <= s < lo[t >> 4] + W.  Nothing else is new: topology, emissions, gamma, the onset and last-frame distributions, medians,
durations, confidences and words are tests/_ctc_segment_ref.py's, and with lo = 0 and W >= 2 L + 1 the two files agree.

The lattices are kept in window coordinates, [T, W] and not [T, 2 L + 1], so that 20,000 frames against 6,000 labels run in seconds.
corridor() is decode.ctc_corridor's rule in numpy, sanitise() what the kernel does to a caller's lo before it trusts it."""
import numpy as np

from _ctc_segment_ref import NEG, SCALES, log_softmax, word_spans

B16 = 16                                                 # frames per block (v100_ctc_segment_long_block)


def lo_max(n, W):
    """The largest admissible lo: even, and the window [lo, lo + W) still holds state n - 1 (it may stick out one state past n)."""
    return (max(n - W, 0) + 1) & ~1


def sanitise(lo, n, W):
    """Clamp to [0, lo_max], clear bit 0, running maximum."""
    lo = np.clip(np.asarray(lo, np.int64), 0, lo_max(n, W)) & ~1
    return np.maximum.accumulate(lo) if lo.size else lo


def corridor(path, Tb, L, W, nblk=None):
    """lo [nblk] from a CTC path (extended positions, one per frame): c_k = path[16 k], lo_k = clamp((c_k + 16 - W / 2) & ~1, 0, hi),
    then a running maximum; blocks beyond the row's Tb frames repeat the last value (all 0 where Tb = 0)."""
    nb = (Tb + B16 - 1) // B16
    nblk = nb if nblk is None else nblk
    out = np.zeros(nblk, np.int64)
    if nb:
        c = np.asarray(path, np.int64)[:Tb:B16]
        lo = np.maximum.accumulate(np.clip((c + 16 - W // 2) & ~1, 0, lo_max(2 * L + 1, W)))
        out[:nb] = lo[:nblk]
        out[nb:] = lo[-1]
    return out


def _window(row, lo_row, first, count):
    """The values of states first .. first + count - 1 out of a row that holds the states lo_row .. lo_row + W - 1; -inf for the
    states that the row does not hold (they were dead at the row's frame)."""
    out = np.full(count, NEG)
    a, b = max(first, lo_row), min(first + count, lo_row + len(row))
    if a < b:
        out[a - first:b - first] = row[a - lo_row:b - lo_row]
    return out


def segment_one_banded(logits, labels, lo, band, blank=0, sep=1):
    """One recording: logits [T, V], labels a sequence of L ints, lo [ceil(T / 16)] (sanitised here), band = W.  Returns
    _ctc_segment_ref.segment_one's dict without the two [T, L] cdf tables."""
    x = np.asarray(logits, np.float64)
    T, V = x.shape
    labels = [int(c) for c in labels]
    L = len(labels)
    n = 2 * L + 1
    W = int(band)
    res = {"feasible": False, "log_prob": NEG, "start": np.zeros(L, np.int64), "end": np.zeros(L, np.int64),
           "duration": np.zeros(L), "log_confidence": np.full(L, NEG), "start_margin": np.full(L, 0.5), "end_margin": np.full(L, 0.5),
           "numerator": np.zeros(L)}

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
    nblk = (T + B16 - 1) // B16
    lo = sanitise(np.asarray(lo).reshape(-1)[:nblk], n, W)
    assert lo.shape == (nblk,)
    lp = log_softmax(x)
    # everything per state, padded so that any window can be cut out of it: states >= n are dead
    z = np.full(n + W + 2, blank, np.int64)
    z[1:n:2] = labels
    dead = np.ones(n + W + 2, bool)
    dead[:n] = False
    skip = np.zeros(n + W + 2, bool)                     # the +2 transition INTO s
    if L >= 2:
        skip[3:n:2] = z[3:n:2] != z[1:n - 2:2]
    skip_out = np.zeros(n + W + 2, bool)                 # ... OUT of s
    skip_out[:max(n - 2, 0)] = skip[2:max(n, 2)]
    blk = np.arange(T) >> 4
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        em = np.empty((T, W))
        for k in range(nblk):
            a = lo[k]
            e = lp[k * B16:(k + 1) * B16][:, z[a:a + W]]
            e[:, dead[a:a + W]] = NEG
            em[k * B16:(k + 1) * B16] = e
        alpha = np.full((T, W), NEG)
        enter = np.full((T, W), NEG)
        if lo[0] == 0:
            alpha[0, :min(2, n, W)] = em[0, :min(2, n, W)]
            enter[0, :min(2, n, W)] = 0.0
        for t in range(1, T):                            # a predecessor counts where it was live at t - 1, whatever the window is at t
            a0 = lo[blk[t]]
            a = _window(alpha[t - 1], lo[blk[t - 1]], a0 - 2, W + 2)
            enter[t] = np.logaddexp(a[1:W + 1], np.where(skip[a0:a0 + W], a[:W], NEG))
            alpha[t] = em[t] + np.logaddexp(a[2:], enter[t])  # em is -inf at the dead states

        def at(row, t, s):
            j = s - lo[blk[t]]
            return row[j] if 0 <= j < W and s >= 0 else NEG
        logp = np.logaddexp(at(alpha[T - 1], T - 1, n - 1), at(alpha[T - 1], T - 1, n - 2))
        if not np.isfinite(logp):
            if np.isnan(logp):
                res["log_prob"] = np.nan
            return finish()
        beta = np.full((T, W), NEG)
        leave = np.full((T, W), NEG)
        a0 = lo[nblk - 1]
        for s in (n - 1, n - 2):
            if s >= 0 and 0 <= s - a0 < W:
                beta[T - 1, s - a0] = leave[T - 1, s - a0] = 0.0
        for t in range(T - 2, -1, -1):
            a0 = lo[blk[t]]
            bt = _window(em[t + 1] + beta[t + 1], lo[blk[t + 1]], a0, W + 2)      # ... and a successor where it is live at t + 1
            live = ~dead[a0:a0 + W]
            leave[t] = np.where(live, np.logaddexp(bt[1:W + 1], np.where(skip_out[a0:a0 + W], bt[2:], NEG)), NEG)
            beta[t] = np.where(live, np.logaddexp(bt[:W], leave[t]), NEG)
        gamma = np.exp(alpha + beta - logp)
        onset = np.exp(enter + em + beta - logp)
        last = np.exp(alpha + leave - logp)
        gamma, onset, last = (np.where(np.isnan(v), 0.0, v) for v in (gamma, onset, last))
        gnum = gamma * np.where(gamma > 0, em, 0.0)      # 0 * -inf is 0: a frame never spent there
    res["feasible"], res["log_prob"] = True, float(logp)
    # per label, block by block: slot j of block k is state lo[k] + j; label i is state 2 i + 1, so (lo even) the odd slots
    jj = np.arange(1, W, 2)
    cum_on, cum_la = np.zeros(L), np.zeros(L)            # the two cdfs up to the block before
    prev_on, prev_la = np.zeros(L), np.zeros(L)          # ... and one frame before that block's end
    got_on, got_la = np.zeros(L, bool), np.zeros(L, bool)

    def medians(pmf, idx, t0, cum, prev, got, key, mkey, plus):
        c = np.cumsum(np.concatenate([cum[idx][None], pmf]), axis=0)          # row r + 1: the cdf at frame t0 + r
        hit = c[1:] >= 0.5
        first = np.argmax(hit, axis=0)
        new = hit.any(axis=0) & ~got[idx]
        cols = np.nonzero(new)[0]
        r = first[cols]
        res[key][idx[cols]] = t0 + r + plus
        res[mkey][idx[cols]] = np.minimum(np.abs(c[r + 1, cols] - 0.5), np.abs(c[r, cols] - 0.5))
        got[idx[cols]] = True
        prev[idx] = c[-2]
        cum[idx] = c[-1]

    for k in range(nblk):
        a0, t0, t1 = lo[k], k * B16, min(T, (k + 1) * B16)
        idx = (a0 + jj - 1) // 2
        keep = idx < L
        idx, cols = idx[keep], jj[keep]
        if idx.size == 0:
            continue
        np.add.at(res["duration"], idx, gamma[t0:t1][:, cols].sum(axis=0))
        np.add.at(res["numerator"], idx, gnum[t0:t1][:, cols].sum(axis=0))
        medians(onset[t0:t1][:, cols], idx, t0, cum_on, prev_on, got_on, "start", "start_margin", 0)
        medians(last[t0:t1][:, cols], idx, t0, cum_la, prev_la, got_la, "end", "end_margin", 1)
    for got, cum, prev, key, mkey, plus in ((got_on, cum_on, prev_on, "start", "start_margin", 0),
                                            (got_la, cum_la, prev_la, "end", "end_margin", 1)):
        miss = ~got                                      # a cdf that never reaches 1/2: the last frame, as _ctc_segment_ref._median
        res[key][miss] = T - 1 + plus
        res[mkey][miss] = np.minimum(np.abs(cum[miss] - 0.5), np.abs(prev[miss] - 0.5))
    with np.errstate(invalid="ignore", divide="ignore"):
        res["log_confidence"] = res["numerator"] / res["duration"]
    return finish()


def segment_batch_banded(logits, lengths, labels, label_lengths, lo, band, blank=0, sep=1):
    """The padded batch as decode.ctc_segment_long returns it (numpy, float64 / int64), in _ctc_segment_ref.segment_batch's layout;
    lo [B, ceil(T / 16)]."""
    x = np.asarray(logits)
    B, T, V = x.shape
    labels = np.asarray(labels).reshape(B, -1)
    lo = np.asarray(lo).reshape(B, -1)
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
        r = segment_one_banded(x[b, :n], labels[b, :L], lo[b], band, blank, sep)
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


def viterbi_corridor(logits, labels, W, blank=0, align_band=2048, nblk=None):
    """lo from the path that _align_long_ref.mirror finds on the fp32 log-softmax of the logits (what decode.ctc_segment_long does
    when it is given neither a path nor a corridor); zeros where the aligner loses the row."""
    import _align_long_ref as AR
    x = np.asarray(logits, np.float32)
    _, ok, path, _ = AR.mirror(AR.log_softmax32(x), labels, align_band, blank)
    if not ok:
        return np.zeros((len(x) + B16 - 1) // B16 if nblk is None else nblk, np.int64), path, 0
    return corridor(path, len(x), len(labels), W, nblk), path, 1


# ---- the case lists shared by tests/test_ctc_segment_long_cpu.py, tests/test_gpu_ctc_segment_long.py and
# tools/bench_ctc_segment_long.py (which measures the errors that the tolerances beyond K26's shapes come from)
EXACT_T = (1, 2, 15, 16, 17, 31, 32, 33, 300)
EXACT_L = (0, 1, 5, 37)
EXACT_V = (2, 29, 128)
EXACT = [(T, L, V) for T in EXACT_T for L in EXACT_L for V in EXACT_V if T >= 2 * L - 1]      # fewer frames cannot hold L equal labels (V = 2)
MOVING = ((400, 100, 2), (400, 100, 29), (400, 60, 2), (400, 60, 29), (1000, 200, 2), (1000, 200, 71))   # (T, L, V), band 64
MOVING_BAND = 64
OVERFLOW = (3000, 5, 4, 6000.0)                          # T, L, V, nats below the frame's best class
LONG = (20000, 6000, 29, 256, 6.0)                       # T, L, V, band, planted nats


def diffuse_case(T, L, V):
    """(logits [3, T, V] fp32, labels [3, L] int64): seeded normal logits, row r at scale SCALES[r]; V = 2 repeats one label."""
    rng = np.random.default_rng(7000000 + 1000 * T + 10 * L + V)
    x = np.stack([rng.standard_normal((T, V)) * s for s in SCALES]).astype(np.float32)
    labels = rng.integers(1, V, (len(SCALES), L)).astype(np.int64)
    return x, labels


def planted_case(T, L, V, nats=6.0, seed=None):
    """(logits [1, T, V] fp32, labels [1, L], path [T]) from _align_long_ref.planted."""
    import _align_long_ref as AR
    x, labels, path = AR.planted(31 * T + L + V if seed is None else seed, T, L, V, nats=nats)
    return x[None], labels[None], path


def overflow_case():
    """Every frame's best class is one the transcript does not hold; the transcript's labels and the blank lie `nats` below it, so
    the lattice loses about 8,656 bits a frame and the running exponent passes 2^24 before frame 2,000."""
    T, L, V, nats = OVERFLOW
    rng = np.random.default_rng(33)
    x = rng.standard_normal((T, V)).astype(np.float32)
    x[:, V - 1] += np.float32(nats)
    labels = np.array([[1, 2, 1, 2, 2]], np.int64)[:, :L]
    return x[None], labels
