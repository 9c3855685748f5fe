"""References for decode.ctc_align_long (K29, csrc/align_long.hip), shared by test_align_long_cpu.py, test_gpu_align_long.py and
tools/bench_align_long.py.

  mirror(...)      the kernel's recurrence in numpy float32: the same operations in the same order (first maximum wins, one fp32
                   add after the max, the maximum subtracted every R frames and kept in a float64 offset, the window's start moved
                   by the same rule), so path, align, ok and score must equal the launch's exactly.
  viterbi_f64(...) the unbanded Viterbi over the same topology in float64: what the banded one computes when the band never binds.
  planted(...)     seeded test material: a monotone alignment and logits that are one-hot on it over noise.
"""
import numpy as np

R = 16                                                   # re-centring period (v100_ctc_align_long_block)
NEG = np.float32(-np.inf)


def _states(labels, V, blank, free):
    """Per extended position: emission column (V = the free-end column), and whether v - 2 is a candidate."""
    labels = np.asarray(labels, np.int64)
    n = 2 * len(labels) + 1
    ext = np.full(n, blank, np.int64)
    ext[1::2] = labels
    col = np.clip(ext, 0, V - 1)
    skip = np.zeros(n, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    if free:
        col[0] = col[n - 1] = V
    return n, col, skip


def _finish(T, S, n, j, moves, lo_of_block, feasible, score):
    path = np.zeros(T, np.int32)
    align = np.zeros(S, np.int32)
    if not feasible:
        return float("-inf"), 0, path, align
    Tb = len(moves)
    for t in range(Tb - 1, -1, -1):
        path[t] = j
        if t > 0:
            j -= int(moves[t][j - lo_of_block[t // R]])
    np.add.at(align, path[:Tb], 1)
    return score, 1, path, align


def mirror(logp, labels, band, blank=0, free_logp=None, T_out=None, S_out=None):
    """One recording: logp [Tb, V] float32, labels [L] -> (score float, ok, path [T_out] int32, align [S_out] int32)."""
    logp = np.ascontiguousarray(logp, np.float32)
    Tb, V = logp.shape
    W = int(band)
    n, col, skip = _states(labels, V, blank, free_logp is not None)
    T_out = Tb if T_out is None else T_out
    S_out = n if S_out is None else S_out
    if Tb < 1:
        return _finish(T_out, S_out, n, 0, [], [], False, 0.0)
    fl = np.zeros((Tb, 1), np.float32) if free_logp is None else np.asarray(free_logp, np.float32).reshape(Tb, 1)
    rows = np.concatenate([logp, fl], axis=1)            # column V: the free-end emission
    # window slots beyond n are dead states: they stay -inf
    colp = np.concatenate([col, np.zeros(W, np.int64)])
    skipp = np.concatenate([skip, np.zeros(W, bool)])
    dead = np.concatenate([np.zeros(n, bool), np.ones(W, bool)])
    fr = np.concatenate([col == V, np.zeros(W, bool)])
    lo, offset = 0, np.float64(0.0)
    sp = np.full(W + 2, NEG, np.float32)                 # two -inf in front of slot 0: the states below lo
    s = sp[2:]
    k = min(2, n)
    s[:k] = rows[0, colp[:k]]
    moves = [np.zeros(W, np.uint8)]
    lo_of_block = [0]
    two = np.uint8(2)
    for t0 in range(0, Tb, R):
        if t0 > 0:
            m = s.max()
            if m > NEG:
                offset += np.float64(m)
                cand = np.where(fr[lo:lo + W], NEG, s)   # a free end state bounds every other score: it does not steer the window
                nlo = lo
                if cand.max() > NEG:
                    a = int(np.argmax(cand))             # the first slot that attains the maximum
                    nlo = min(max(lo, lo + a - W // 2), max(n - W, 0))
                sh = nlo - lo
                new = np.full(W, NEG, np.float32)
                new[:W - sh] = s[sh:] - m
                s[:] = new
                lo = nlo
            lo_of_block.append(lo)
        t1 = min(Tb, t0 + R)
        c, sk, dd = colp[lo:lo + W], skipp[lo:lo + W], dead[lo:lo + W]
        E = rows[t0:t1][:, c]                            # [frames, W]
        E[:, dd] = NEG                                   # -inf + anything finite stays -inf: the dead states
        c1, c2 = sp[1:W + 1], sp[:W]
        for t in range(max(t0, 1), t1):
            m1 = c1 > s
            best = np.where(m1, c1, s)
            m2 = c2 > best
            m2 &= sk
            best = np.where(m2, c2, best)
            best += E[t - t0]
            moves.append(np.where(m2, two, m1.view(np.uint8)))
            s[:] = best
    get = lambda v: s[v - lo] if lo <= v < lo + W else NEG    # noqa: E731
    j = 0
    if n >= 2:
        j = n - 1 if get(n - 1) > get(n - 2) else n - 2
    sj = get(j)
    feasible = bool(sj > NEG)
    return _finish(T_out, S_out, n, j, moves, lo_of_block, feasible, float(offset + np.float64(sj)) if feasible else 0.0)


def mirror_batch(logp, labels, in_len=None, lab_len=None, band=2048, blank=0, free_ends=False):
    """The launch's outputs for a batch: logp [B, T, V], labels [B, Lmax] -> (score [B] f64, ok [B] i32, path [B, T], align [B, 2 Lmax + 1])."""
    logp, labels = np.asarray(logp, np.float32), np.asarray(labels, np.int64)
    B, T, V = logp.shape
    Lmax = labels.shape[1]
    out = []
    for b in range(B):
        Tb = T if in_len is None else max(min(int(in_len[b]), T), 0)
        L = Lmax if lab_len is None else min(max(int(lab_len[b]), 0), Lmax)
        free = logp[b, :Tb].max(-1) if free_ends else None
        out.append(mirror(logp[b, :Tb], labels[b, :L], band, blank, free, T, 2 * Lmax + 1))
    return (np.array([o[0] for o in out], np.float64), np.array([o[1] for o in out], np.int32),
            np.stack([o[2] for o in out]), np.stack([o[3] for o in out]))


def viterbi_f64(logp, labels, blank=0, free_logp=None):
    """The unbanded Viterbi in float64 with the mirror's candidate order and end rule -> (score, ok, path, align)."""
    logp = np.asarray(logp, np.float64)
    Tb, V = logp.shape
    n, col, skip = _states(labels, V, blank, free_logp is not None)
    if Tb < 1:
        return _finish(Tb, n, n, 0, [], [], False, 0.0)
    fl = np.zeros((Tb, 1)) if free_logp is None else np.asarray(free_logp, np.float64).reshape(Tb, 1)
    E = np.concatenate([logp, fl], axis=1)[:, col]
    sp = np.full(n + 2, -np.inf)
    s = sp[2:]
    s[:min(2, n)] = E[0, :min(2, n)]
    moves = [np.zeros(n, np.uint8)]
    for t in range(1, Tb):
        best = s.copy()
        c1 = sp[1:n + 1]
        m1 = c1 > best
        best[m1] = c1[m1]
        m2 = skip & (sp[:n] > best)
        best[m2] = sp[:n][m2]
        mv = m1.astype(np.uint8)
        mv[m2] = 2
        s[:] = best + E[t]
        moves.append(mv)
    j = 0
    if n >= 2:
        j = n - 1 if s[n - 1] > s[n - 2] else n - 2
    feasible = bool(s[j] > -np.inf)
    return _finish(Tb, n, n, j, moves, [0] * (Tb // R + 1), feasible, float(s[j]))


def planted(seed, T, L, V, blank=0, nats=20.0, noise=1.0, repeats=False):
    """A seeded monotone alignment of L labels over T >= 2 L + 1 frames and logits that are `nats` on it over N(0, noise):
    (logits [T, V] float32, labels [L] int64, path [T] int32 extended positions).  Every label gets at least one frame and is
    followed by at least one blank frame, so the planted path is a valid CTC path whatever the labels are."""
    rng = np.random.default_rng(seed)
    others = np.array([c for c in range(V) if c != blank])
    labels = rng.choice(others, size=L).astype(np.int64)
    if repeats and L >= 2:
        labels[1::2] = labels[:-1:2][:len(labels[1::2])]  # "aab..." pairs: no skip over the blank between them
    n = 2 * L + 1
    assert T >= n
    dur = np.ones(n, np.int64)
    extra = rng.multinomial(T - n, np.full(n, 1.0 / n))
    dur += extra
    path = np.repeat(np.arange(n, dtype=np.int32), dur)
    ext = np.full(n, blank, np.int64)
    ext[1::2] = labels
    logits = (rng.standard_normal((T, V)) * noise).astype(np.float32)
    logits[np.arange(T), ext[path]] += np.float32(nats)
    return logits, labels, path


def log_softmax32(x):
    """log_softmax in float32 on the host (test material only: the GPU tests feed the SAME array to the launch and the mirror)."""
    x = np.asarray(x, np.float32)
    z = x - x.max(-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(-1, keepdims=True, dtype=np.float32))).astype(np.float32)
