"""Host references for the edit-distance tests, written from the recurrence (not from the code under test):

    D[0][j] = j, D[i][0] = i, D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (a[i-1] != b[j-1]))

lev_loop is the textbook double loop; lev_rows the same recurrence a row at a time in numpy, for long rows: with
t[j] = min(D[i-1][j] + 1, D[i-1][j-1] + neq[j]) and t[0] = i, unrolling D[i][j] = min(t[j], D[i][j-1] + 1) gives
D[i][j] = min_{k <= j} (t[k] + j - k) = cummin(t - j) + j.  Tokens are anything comparable with == (ints, tuples of ints)."""
import numpy as np


def lev_loop(a, b):
    n, m = len(a), len(b)
    prev = list(range(m + 1))
    for i in range(1, n + 1):
        cur = [i] + [0] * m
        for j in range(1, m + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[m]


def lev_rows(a, b):
    """a, b: 1-d integer arrays (int64: all 64 bits compare)."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    m = len(b)
    j = np.arange(m + 1, dtype=np.int64)
    d = j.copy()
    t = np.empty(m + 1, dtype=np.int64)
    for i in range(1, len(a) + 1):
        t[0] = i
        np.minimum(d[1:] + 1, d[:-1] + (b != a[i - 1]), out=t[1:])
        d = np.minimum.accumulate(t - j) + j
    return int(d[m])


def split_words(ids, sep):
    """The maximal runs of ids != sep, as tuples: str.split() on the decoded text."""
    words, cur = [], []
    for x in ids:
        x = int(x)
        if x == sep:
            if cur:
                words.append(tuple(cur))
            cur = []
        else:
            cur.append(x)
    if cur:
        words.append(tuple(cur))
    return words


def word_ids(a_words, b_words):
    """Words -> small integers, equal words to equal integers (so that lev_rows can score word sequences)."""
    table = {}
    return [table.setdefault(w, len(table)) for w in a_words], [table.setdefault(w, len(table)) for w in b_words]


def score_rows(hyp, hyp_len, ref, ref_len, sep=None):
    """Per-row (dist, hyp_n, ref_n) of padded [B, T] integer arrays with lengths clamped to [0, width], as int lists."""
    hyp, ref = np.asarray(hyp), np.asarray(ref)
    out = []
    for b in range(hyp.shape[0]):
        h = hyp[b, :min(max(int(hyp_len[b]), 0), hyp.shape[1])]
        r = ref[b, :min(max(int(ref_len[b]), 0), ref.shape[1])]
        if sep is not None:
            h, r = word_ids(split_words(h, sep), split_words(r, sep))
        out.append((lev_rows(h, r), len(h), len(r)))
    return [list(c) for c in zip(*out)]
