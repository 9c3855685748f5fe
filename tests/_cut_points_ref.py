"""The definition of decode.ctc_cut_points (K31) in numpy, and beside it an independent brute-force checker of what the rule promises.

mirror(logits, lengths, ...) follows the rule step by step with array operations: margins (one fp32 subtraction per frame), trim,
stage A (pauses of min_gap silent frames or more), stage B (oversized cores, left to right: the longest admissible silent run, ties
to the latest, else a forced cut at the first maximum of the margin), pads.  Every decision is an integer comparison or a comparison
of such margins, so the device must equal it exactly.

check(...) does not share a line with it: plain Python loops over frames and segments."""
import numpy as np


def margins(x, blank):
    """d[t] = x[t, blank] - max over v != blank of x[t, v] in fp32 (a NaN anywhere in the frame gives NaN), x [n, V] fp32."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (x[:, blank] - np.delete(x, blank, axis=1).max(axis=1)).astype(np.float32)


def _runs(flag):
    """(starts, ends) of the maximal True runs of a bool vector."""
    e = np.diff(np.concatenate([[0], flag.astype(np.int8), [0]]))
    return np.flatnonzero(e == 1), np.flatnonzero(e == -1)


def pieces_of_row(d, max_frames=3000, min_gap=25, margin=0.0, pad=5, min_frames=50):
    """The core pieces [(start, end, forced)] of one row before the pads, from its margins d [n]."""
    with np.errstate(invalid="ignore"):
        silent = d > np.float32(margin)                   # a NaN is not silent
    dk = np.where(np.isnan(d), -np.inf, d).astype(np.float32)
    loud = np.flatnonzero(~silent)
    if loud.size == 0:
        return []
    a0, b0 = int(loud[0]), int(loud[-1]) + 1
    rs, re = _runs(silent[a0:b0])
    rs, re = rs + a0, re + a0
    C = max_frames - 2 * pad
    cut = (re - rs) >= min_gap if min_gap is not None else np.zeros(rs.shape, dtype=bool)
    starts = np.concatenate([[a0], re[cut]])
    ends = np.concatenate([rs[cut], [b0]])
    out = []
    for a, b in zip(starts.tolist(), ends.tolist()):
        if b - a <= C:
            out.append((a, b, 0))
            continue
        j1 = int(np.searchsorted(rs, b, "left"))          # the runs of this core: those that begin before its end
        forced = 0
        while b - a > C:
            jl = int(np.searchsorted(rs, a + min_frames, "left"))
            jh = min(int(np.searchsorted(rs, a + C, "right")), j1)
            cand = np.arange(jl, jh)
            cand = cand[b - re[cand] >= min_frames]
            if cand.size:
                ln = re[cand] - rs[cand]
                j = int(cand[np.flatnonzero(ln == ln.max())[-1]])         # the longest, ties to the latest
                out.append((a, int(rs[j]), forced))
                a, forced = int(re[j]), 0
            else:
                lo, hi = a + max(C // 2, min_frames), min(a + C, b - min_frames)
                t = lo + int(np.argmax(dk[lo:hi + 1]))                     # the first maximum
                out.append((a, t, forced))
                a, forced = t, 1
        out.append((a, b, forced))
    return out


def pad_pieces(pieces, n, pad):
    """Widen the pieces into the silence around them: (start, end, forced) lists."""
    S = len(pieces)
    start, end, forced = [p[0] for p in pieces], [p[1] for p in pieces], [p[2] for p in pieces]
    s2, e2 = list(start), list(end)
    for i in range(S):
        if i == 0:
            s2[i] = start[i] - min(pad, start[i])
        elif not forced[i]:
            s2[i] = start[i] - min(pad, (start[i] - end[i - 1]) // 2)
        if i == S - 1:
            e2[i] = end[i] + min(pad, n - end[i])
        elif not forced[i + 1]:
            e2[i] = end[i] + min(pad, (start[i + 1] - end[i]) // 2)
    return s2, e2, forced


def mirror(logits, lengths=None, blank=0, max_frames=3000, min_gap=25, margin=0.0, pad=5, min_frames=50):
    """logits [B, T, V] -> (start [B, S], end [B, S], forced [B, S], n_seg [B]) int32, S the largest count (0 columns if none)."""
    logits = np.asarray(logits, dtype=np.float32)
    B, T, V = logits.shape
    C = max_frames - 2 * pad
    assert 1 <= T <= 1 << 20 and 2 <= V <= 128 and 0 <= blank < V and 2 <= max_frames <= 4096 and pad >= 0 and min_frames >= 1
    assert C >= 2 * min_frames and (min_gap is None or min_gap >= 1)
    rows = []
    for b in range(B):
        n = T if lengths is None else int(min(max(int(lengths[b]), 0), T))
        d = margins(logits[b, :n], blank)
        rows.append(pad_pieces(pieces_of_row(d, max_frames, min_gap, margin, pad, min_frames), n, pad))
    S = max(len(r[0]) for r in rows)
    out = [np.zeros((B, S), dtype=np.int32) for _ in range(3)]
    n_seg = np.zeros((B,), dtype=np.int32)
    for b, r in enumerate(rows):
        n_seg[b] = len(r[0])
        for k in range(3):
            out[k][b, :len(r[k])] = r[k]
    return out[0], out[1], out[2], n_seg


def check(logits_row, n, start, end, forced, blank=0, max_frames=3000, min_gap=25, margin=0.0, pad=5, min_frames=50):
    """Brute force over one row: raises AssertionError naming the first promise that start / end / forced (the row's n_seg entries)
    break.  Independent of mirror(): frame-by-frame loops."""
    x = np.asarray(logits_row, dtype=np.float32)[:n]
    S = len(start)
    C = max_frames - 2 * pad
    loud = []
    for vals in x.tolist():                               # Python floats hold the fp32 values exactly
        others = vals[:blank] + vals[blank + 1:]
        bad = any(v != v for v in vals)
        with np.errstate(invalid="ignore"):
            dt = np.float32(vals[blank]) - np.float32(max(others)) if not bad else np.float32("nan")
        loud.append(not (dt > np.float32(margin)))
    if not any(loud):
        assert S == 0, "a row without a non-silent frame has segments"
        return
    assert S >= 1, "no segment although there are non-silent frames"
    owner = [-1] * n
    for i in range(S):
        s, e = int(start[i]), int(end[i])
        assert 0 <= s < e <= n, f"segment {i} = [{s}, {e}) is empty or outside [0, {n})"
        assert e - s <= max_frames, f"segment {i} is {e - s} frames long"
        assert i == 0 or s >= int(end[i - 1]), f"segment {i} begins before segment {i - 1} ends"
        assert int(forced[i]) in (0, 1) and (i > 0 or int(forced[i]) == 0)
        if int(forced[i]):
            assert s == int(end[i - 1]), f"forced segment {i} does not begin where segment {i - 1} ends"
        for t in range(s, e):
            owner[t] = i
    for t in range(n):
        assert not loud[t] or owner[t] >= 0, f"non-silent frame {t} lies in no segment"
    # the cores: what lies between pauses of min_gap silent frames or more inside the trimmed recording
    first, last = loud.index(True), n - 1 - loud[::-1].index(True)
    cores, t, a = [], first, first
    while t <= last:
        if loud[t]:
            t += 1
            continue
        r = t
        while not loud[r]:
            r += 1
        if min_gap is not None and r - t >= min_gap:
            cores.append((a, t))
            a = r
        t = r
    cores.append((a, last + 1))
    for a, b in cores:
        segs = sorted({owner[t] for t in range(a, b) if owner[t] >= 0})
        assert segs, f"core [{a}, {b}) lies in no segment"
        for i in segs:
            assert int(start[i]) >= a - pad and int(end[i]) <= b + pad, f"segment {i} spans more than the core [{a}, {b})"
        if len(segs) == 1:
            assert b - a <= C, f"core [{a}, {b}) of {b - a} frames was not split"
        else:
            assert b - a > C, f"core [{a}, {b}) of {b - a} frames was split"
            for i in segs:
                inside = sum(1 for t in range(max(a, int(start[i])), min(b, int(end[i]))))
                assert inside >= min_frames, f"piece {i} of core [{a}, {b}) holds {inside} frames"
    for i in range(1, S):                                 # two segments never share a core's pause
        if not int(forced[i]):
            assert all(not loud[t] for t in range(int(end[i - 1]), int(start[i])))


def planted(seed, n_frames, V=29, pause=(30, 80), speech=(100, 300), label=(2, 8), amp=20.0, noise=1.0, blank=0):
    """One-hot logits at `amp` nats plus Gaussian noise: runs of labels (each held label[0]..label[1] frames, a blank frame between
    repeats) in utterances of speech[0]..speech[1] frames, separated by pauses of pause[0]..pause[1] blank frames.  Returns
    logits [n_frames, V] fp32 and the frame labels [n_frames]."""
    rng = np.random.default_rng(seed)
    lab = np.full((n_frames,), blank, dtype=np.int64)
    t = int(rng.integers(0, pause[1]))
    others = [v for v in range(V) if v != blank]
    while t < n_frames:
        stop = min(n_frames, t + int(rng.integers(speech[0], speech[1] + 1)))
        prev = -1
        while t < stop:
            v = others[int(rng.integers(len(others)))]
            if v == prev:
                t += 1                                    # a blank frame between repeats
            k = int(rng.integers(label[0], label[1] + 1))
            lab[t:min(stop, t + k)] = v
            t += k
            prev = v
            if rng.random() < 0.2:
                t += int(rng.integers(1, 4))              # a short blank run inside the utterance
                prev = -1
        t = stop + int(rng.integers(pause[0], pause[1] + 1))
    x = rng.standard_normal((n_frames, V)).astype(np.float32) * np.float32(noise)
    x[np.arange(n_frames), lab] += np.float32(amp)
    return x, lab


def from_labels(lab, V, blank=0, seed=0, noise=1.0, amp=20.0):
    """Logits [T, V] whose frame t peaks at lab[t] (`amp` nats above Gaussian noise); lab == blank is a silent frame."""
    lab = np.asarray(lab, dtype=np.int64)
    x = np.random.default_rng(seed).standard_normal((lab.shape[0], V)).astype(np.float32) * np.float32(noise)
    x[np.arange(lab.shape[0]), lab] += np.float32(amp)
    return x


def pattern(spec, V=29, blank=0, seed=0, noise=1.0):
    """Logits from a run-length spec: [("s", 5), ("n", 10), ...] -- "s" silent frames, "n" non-silent ones (labels change every
    three frames, never the blank)."""
    rng = np.random.default_rng(seed + 1000)
    others = [v for v in range(V) if v != blank]
    lab = []
    for kind, count in spec:
        for i in range(count):
            if kind == "s":
                lab.append(blank)
            else:
                if i % 3 == 0:
                    cur = others[int(rng.integers(len(others)))]
                lab.append(cur)
    return from_labels(lab, V, blank, seed, noise)


SMALL = dict(max_frames=8, min_gap=3, margin=0.0, pad=1, min_frames=2)
MID = dict(max_frames=16, min_gap=4, margin=0.0, pad=2, min_frames=4)


def case_list(span=64, per_pass=32768):
    """[(name, logits [B, T, V], lengths or None, arguments)]: the list tests/test_gpu_cut_points.py and tools/cut_points_host.py
    run.  span / per_pass: the kernel's frames per thread and per pass of its run scan."""
    cases = []

    def add(name, x, lengths=None, **kw):
        x = np.asarray(x, dtype=np.float32)
        cases.append((name, x if x.ndim == 3 else x[None], None if lengths is None else np.asarray(lengths, dtype=np.int64), kw))

    def noisy(seed, T, V=29, blank=0, p=0.35, hold=3):
        """Random short runs: each block of 1..hold frames is silent with probability p."""
        rng = np.random.default_rng(seed)
        spec = []
        t = 0
        while t < T:
            k = min(int(rng.integers(1, hold + 1)), T - t)
            spec.append(("s" if rng.random() < p else "n", k))
            t += k
        return pattern(spec, V, blank, seed)

    # the smallest lengths and the word of 64 silent bits, B = 3 with lengths {0, short, T}, both blanks
    for T in sorted({1, 2, 63, 64, 65, span - 1, span, span + 1}):
        for blank in (0, 28):
            x = np.stack([noisy(10 * T + b, T, 29, blank) for b in range(3)])
            add(f"T={T} blank={blank} small", x, [0, max(T // 3, 1), T], blank=blank, **SMALL)
    # around the pass of the run scan, and many passes
    for T in (per_pass - 1, per_pass, per_pass + 1):
        x, _ = planted(T, T)
        add(f"T={T} planted", x, None, max_frames=512, min_gap=25, pad=5, min_frames=50)
        add(f"T={T} short runs", noisy(T, T, 29, 0, 0.4, 5), None, **MID)
    x, _ = planted(7, 70001)
    add("T=70001 planted, defaults", np.stack([x, np.roll(x, 12345, axis=0)]), [70001, 40000])
    add("T=70001 planted, stage B only", x, None, max_frames=1000, min_gap=None, pad=5, min_frames=50)
    # the widths of the vocabulary
    for V in (2, 128):
        for blank in (0, V - 1):
            add(f"V={V} blank={blank}", np.stack([noisy(V + blank + b, 300, V, blank) for b in range(2)]), [300, 299], blank=blank, **MID)
    # degenerate rows
    T = 100
    sil = pattern([("s", T)])
    loud = pattern([("n", T)])
    add("all frames silent", sil, None, **MID)
    add("no frame silent", loud, None, **MID)
    add("no frame silent, max_frames 8, pad 0", loud, None, max_frames=8, min_gap=3, pad=0, min_frames=2)
    add("one non-silent frame at an end", np.stack([pattern([("n", 1), ("s", T - 1)]), pattern([("s", T - 1), ("n", 1)]),
                                                    pattern([("n", 1), ("s", T - 2), ("n", 1)])]), None, **MID)
    add("all silent / none / mixed rows of one batch", np.stack([sil, loud, noisy(5, T)]), [T, T - 1, T - 2], **MID)
    # runs: touching both ends, exactly min_gap and one less
    g = MID["min_gap"]
    add("runs at both ends, of min_gap and min_gap - 1", pattern([("s", 7), ("n", 6), ("s", g), ("n", 5), ("s", g - 1), ("n", 6), ("s", 9)]),
        None, **MID)
    add("runs at both ends, pad 0", pattern([("s", 1), ("n", 6), ("s", g), ("n", 5), ("s", g + 1), ("n", 6), ("s", 2)]), None,
        max_frames=16, min_gap=g, pad=0, min_frames=4)
    add("odd silences of 1, 2, 3 frames to share", pattern([("s", 1), ("n", 5), ("s", 5), ("n", 5), ("s", 6), ("n", 5), ("s", 7), ("n", 4), ("s", 2)]),
        None, max_frames=16, min_gap=4, pad=3, min_frames=2)
    # stage B: equal candidates (the latest wins), a staircase of shrinking runs, five and more splits, forced cuts with equal maxima
    add("equal candidate runs", pattern([("n", 5), ("s", 2), ("n", 3), ("s", 2), ("n", 3), ("s", 2), ("n", 6), ("s", 1), ("n", 5)]), None,
        max_frames=20, min_gap=5, pad=2, min_frames=4)
    stairs = [("n", 6)]
    for k in range(9, 0, -1):
        stairs += [("s", k), ("n", 6)]
    add("a staircase of shrinking runs", pattern(stairs), None, max_frames=24, min_gap=10, pad=2, min_frames=5)
    add("a staircase of growing runs", pattern(stairs[::-1]), None, max_frames=24, min_gap=10, pad=2, min_frames=5)
    add("a staircase, stage B only", pattern(stairs), None, max_frames=24, min_gap=None, pad=0, min_frames=5)
    long_core = []
    for k in range(40):
        long_core += [("n", 5 + k % 4), ("s", 1 + k % 3)]
    add("a core split many times", pattern(long_core + [("n", 3)]), None, max_frames=16, min_gap=4, pad=1, min_frames=3)
    add("a core split many times, tiny frames", pattern(long_core + [("n", 3)]), None, **SMALL)
    flat = np.zeros((150, 29), dtype=np.float32)
    flat[:, 3] = 2.0                                       # every margin equals -2: the first maximum is the window's first frame
    add("forced cuts with equal maxima", flat, None, **MID)
    flat2 = flat.copy()
    flat2[::5, 0] = 1.5                                    # equal maxima (-0.5) every fifth frame
    add("forced cuts with equal maxima every fifth frame", flat2, None, max_frames=16, min_gap=4, pad=0, min_frames=4)
    zero = np.zeros((90, 29), dtype=np.float32)
    zero[::2, 0] = -0.0                                    # margins of +0 and -0: not silent at margin 0, and equal
    add("margins of plus and minus zero", zero, None, **MID)
    # NaN and infinities
    bad = noisy(77, 400)
    rng = np.random.default_rng(78)
    for value in (np.nan, np.inf, -np.inf):
        t, v = rng.integers(0, 400, 40), rng.integers(0, 29, 40)
        bad[t, v] = value
    bad[200:230, :] = np.nan
    bad[300:310, 0] = np.inf
    bad[320:330, 1:] = -np.inf
    add("NaN and infinite logits", bad, None, **MID)
    add("NaN and infinite logits, blank 28", bad, None, blank=28, **SMALL)
    allnan = np.full((70, 5), np.nan, dtype=np.float32)
    add("every logit NaN", allnan, None, **SMALL)
    # arguments
    x = noisy(91, 500, 29, 0, 0.45, 6)
    for max_frames in (8, 16):
        for pad in (0, 5) if max_frames == 16 else (0, 2):
            for min_gap in (None, 1, 4):
                add(f"max_frames={max_frames} pad={pad} min_gap={min_gap}", x, None, max_frames=max_frames, min_gap=min_gap, pad=pad,
                    min_frames=(max_frames - 2 * pad) // 2 if pad else 2)
    add("margin 3.5", noisy(92, 500, 29, 0, 0.45, 6), None, max_frames=16, min_gap=4, margin=3.5, pad=2, min_frames=4)
    add("margin 25 (above every frame)", noisy(93, 200), None, max_frames=16, min_gap=4, margin=25.0, pad=2, min_frames=4)
    add("margin -30 (below every frame)", noisy(94, 200), None, max_frames=16, min_gap=4, margin=-30.0, pad=2, min_frames=4)
    return cases
