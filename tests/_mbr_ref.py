"""The float64 oracle of decode.mbr_nbest (K35, csrc/mbr.hip), its bounds and its case list.

The oracle shares nothing with the kernels' trimming or hashing: a row is split into tuples in plain Python (a token is the tuple of a
word's ids, or the 1-tuple of an id at the id level), distances are the textbook Levenshtein recurrence over whole rows (row-vectorised
numpy for long rows, on dictionary-numbered tokens), the softmax is math.exp in float64, and the order is a stable sort on the
float32-rounded risk, absent hypotheses (score -inf or NaN) behind in the given order.

Bounds, derived and not tuned.  The device forms the posterior p and the risk R in fp64 -- 2^-53 relative per operation over at most
64 terms, all of one sign, so about 2^-46 relative in all: negligible -- and stores fp32, which rounds by at most 2^-24 relative (2^-150
absolute in the denormal range).  The bounds asked are twice that, with a denormal floor:
    |post - p| <= 2^-23 p + 2^-149,    |risk - R| <= 2^-23 R + 2^-149,    |expected_len - E| <= 2^-23 E + 2^-149.
Every integer output (dist, ref_dist, ref_n, n_tokens, order) is EQUAL.  `order` is decided by the float32-rounded risk, so the
comparison is exact only where two risks of an utterance are either equal in float64 or further apart than the rounding can move them:
well_separated() checks that on the case list (tests/test_mbr_cpu.py), as K34's list is checked."""
import math

import numpy as np

SEP = 1
I64_MAX, I64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def bound(x):
    """twice the fp32 rounding of a value stored from fp64, with a denormal floor"""
    return 2.0 ** -23 * np.abs(np.asarray(x, dtype=np.float64)) + 2.0 ** -149


def present(score) -> bool:
    return bool(score > -math.inf)                       # NaN compares false: absent


def split_tokens(row, n, sep):
    """the tokens of row[:n]: 1-tuples of ids with sep=None, else the tuples of the maximal runs of ids != sep"""
    row = [int(v) for v in row[:max(n, 0)]]
    if sep is None:
        return [(v,) for v in row]
    out, cur = [], []
    for v in row:
        if v == sep:
            if cur:
                out.append(tuple(cur))
            cur = []
        else:
            cur.append(v)
    if cur:
        out.append(tuple(cur))
    return out


def levenshtein(a, b) -> int:
    """unit costs, whole rows; textbook for small tables, one numpy row a step for long ones"""
    a, b = list(a), list(b)
    n, m = len(a), len(b)
    if n == 0 or m == 0:
        return max(n, m)
    if n * m <= 1 << 14:
        prev = list(range(m + 1))
        for i in range(1, n + 1):
            cur = [i] + [0] * m
            for j in range(1, m + 1):
                cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
            prev = cur
        return prev[m]
    number = {}
    an = np.array([number.setdefault(t, len(number)) for t in a], dtype=np.int64)
    bn = np.array([number.setdefault(t, len(number)) for t in b], dtype=np.int64)
    idx = np.arange(m + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(1, n + 1):
        cur = np.empty(m + 1, dtype=np.int64)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (bn != an[i - 1]))
        prev = np.minimum.accumulate(cur - idx) + idx    # cur[j] = min over k <= j of cur[k] + (j - k): the insertions from the left
    return int(prev[m])


def oracle(ids, lens, scores, sep=SEP, scale=1.0, ref=None, ref_len=None):
    ids, lens, scores = np.asarray(ids), np.asarray(lens), np.asarray(scores, dtype=np.float32)
    B, N, T = ids.shape
    out = {"dist": np.full((B, N, N), -1, dtype=np.int32), "n_tokens": np.zeros((B, N), dtype=np.int32),
           "posterior": np.zeros((B, N)), "risk": np.full((B, N), math.inf), "order": np.zeros((B, N), dtype=np.int32),
           "expected_len": np.zeros(B), "ref_dist": None, "ref_n": None}
    if ref is not None:
        out["ref_dist"], out["ref_n"] = np.full((B, N), -1, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for b in range(B):
        here = [present(scores[b, i]) for i in range(N)]
        toks = [split_tokens(ids[b, i], min(max(int(lens[b, i]), 0), T), sep) if here[i] else [] for i in range(N)]
        for i in range(N):
            out["n_tokens"][b, i] = len(toks[i])
            for j in range(i, N):
                if here[i] and here[j]:
                    out["dist"][b, i, j] = out["dist"][b, j, i] = 0 if i == j else levenshtein(toks[i], toks[j])
        if ref is not None:
            rt = split_tokens(ref[b], min(max(int(ref_len[b]), 0), ref.shape[1]), sep)
            out["ref_n"][b] = len(rt)
            for i in range(N):
                if here[i]:
                    out["ref_dist"][b, i] = levenshtein(toks[i], rt)
        live = [i for i in range(N) if here[i]]
        if live:
            s_max = max(float(scores[b, i]) for i in live)
            e = {i: math.exp(0.0 if (float(scores[b, i]) == s_max or scale == 0.0) else scale * (float(scores[b, i]) - s_max)) for i in live}
            z = 0.0
            for i in live:
                z += e[i]
            for i in live:
                out["posterior"][b, i] = e[i] / z
            for i in live:
                r = 0.0
                for j in live:
                    if j != i:
                        r += out["posterior"][b, j] * float(out["dist"][b, i, j])
                out["risk"][b, i] = r
            el = 0.0
            for j in live:
                el += out["posterior"][b, j] * float(len(toks[j]))
            out["expected_len"][b] = el
        key = out["risk"][b].astype(np.float32)
        ranked = sorted(live, key=lambda i: key[i])      # sorted() is stable: equal keys keep the given order
        out["order"][b] = ranked + [i for i in range(N) if not here[i]]
    return out


def well_separated(ref):
    """[] if, in every utterance, two present risks are equal in float64 or differ by more than four times the bound of the larger"""
    bad = []
    for b in range(ref["risk"].shape[0]):
        r = np.sort(ref["risk"][b][np.isfinite(ref["risk"][b])])
        for lo, hi in zip(r[:-1], r[1:]):
            if lo != hi and hi - lo <= 4 * bound(hi):
                bad.append((b, float(lo), float(hi)))
    return bad


def pack(utts, T=None):
    """utts: B lists of N rows (lists of ids) -> ids [B, N, T] int64 zero padded, lens [B, N] int32"""
    B, N = len(utts), len(utts[0])
    T = T or max(1, max(len(r) for u in utts for r in u))
    ids, lens = np.zeros((B, N, T), dtype=np.int64), np.zeros((B, N), dtype=np.int32)
    for b, u in enumerate(utts):
        assert len(u) == N
        for i, r in enumerate(u):
            ids[b, i, :len(r)] = r
            lens[b, i] = len(r)
    return ids, lens


def words(*ws, lead=0, trail=0, gap=1):
    """ids of the words ws (tuples or ints) with `gap` separators between them, `lead` before and `trail` after"""
    out = [SEP] * lead
    for k, w in enumerate(ws):
        if k:
            out += [SEP] * gap
        out += list(w) if isinstance(w, (tuple, list)) else [w]
    return out + [SEP] * trail


def log_scores(p):
    return np.log(np.asarray(p, dtype=np.float64)).astype(np.float32)


def middles_rows(rng, level):
    """rows with a common prefix of 3 and a common suffix of 2 tokens round middles of 129, 1, 64, 63, 128, 65 and 40 tokens, in
    that order, so that the longer middle is the first row of some pairs and the second of others; the first and last token of every
    middle differ from the neighbours', so that the trimming stops exactly there"""
    rows = []
    for k, n in enumerate((129, 1, 64, 63, 128, 65, 40)):
        mid = rng.integers(20, 24, size=n).tolist()
        mid[0], mid[-1] = 30 + k, (40 + k if n > 1 else 30 + k)
        toks = [11, 12, 13] + mid + [14, 15]
        rows.append(toks if level == "id" else words(*[(t, t + 1) if t % 3 == 0 else (t,) for t in toks]))
    return rows


def flip_case():
    """posteriors 0.4 / 0.3 / 0.3: the second and third are one word apart and both four words from the first, so the expected error of
    the first is 0.6 * 4 = 2.4 and of the second 0.4 * 4 + 0.3 = 1.9: the MBR choice is not the one with the best score"""
    ids, lens = pack([[words(5, 6, 7, 8), words(15, 16, 17, 18), words(15, 16, 17, 19)]])
    return ids, lens, log_scores([[0.4, 0.3, 0.3]])


def case_list():
    """[(name, ids, lens, scores, kw)]; kw: sep (None: the id level), scale, ref, ref_len"""
    rng = np.random.default_rng(35)
    inf, nan = math.inf, math.nan
    f32 = lambda a: np.asarray(a, dtype=np.float32)      # noqa: E731
    cases = []

    def add(name, utts, scores, T=None, lens=None, **kw):
        ids, ln = pack(utts, T)
        if lens is not None:
            ln = np.asarray(lens, dtype=np.int32)
        if "ref" in kw:
            r, rl = pack([[row] for row in kw["ref"]], kw.pop("Tr", None))
            kw["ref"], kw["ref_len"] = r[:, 0], np.asarray(kw.get("ref_len", rl[:, 0]), dtype=np.int32)
        cases.append((name, ids, ln, f32(scores), kw))

    def draws(B, N):
        return np.sort(rng.uniform(-9.0, -1.0, size=(B, N)))[:, ::-1].copy()

    a, bb, c, d = (5, 6), (7,), (8, 9, 10), (11,)
    add("N = 1", [[words(a, bb)]], [[-2.0]])
    add("N = 2", [[words(a, bb, c), words(a, c)]], [[-1.0, -1.5]])
    add("N = 3", [[words(a, bb, c), words(a, c), words(d, c, c)]], [[-1.0, -1.5, -1.75]])
    add("T = 1", [[[5], [SEP], [6], [5]]], [[-1.0, -1.25, -2.0, -3.0]])
    add("T = 1, id level", [[[5], [SEP], [6], [5]]], [[-1.0, -1.25, -2.0, -3.0]], sep=None)
    add("B = 3, a pattern a row", [
        [words(a, bb, c, d), words(a, bb, c), words(a, c, d), words(bb, bb)],
        [words(c), [], words(c, c), words(d, c)],
        [words(a, a, a, a, a), words(a, a, a, a), words(a, a, a), words(a, a, a, a, a, a)]],
        [[-1.0, -1.1, -2.0, -4.0], [-0.5, -inf, -0.75, -3.0], [-3.0, -1.0, -inf, -inf]])
    trims = [[2, 3, 4, 5, 6], [2, 3, 4, 5, 6], [2, 3, 4], [4, 5, 6], [7, 7, 7], [7, 7], [8, 9, 8, 9], [8, 9], [3, 3, 4, 5, 6],
             [2, 3, 4, 5, 3], [], [9]]
    add("trimming, id level", [trims], draws(1, len(trims)), sep=None)
    add("trimming, word level", [[words(*[(t, 20 + t) for t in r]) for r in trims]], draws(1, len(trims)))
    add("size switches, id level", [middles_rows(rng, "id")], draws(1, 7), sep=None, scale=0.5)
    add("size switches, word level", [middles_rows(rng, "word")], draws(1, 7), scale=0.5)
    odd = [words(a, bb, c), words(a, bb, c, lead=2, trail=3, gap=2), [SEP, SEP, SEP], words((5, 7), bb, c), words((5, 6, 6), bb, c),
           words((5, 5), (5, 5, 5), (5,)), words((5, 5, 5), (5, 5), (5,)), words((I64_MAX, I64_MIN), (I64_MIN,), (-1,), (0,)),
           words((I64_MAX, I64_MIN), (I64_MAX,), (-1,), (0,))]
    add("word oddities", [odd], draws(1, len(odd)))
    add("the separator is an id at the id level", [odd], draws(1, len(odd)), sep=None)
    add("another separator", [[[5, 0, 6, 0, 0, 7], [5, 0, 6, 7], [0, 0, 5]]], [[-1.0, -2.0, -2.5]], sep=0)
    add("absent in the middle and at the end, NaN, a row with none", [
        [words(a, bb), words(a, c), words(c, c, c), words(a), words(d, d), words(a, bb, c)],
        [words(a), words(bb), words(c), words(d), words(a), words(bb)]],
        [[-1.0, -inf, -1.5, nan, -2.0, -inf], [-inf, nan, -inf, -inf, nan, -inf]])
    add("lens above T and negative", [[words(a, bb, c), words(a, bb), words(a, c, c), words(d)]], draws(1, 4), T=12,
        lens=[[15, -3, 1 << 30, -(1 << 31)]])
    post = [[words(a, bb, c), words(a, bb), words(a, c, c), words(d), words(a, bb, c, d)]]
    add("scale 0", post, [[-1.0, -7.0, -30.0, -2.0, -900.0]], scale=0.0)
    add("equal scores", post, [[-3.5] * 5])
    add("scores 10^4 apart", post, [[-1.0, -10001.0, -20001.0, -1.0e4, -3.0e4]])
    add("scale 2", post, draws(1, 5), scale=2.0)
    add("scale 0.25", post, draws(1, 5), scale=0.25)
    fi, fl, fs = flip_case()
    cases.append(("the MBR choice is not rank 0", fi, fl, fs, {}))
    base = rng.integers(2, 8, size=12).tolist()
    many = []
    for _ in range(64):
        row = list(base)
        for _ in range(int(rng.integers(0, 4))):
            row[int(rng.integers(0, 12))] = int(rng.integers(1, 8))
        many.append(row[:int(rng.integers(9, 13))])
    add("N = 64", [many], draws(1, 64))
    add("N = 64, id level", [many], draws(1, 64), sep=None)
    add("a reference", [[words(a, bb, c), words(a, c), words(d, c, c)]] * 2, [[-1.0, -1.5, -inf]] * 2, ref=[words(a, bb, c, d), words(c)])
    add("an empty reference, Tr != T", [[words(a, bb, c), [], words(d, c, c)]], [[-1.0, -1.5, -2.5]], ref=[[]], Tr=3)
    add("a wider reference, id level", [[[2, 3, 4], [2, 4], [3]]], [[-1.0, -1.5, -2.5]], ref=[[2, 3, 3, 4, 5, 6, 7, 8]], sep=None,
        ref_len=[40])
    add("a reference of separators", [[words(a), [SEP], []]], [[-1.0, -1.5, -2.5]], ref=[[SEP, SEP]])
    return cases


FIELDS = ("ids", "lens", "scores", "risk", "posterior", "n_tokens", "order", "dist", "expected_len", "ref_dist", "ref_n")


def check(name, got, ref, ids, lens, scores):
    """what differs between a result (numpy arrays by MBR field name) and the oracle's: ([messages], {field: worst error / bound})"""
    bad, worst = [], {}
    B, N, T = ids.shape
    rows, order = np.arange(B)[:, None], got["order"].astype(np.int64)
    for k in ("order", "dist", "ref_dist", "ref_n"):
        if (ref[k] is None) != (got[k] is None) or (ref[k] is not None and not np.array_equal(got[k], ref[k])):
            bad.append(f"{name}: {k} differs from the oracle")
    if bad:
        return bad, worst
    if not np.array_equal(got["n_tokens"], ref["n_tokens"][rows, order]):
        bad.append(f"{name}: n_tokens differs from the oracle")
    if not (np.array_equal(got["ids"], ids[rows, order]) and np.array_equal(got["lens"], lens[rows, order])
            and np.array_equal(got["scores"].view(np.int32), scores[rows, order].view(np.int32))):
        bad.append(f"{name}: ids, lens or scores are not the gather by order")
    for k, want in (("posterior", ref["posterior"][rows, order]), ("risk", ref["risk"][rows, order]), ("expected_len", ref["expected_len"])):
        g = got[k].astype(np.float64)
        far = np.isinf(want)
        if not np.array_equal(g[far], want[far]):
            bad.append(f"{name}: {k} is not +inf where there is no hypothesis")
        err = np.abs(g[~far] - want[~far]) / bound(want[~far])
        worst[k] = float(np.max(err, initial=0.0))
        if not np.all(err <= 1.0):                       # (a NaN fails here too)
            bad.append(f"{name}: {k} is {worst[k]:.3g} bounds away")
    # the order from the outputs alone: the stable argsort of the returned fp32 risk, absent hypotheses (+inf) last in the given order
    key = np.empty((B, N), dtype=np.float32)
    key[rows, order] = got["risk"]
    if not np.array_equal(np.argsort(key, axis=1, kind="stable"), order):
        bad.append(f"{name}: order is not the stable argsort of the returned risk")
    d = got["dist"]
    if not (np.array_equal(d, d.transpose(0, 2, 1)) and np.all(np.diagonal(d, axis1=1, axis2=2) <= 0)):
        bad.append(f"{name}: dist is not symmetric with a zero diagonal")
    live = np.isfinite(ref["risk"])
    for b in range(B):
        if live[b].any():
            chosen, least = ref["risk"][b, order[b, 0]], ref["risk"][b][live[b]].min()
            if chosen - least > 2 * bound(least):
                bad.append(f"{name}: the oracle's risk of the chosen hypothesis, {chosen}, is not its minimum, {least}")
    return bad, worst


def write_cases(f, cases):
    """the case file of tools/mbr_host.cpp"""
    import struct
    f.write(struct.pack("<i", len(cases)))
    for _, ids, lens, scores, kw in cases:
        B, N, T = ids.shape
        ref, sep = kw.get("ref"), kw.get("sep", SEP)
        f.write(struct.pack("<5iqd", B, N, T, 0 if ref is None else ref.shape[1], 0 if sep is None else 1, 0 if sep is None else sep,
                            kw.get("scale", 1.0)))
        for a, dt in ((ids, "<i8"), (lens, "<i4"), (scores, "<f4")) + (() if ref is None else ((ref, "<i8"), (kw["ref_len"], "<i4"))):
            f.write(np.ascontiguousarray(a).astype(dt).tobytes())


def read_results(raw, cases):
    """the result file of tools/mbr_host.cpp -> a dict by MBR field name per case"""
    at, out = 0, []
    for _, ids, lens, scores, kw in cases:
        B, N, T = ids.shape
        has_ref = kw.get("ref") is not None
        got = {"ref_dist": None, "ref_n": None}
        layout = [("order", "<i4", (B, N)), ("n_tokens", "<i4", (B, N)), ("lens", "<i4", (B, N)), ("scores", "<f4", (B, N)),
                  ("risk", "<f4", (B, N)), ("posterior", "<f4", (B, N)), ("ids", "<i8", (B, N, T)), ("dist", "<i4", (B, N, N)),
                  ("expected_len", "<f4", (B,))] + ([("ref_dist", "<i4", (B, N)), ("ref_n", "<i4", (B,))] if has_ref else [])
        for k, dt, shape in layout:
            n = int(np.prod(shape))
            got[k] = np.frombuffer(raw, dtype=dt, count=n, offset=at).reshape(shape)
            at += n * np.dtype(dt).itemsize
        out.append(got)
    assert at == len(raw)
    return out
