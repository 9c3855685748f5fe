"""Float64 host oracle of the DTW scores (K27, csrc/dtw.hip), in numpy, from the definition in include/voice100_hip.h:

    d(i,j) = sqrt(sum_{k >= skip} (x[i][k] - y[j][k])^2)
    C(0,0) = d(0,0), C(i,j) = d(i,j) + min(C(i-1,j-1), C(i-1,j), C(i,j-1)), predecessors outside the matrix absent, a tie to the
    first candidate in that order; the path is the backtrace from (n-1,m-1), reported forwards.

The inputs are the fp32 arrays the device gets, converted to float64.  Besides the scores a case reports its DECISION MARGIN: the
minimum over the cells of its path of (second-best predecessor - best predecessor) / C(i,j), cells with one predecessor skipped.  A
device whose every C is within a relative eps of the oracle's must take the oracle's path when the margin exceeds 2 eps."""
import math

import numpy as np


def local_distance(x, y, skip=0):
    """[n, m] float64 distances between the rows of x [n, D] and y [m, D] over the dimensions skip .. D-1, from differences."""
    x, y = np.asarray(x, np.float64)[:, skip:], np.asarray(y, np.float64)[:, skip:]
    ss = np.zeros((len(x), len(y)))
    for k in range(x.shape[1]):                          # one dimension at a time: no [n, m, D] temporary
        ss += (x[:, k, None] - y[None, :, k]) ** 2
    return np.sqrt(ss)


def dtw_matrix(d):
    """Cumulative costs C [n, m] and moves (0 diagonal, 1 up, 2 left) of the distance matrix d [n, m]; anti-diagonal sweep."""
    n, m = d.shape
    C = np.full((n + 1, m + 1), np.inf)                  # shifted by one: C[i + 1, j + 1] is C(i,j), row / column 0 are absent
    mv = np.zeros((n, m), np.int8)
    C[0, 0] = 0.0                                        # the virtual predecessor of (0,0), read by that cell alone
    for s in range(n + m - 1):
        i = np.arange(max(0, s - m + 1), min(n, s + 1))
        j = s - i
        cand = np.stack([C[i, j], C[i, j + 1], C[i + 1, j]])             # diagonal, up, left
        best = cand.argmin(0)                                            # the FIRST minimum: the tie rule
        C[i + 1, j + 1] = d[i, j] + cand[best, np.arange(len(i))]
        mv[i, j] = best
    return C[1:, 1:], mv


def backtrace(mv):
    n, m = mv.shape
    i, j, path = n - 1, m - 1, []
    while True:
        path.append((i, j))
        if i == 0 and j == 0:
            break
        k = 2 if i == 0 else (1 if j == 0 else mv[i, j])
        if k != 2:
            i -= 1
        if k != 1:
            j -= 1
    return path[::-1]


def margin(C, path):
    """min over the path's cells with three predecessors of (second best - best) / C(i,j); inf when there is no such cell."""
    out = np.inf
    for i, j in path:
        if i == 0 or j == 0:
            continue
        c = sorted((C[i - 1, j - 1], C[i - 1, j], C[i, j - 1]))
        if C[i, j] > 0:
            out = min(out, (c[1] - c[0]) / C[i, j])
        elif c[1] == c[0]:
            out = 0.0
    return out


def path_sums(path, f0x, f0y, f0_floor):
    """voiced, vuv_errors, f0_sq_cents, f0_sq_hz along the path."""
    if not path:
        return 0, 0, 0.0, 0.0
    p = np.asarray(path)
    fx, fy = np.asarray(f0x, np.float64)[p[:, 0]], np.asarray(f0y, np.float64)[p[:, 1]]
    floor = np.float64(np.float32(f0_floor))
    with np.errstate(invalid="ignore"):
        vx, vy = fx >= floor, fy >= floor                # a NaN is unvoiced
    both = vx & vy
    cents = 1200.0 * np.log2(fx[both] / fy[both])
    return int(both.sum()), int((vx != vy).sum()), float((cents ** 2).sum()), float(((fx[both] - fy[both]) ** 2).sum())


def score_pair(x, y, f0x=None, f0y=None, skip=0, f0_floor=30.0, dtw=True):
    """One pair, already cut to its lengths: {"cost", "path" [(i, j)], "path_len", "margin", "voiced", "vuv_errors", "f0_sq_cents",
    "f0_sq_hz"} (the last four 0 without f0 tracks)."""
    n, m = len(x), len(y)
    res = {"cost": 0.0, "path": [], "path_len": 0, "margin": np.inf, "voiced": 0, "vuv_errors": 0, "f0_sq_cents": 0.0, "f0_sq_hz": 0.0}
    if n == 0 or m == 0:
        return res
    if dtw:
        C, mv = dtw_matrix(local_distance(x, y, skip))
        path = backtrace(mv)
        res.update(cost=float(C[-1, -1]), path=path, margin=margin(C, path))
    else:
        p = min(n, m)
        xs, ys = np.asarray(x, np.float64)[:p, skip:], np.asarray(y, np.float64)[:p, skip:]
        path = [(i, i) for i in range(p)]
        res.update(cost=float(np.sqrt(((xs - ys) ** 2).sum(-1)).sum()), path=path)
    res["path_len"] = len(path)
    if f0x is not None:
        v, e, c, h = path_sums(path, f0x, f0y, f0_floor)
        res.update(voiced=v, vuv_errors=e, f0_sq_cents=c, f0_sq_hz=h)
    return res


def score_batch(x, x_len, y, y_len, f0x=None, f0y=None, skip=0, f0_floor=30.0, dtw=True):
    """Rows of padded batches; lengths clamp to [0, width] (None: full width).  A list of score_pair results."""
    out = []
    for b in range(len(x)):
        n = x.shape[1] if x_len is None else min(max(int(x_len[b]), 0), x.shape[1])
        m = y.shape[1] if y_len is None else min(max(int(y_len[b]), 0), y.shape[1])
        out.append(score_pair(x[b, :n], y[b, :m], None if f0x is None else f0x[b, :n], None if f0y is None else f0y[b, :m], skip,
                              f0_floor, dtw))
    return out


def totals_of(rows):
    """[pairs, cost, voiced, vuv_errors, f0_sq_cents, f0_sq_hz] summed over score_pair results."""
    return [float(sum(r[k] for r in rows)) for k in ("path_len", "cost", "voiced", "vuv_errors", "f0_sq_cents", "f0_sq_hz")]


def rates_of(totals, utterances):
    """What SynthesisScore.compute() must return for these totals."""
    pairs, cost, voiced, vuv, cents, hz = totals
    nan = float("nan")
    return {"mcd": 10.0 / math.log(10.0) * math.sqrt(2.0) * cost / pairs if pairs > 0 else nan,
            "f0_rmse_cents": math.sqrt(cents / voiced) if voiced > 0 else nan,
            "f0_rmse_hz": math.sqrt(hz / voiced) if voiced > 0 else nan, "vuv_error": vuv / pairs if pairs > 0 else nan,
            "frames": int(pairs), "voiced_frames": int(voiced), "utterances": utterances}


def brute_force(d):
    """Every monotone path from (0,0) to (n-1,m-1) with steps (1,1), (1,0), (0,1), each summed from its start: the least cost and
    the list of the paths that reach it."""
    n, m = d.shape
    best, best_paths = np.inf, []

    def walk(i, j, cost, path):
        nonlocal best, best_paths
        cost = cost + d[i, j]
        path = path + [(i, j)]
        if i == n - 1 and j == m - 1:
            if cost < best:
                best, best_paths = cost, [path]
            elif cost == best:
                best_paths.append(path)
            return
        if i + 1 < n and j + 1 < m:
            walk(i + 1, j + 1, cost, path)
        if i + 1 < n:
            walk(i + 1, j, cost, path)
        if j + 1 < m:
            walk(i, j + 1, cost, path)
    walk(0, 0, 0.0, [])
    return best, best_paths


def tie_rule_path(paths):
    """Of several cheapest paths, the one the definition's backtrace takes: decided from the END, at every cell the diagonal
    predecessor before the upper one before the left one, among those that some remaining path uses."""
    paths = [list(p) for p in paths]
    k = 1                                                # cells from the end that all remaining paths share
    while len(paths) > 1:
        i, j = paths[0][-k]
        for pred in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):
            keep = [p for p in paths if len(p) > k and p[-k - 1] == pred]
            if keep:
                paths = keep
                break
        k += 1
    return paths[0]
