"""CPU checks of K33 (decode.ctc_segment_long): the banded float64 oracle against K26's unbanded one, the corridor rule, the cap on
near-tied boundaries over the diffuse case list, and the host side of the C ABI (no GPU anywhere)."""
import ctypes
import os

import numpy as np
import pytest

import _align_long_ref as AR
import _ctc_segment_long_ref as LR
import _ctc_segment_ref as SR

FLOATS = ("duration", "log_confidence", "start_margin", "end_margin", "word_log_confidence", "word_start_margin", "word_end_margin")
INTS = ("start", "end", "word_first", "word_count", "word_start", "word_end")
BASE = ((1, 1, 2), (2, 1, 29), (17, 5, 29), (63, 20, 71), (65, 32, 128), (129, 40, 29), (300, 37, 29))


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


@pytest.mark.parametrize("T,L,V", BASE)
def test_unbanded_corridor_is_k26(T, L, V):
    """lo = 0 and band >= n: every field of the banded oracle equals _ctc_segment_ref.segment_one's"""
    x, labels = SR.parity_case(T, L, V)
    band = 64 * ((2 * L + 1 + 63) // 64)
    for r in range(len(SR.SCALES)):
        ref = SR.segment_one(x[r], labels[r])
        got = LR.segment_one_banded(x[r], labels[r], np.zeros((T + 15) // 16, np.int64), band)
        assert got["feasible"] == ref["feasible"]
        if not ref["feasible"]:
            continue
        assert abs(got["log_prob"] - ref["log_prob"]) <= 1e-12 * max(1.0, abs(ref["log_prob"]))
        for k in FLOATS:
            assert np.allclose(got[k], ref[k], rtol=1e-12, atol=1e-12), k
        for k in INTS:
            assert np.array_equal(got[k], ref[k]), k


def masked_full_lattice(x, labels, lo, W, blank=0):
    """The definition, written out on the whole [T, n] lattice: K26's recursions with alpha and beta set to zero at the dead states"""
    lp = SR.log_softmax(x)
    T, L = len(x), len(labels)
    n = 2 * L + 1
    z = np.full(n, blank, np.int64)
    z[1::2] = labels
    em = lp[:, z]
    skip = np.zeros(n, bool)
    skip[3::2] = z[3::2] != z[1:-2:2]
    skip_out = np.zeros(n, bool)
    skip_out[:n - 2] = skip[2:]
    s = np.arange(n)[None]
    first = np.repeat(np.asarray(lo), 16)[:T, None]
    live = (s >= first) & (s < first + W)
    alpha, beta = np.full((T, n), SR.NEG), np.full((T, n), SR.NEG)
    alpha[0, :2] = em[0, :2]
    alpha[0, ~live[0]] = SR.NEG
    for t in range(1, T):
        a = alpha[t - 1]
        enter = np.logaddexp(SR._shift(a, 1), np.where(skip, SR._shift(a, 2), SR.NEG))
        alpha[t] = np.where(live[t], em[t] + np.logaddexp(a, enter), SR.NEG)
    logp = np.logaddexp(alpha[-1, -1], alpha[-1, -2])
    beta[-1, -2:] = 0.0
    beta[-1, ~live[-1]] = SR.NEG
    for t in range(T - 2, -1, -1):
        bt = em[t + 1] + beta[t + 1]
        leave = np.logaddexp(SR._shift(bt, -1), np.where(skip_out, SR._shift(bt, -2), SR.NEG))
        beta[t] = np.where(live[t], np.logaddexp(bt, leave), SR.NEG)
    gamma = np.exp(alpha + beta - logp)
    return logp, gamma[:, 1::2].sum(0), gamma.sum(1)


@pytest.mark.parametrize("T,L,W,step", ((100, 20, 16, 6), (100, 20, 8, 6), (70, 30, 16, 14), (64, 9, 6, 4)))
def test_oracle_is_the_masked_full_lattice(T, L, W, step):
    """the [T, W] storage changes nothing: windows that move by less than, and by nearly, their own width (a transition between a
    state that was live at t - 1 and one that is live at t counts, whatever happens to the window between the two frames)"""
    rng = np.random.default_rng(T + L + W)
    with np.errstate(all="ignore"):
        x = rng.standard_normal((T, 5))
        labels = rng.integers(1, 5, L)
        lo = LR.sanitise(np.arange((T + 15) // 16) * step, 2 * L + 1, W)
        assert len(set(lo)) >= 3
        logp, dur, total = masked_full_lattice(x, labels, lo, W)
        got = LR.segment_one_banded(x, labels, lo, W)
    assert np.isfinite(logp) and abs(got["log_prob"] - logp) < 1e-10 and np.allclose(got["duration"], dur, rtol=0, atol=1e-10)
    assert np.allclose(total, 1.0, atol=1e-10)          # the posterior of every frame sums to one inside the corridor
    assert got["log_prob"] < SR.segment_one(x, labels)["log_prob"]


def test_infeasible_and_empty_rows():
    z = np.zeros(1, np.int64)
    x = np.zeros((4, 5))
    for labels in ([1, 1, 1], [0], [7], [-1]):            # too few frames, the blank, outside [0, V)
        r = LR.segment_one_banded(x, labels, z, 64)
        assert not r["feasible"] and r["log_prob"] == -np.inf and not r["start"].any() and not r["duration"].any()
        assert len(r["word_first"]) == len(SR.word_spans(labels, 1))
    assert LR.segment_one_banded(np.zeros((0, 5)), [], z[:0], 64)["log_prob"] == 0.0
    assert not LR.segment_one_banded(np.zeros((0, 5)), [2], z[:0], 64)["feasible"]
    r = LR.segment_one_banded(x, [], z, 64)
    assert r["feasible"] and abs(r["log_prob"] - 4 * np.log(0.2)) < 1e-12


@pytest.mark.parametrize("T,L", ((400, 100), (401, 95), (700, 131), (700, 132), (1000, 300)))
def test_corridor_rule_on_planted_paths(T, L):
    """W = 64, n - W odd and even: the path lies inside the window at every frame, lo is even, monotone and within [0, hi], and the
    last window holds n - 1"""
    W, n = 64, 2 * L + 1
    for seed in range(3):
        _, _, path = AR.planted(seed, T, L, 29)
        lo = LR.corridor(path, T, L, W)
        assert lo.shape == ((T + 15) // 16,) and not (lo & 1).any() and (np.diff(lo) >= 0).all()
        assert lo.min() >= 0 and lo.max() <= LR.lo_max(n, W) and np.array_equal(lo, LR.sanitise(lo, n, W))
        per_frame = np.repeat(lo, 16)[:T]
        assert (path >= per_frame).all() and (path < per_frame + W).all()
        assert lo[-1] <= n - 1 < lo[-1] + W
        wide = LR.corridor(path, T, L, W, nblk=len(lo) + 3)                     # blocks beyond the row repeat the last value
        assert np.array_equal(wide[:len(lo)], lo) and (wide[len(lo):] == lo[-1]).all()
    assert {(n - W) & 1 for n in (2 * 95 + 1, 2 * 131 + 1)} == {1} and LR.lo_max(2 * 131 + 1, 64) == 200 and LR.lo_max(64, 64) == 0
    assert not LR.corridor(np.zeros(0, np.int32), 0, 5, 64, nblk=4).any()


def test_sanitise():
    n, W = 2 * 100 + 1, 64
    lo = LR.sanitise([5, 3, -7, 90, 40, 100000, 8], n, W)
    assert lo.tolist() == [4, 4, 4, 90, 90, 138, 138] and LR.lo_max(n, W) == 138


def test_planted_band_64_loses_nothing():
    """where the frames pin the path down, the corridor at band 64 holds all the mass that matters"""
    x, labels, _ = LR.planted_case(400, 100, 29)
    lo, _, ok = LR.viterbi_corridor(x[0], labels[0], 64)
    assert ok
    ref = SR.segment_one(x[0], labels[0])
    got = LR.segment_one_banded(x[0], labels[0], lo, 64)
    assert abs(got["log_prob"] - ref["log_prob"]) <= 1e-7 and got["log_prob"] <= ref["log_prob"] + 1e-12
    assert np.allclose(got["duration"], ref["duration"], atol=1e-7) and np.allclose(got["log_confidence"], ref["log_confidence"], atol=1e-7)
    assert np.array_equal(got["start"], ref["start"]) and np.array_equal(got["end"], ref["end"])


@pytest.fixture(scope="module")
def diffuse():
    """the banded oracle over the whole diffuse list, computed once: [(case, row, banded result)]"""
    out = []
    for T, L, V in LR.MOVING:
        x, labels = LR.diffuse_case(T, L, V)
        for r in range(len(SR.SCALES)):
            lo, _, ok = LR.viterbi_corridor(x[r], labels[r], LR.MOVING_BAND)
            assert ok
            out.append(((T, L, V), r, x[r], labels[r], LR.segment_one_banded(x[r], labels[r], lo, LR.MOVING_BAND)))
    return out


def test_banded_log_prob_is_a_lower_bound(diffuse):
    """the corridor holds a subset of the alignments; on the scale-0.1 rows it cuts mass that can be seen"""
    cut = []
    for (T, L, V), r, x, labels, got in diffuse:
        ref = SR.segment_one(x, labels)
        assert got["feasible"] and got["log_prob"] <= ref["log_prob"] + 1e-9 * abs(ref["log_prob"])
        if r == 0:
            cut.append(ref["log_prob"] - got["log_prob"])
    assert min(cut) > 1e-3, cut
    for T, L, V in LR.MOVING:                            # the planted list: a subset still, with next to nothing cut
        x, labels, _ = LR.planted_case(T, L, V, 6.0)
        lo, _, ok = LR.viterbi_corridor(x[0], labels[0], LR.MOVING_BAND)
        ref, got = SR.segment_one(x[0], labels[0]), LR.segment_one_banded(x[0], labels[0], lo, LR.MOVING_BAND)
        assert ok and got["feasible"] and ref["log_prob"] - 1e-6 <= got["log_prob"] <= ref["log_prob"] + 1e-9 * abs(ref["log_prob"])


def test_the_cap_on_undecided_boundaries(diffuse):
    """K26's condition 2 on the oracle alone: over the whole diffuse list at most 2 % of the boundaries lie nearer a tie than the
    decided margin of 2e-4 (single small cases may exceed it: the cap is on the aggregate)"""
    total = near = 0
    for _, _, _, _, got in diffuse:
        for k in ("start_margin", "end_margin", "word_start_margin", "word_end_margin"):
            total += got[k].size
            near += int((got[k] <= 2e-4).sum())
    assert total > 3000 and near <= 0.02 * total, (near, total)


def test_workspace_helper_and_limits(lib):
    f = lib.v100_ctc_segment_long_workspace_bytes
    assert f.restype is ctypes.c_longlong and lib.v100_ctc_segment_long_block() == LR.B16 == 16

    def up16(v):
        return (v + 15) & ~15
    for B, T, L, W in ((1, 1, 0, 64), (3, 300, 37, 128), (4, 90000, 25000, 256), (1, 1 << 20, 1 << 19, 1024)):
        nb = (T + 15) // 16
        assert f(B, T, L, W) == 12 * B * T * (W // 2) + up16(8 * B * nb) + up16(4 * B * nb) + up16(4 * B * L)
    assert f(1, 90000, 25000, 256) == 138240000 + up16(8 * 5625) + up16(4 * 5625) + 100000              # 138 MB for 30 minutes
    assert f(1, 1 << 20, 1 << 19, 1024) > 6.4e9
    for bad in ((0, 10, 1, 64), (1, 0, 1, 64), (1, (1 << 20) + 1, 1, 64), (1, 10, -1, 64), (1, 10, (1 << 19) + 1, 64), (1, 10, 1, 0),
                (1, 10, 1, 32), (1, 10, 1, 96), (1, 10, 1, 1088), (1, 10, 1, -64)):
        assert f(*bad) == 0, bad


def test_argument_checks_come_before_the_device(lib):
    """status 3 for a NULL or partial pointer set, status 1 for a shape or argument outside the limits: both without a GPU"""
    one = ctypes.c_void_p(16)
    seg = lib.v100_ctc_segment_long

    def call(ptrs=None, words=(None,) * 6, B=1, T=10, V=5, L=3, band=64, blank=0):
        p = [one] * 12 if ptrs is None else ptrs             # logits in_len labels lab_len lo ws log_prob ok start end duration log_conf
        return seg(*p, *words, B, T, V, L, band, blank, 1, None)
    for i in (0, 2, 4, 5, 6, 7, 8, 9, 10, 11):
        p = [one] * 12
        p[i] = None
        assert call(p) == 3, i
    assert call(words=(one, one, one, None, one, one)) == 3
    for kw in (dict(B=0), dict(T=0), dict(T=(1 << 20) + 1), dict(L=-1), dict(L=(1 << 19) + 1), dict(V=1), dict(V=129), dict(blank=5),
               dict(blank=-1), dict(band=32), dict(band=100), dict(band=2048)):
        assert call(**kw) == 1, kw
        assert call(words=(one,) * 6, **kw) == 1, kw


def test_python_checks_need_no_gpu():
    import torch
    from voice100_amd import decode
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        decode.ctc_segment_long(torch.zeros(1, 4, 5), None, torch.ones(1, 2, dtype=torch.long), None)
    path = torch.from_numpy(AR.planted(5, 120, 50, 29)[2])[None]
    with pytest.raises(RuntimeError, match="band"):
        decode.ctc_corridor(path, None, 50, band=100)
    for lengths, Tb in ((None, 120), (torch.tensor([70]), 70), (torch.tensor([0]), 0)):
        masked = torch.where(torch.arange(120)[None] < Tb, path, torch.zeros_like(path))     # a path is 0 beyond its row's length
        lo = decode.ctc_corridor(masked, lengths, 50, band=64)
        assert lo.dtype == torch.int32 and lo.shape == (1, 8)
        assert np.array_equal(lo[0].numpy(), LR.corridor(path[0].numpy(), Tb, 50, 64, nblk=8))
    p2 = torch.from_numpy(np.stack([AR.planted(s, 400, 100, 29)[2] for s in range(2)]))
    lo = decode.ctc_corridor(p2, torch.tensor([400, 333]), torch.tensor([100, 83]), band=64)
    assert np.array_equal(lo[0].numpy(), LR.corridor(p2[0].numpy(), 400, 100, 64))
    assert np.array_equal(lo[1].numpy(), LR.corridor(p2[1].numpy(), 333, 83, 64, nblk=25))
