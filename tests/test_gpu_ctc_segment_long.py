"""decode.ctc_segment_long (K33, csrc/ctc_segment_long.hip), decode.ctc_corridor and LongASRPipeline.whole(confidences=True) against
the banded float64 oracle of tests/_ctc_segment_long_ref.py (itself checked in tests/test_ctc_segment_long_cpu.py).

Tolerances.  Shapes inside K26's range (T <= 1100) are held to K26's recorded tolerances: log_prob 9e-5 relative to max(1, |log_prob|),
duration 2e-4 and log_confidence 5e-4 absolute, boundaries compared where the oracle's margin |cdf - 1/2| exceeds 2e-4.  Beyond it
(the exponent-range case of 3,000 frames and the case of 20,000) K26's rule is applied to what tools/bench_ctc_segment_long.py
measured (profiles/ctc_segment_long_bench.json): 8 x the largest error, rounded up to one digit; the decided margin is
max(8 x the duration error, 1e-5), under the cap of 1e-3."""
import math

import numpy as np
import pytest
import torch

import _ctc_segment_long_ref as LR
import _ctc_segment_ref as R
from voice100_amd import _native as N
from voice100_amd.decode import CTCLongSegments, ctc_align_long, ctc_corridor, ctc_segment_long
from voice100_amd.infer import LongASRPipeline

pytestmark = pytest.mark.gpu

K26_TOL = dict(logp=9e-5, dur=2e-4, conf=5e-4, margin=2e-4)
# measured on the device (tools/bench_ctc_segment_long.py, "errors"): the exponent-range case log_prob 3.7e-13, duration 8.4e-5,
# log_confidence 4.1e-4 (on values of -6,000); the 20,000-frame case log_prob 4.4e-8, duration 3.6e-7, log_confidence 2.5e-7
OVERFLOW_TOL = dict(logp=3e-12, dur=7e-4, conf=4e-3, margin=7e-4)
LONG_TOL = dict(logp=4e-7, dur=3e-6, conf=2e-6, margin=1e-5)
UNDECIDED_CAP = 0.02
FIELDS = CTCLongSegments._fields


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def to_np(out):
    return {k: v.cpu().numpy() for k, v in out._asdict().items() if v is not None}


def run(dev, x, lengths, labels, label_lengths, lo=None, band=64, path=None, blank=0, sep=1, twice=True):
    """Two calls (equal bits; two launches each with the word level); the fields as numpy arrays."""
    xt, lt = torch.from_numpy(np.asarray(x)).to(dev), torch.from_numpy(np.asarray(labels)).to(dev)
    il = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    ll = None if label_lengths is None else torch.tensor(label_lengths, dtype=torch.int32, device=dev)
    kw = dict(band=band, blank=blank, sep=sep)
    if lo is not None:
        kw["lo"] = torch.from_numpy(np.asarray(lo, np.int32)).to(dev)
    if path is not None:
        kw["path"] = torch.from_numpy(np.asarray(path, np.int32)).to(dev)
    before = N.launch_count()
    out = ctc_segment_long(xt, il, lt, ll, **kw)
    if lo is not None:
        assert N.launch_count() - before == (1 if sep is None else 2)
    if twice:
        again = ctc_segment_long(xt, il, lt, ll, **kw)
        for k, a, c in zip(FIELDS, out, again):
            assert (a is None and c is None) or torch.equal(bits(a), bits(c)), k
    return to_np(out)


def check(got, ref, tol=K26_TOL, cap=UNDECIDED_CAP):
    """Device fields against segment_batch_banded's: integers equal on the decided boundaries, floats within the tolerances, padding
    zero, infeasible rows as the contract says.  Returns the comparison's figures."""
    c = R.compare(got, ref, tol["margin"])
    print(c)
    assert c["wrong"] == 0, c
    assert c["undecided"] <= cap * max(c["boundaries"], 1), c
    assert c["log_prob_rel"] <= tol["logp"] and c["duration_abs"] <= tol["dur"] and c["log_confidence_abs"] <= tol["conf"], c
    feas = ref["feasible"]
    assert got["log_prob"].dtype == np.float64 and np.array_equal(got["ok"], feas.astype(np.int32))
    live = np.isfinite(ref["start_margin"])              # inside the row's labels
    assert np.all(got["log_prob"][~feas] == -np.inf)
    for k in ("start", "end", "duration", "log_confidence"):
        assert not got[k][~live].any(), k                # padding
    bad = live & ~feas[:, None]
    assert not got["start"][bad].any() and not got["end"][bad].any() and not got["duration"][bad].any()
    assert np.all(got["log_confidence"][bad] == -np.inf)
    if "word_first" in ref:
        assert np.array_equal(got["n_words"], ref["n_words"])
        assert np.array_equal(got["word_first"], ref["word_first"]) and np.array_equal(got["word_count"], ref["word_count"])
        wl = np.isfinite(ref["word_start_margin"])
        for k in ("word_start", "word_end", "word_log_confidence"):
            assert not got[k][~wl].any(), k
        wb = wl & ~feas[:, None]
        assert not got["word_start"][wb].any() and not got["word_end"][wb].any() and np.all(got["word_log_confidence"][wb] == -np.inf)
    ok = live & feas[:, None]                            # what holds for every feasible label, decided or not
    assert np.all(got["start"][ok] < got["end"][ok]) and np.all(got["log_confidence"][ok] <= 0)
    return c


def zeros_lo(B, T):
    return np.zeros((B, (T + 15) // 16), np.int32)


def band_for(L):
    return 64 * ((2 * L + 1 + 63) // 64)


@pytest.mark.parametrize("T", LR.EXACT_T)
def test_exact_form_equals_the_unbanded_oracle(cuda, T):
    """band >= n and lo = 0: K26's quantity, held to K26's oracle at K26's tolerances; the logit scales 0.1 / 3 / 10 are batch rows"""
    assert N.load().v100_ctc_segment_long_block() == 16
    tally = {"boundaries": 0, "undecided": 0}
    cases = [c for c in LR.EXACT if c[0] == T]
    assert cases
    for _, L, V in cases:
        x, labels = R.parity_case(T, max(L, 1), V)
        ll = None if L else [0, 0, 0]
        ref = R.segment_batch(x, None, labels, ll)
        c = check(run(cuda, x, None, labels, ll, lo=zeros_lo(3, T), band=band_for(L)), ref, cap=1.0)
        for k in tally:
            tally[k] += c[k]
    assert tally["undecided"] <= UNDECIDED_CAP * max(tally["boundaries"], 1), tally


def test_two_slots_a_thread_exact_form(cuda):
    """Band 1,024: ctc_segment_long_kernel<2>, a thread owns ring slots q and q + 256.  511 labels fill pairs 0..511, so the second
    slot's accumulators and skip bits are live in every thread; K26's seam case, K26's oracle, K26's tolerances."""
    T, L, V = 1030, 511, 29
    x, labels = R.parity_case(T, L, V)
    ref = R.segment_batch(x, None, labels, None)
    assert ref["feasible"].all() and band_for(L) == 1024
    check(run(cuda, x, None, labels, None, lo=zeros_lo(3, T), band=1024), ref)
    x, labels = R.parity_case(520, 300, 29)              # ... and a band of 640: 320 slots, so only threads 0..63 have a second one
    ref = R.segment_batch(x, None, labels, None)
    assert ref["feasible"].all() and band_for(300) == 640
    check(run(cuda, x, None, labels, None, lo=zeros_lo(3, 520), band=640), ref)


def test_two_slots_a_thread_moving_window(cuda):
    """Band 640 (H = 320 > 256) on 2 L + 1 = 1,401 states: the ring of 320 pairs wraps twice while the window walks from 0 to 762"""
    T, L, V, W = 1100, 700, 29, 640
    x, labels = LR.diffuse_case(T, L, V)
    lo = np.stack([LR.viterbi_corridor(x[r], labels[r], W)[0] for r in range(3)])
    ref = LR.segment_batch_banded(x, None, labels, None, lo, W)
    assert ref["feasible"].all() and lo.max() == LR.lo_max(2 * L + 1, W) == 762 and all(len(set(lo[r])) >= 20 for r in range(3))
    check(run(cuda, x, None, labels, None, lo=lo, band=W), ref, cap=0.1)


_MOVING = {}


def moving(T, L, V, kind):
    """(x [rows, T, V], labels, lo, paths, banded reference), computed once; the corridor comes from _align_long_ref.mirror's path"""
    key = (T, L, V, kind)
    if key not in _MOVING:
        x, labels = LR.diffuse_case(T, L, V) if kind == "diffuse" else LR.planted_case(T, L, V, 6.0)[:2]
        los, paths = [], []
        for r in range(len(x)):
            lo, path, ok = LR.viterbi_corridor(x[r], labels[r], LR.MOVING_BAND)
            assert ok
            los.append(lo)
            paths.append(path)
        lo = np.stack(los)
        _MOVING[key] = (x, labels, lo, np.stack(paths), LR.segment_batch_banded(x, None, labels, None, lo, LR.MOVING_BAND))
    return _MOVING[key]


@pytest.mark.parametrize("T,L,V", LR.MOVING)
def test_moving_window_diffuse(cuda, T, L, V):
    """band 64 against 2 L + 1 = 121 to 401 states: the ring wraps several times.  Every decided boundary equals the banded
    oracle's; on the scale-0.1 row the result is NOT the unbanded oracle's, so the mask is applied."""
    x, labels, lo, paths, ref = moving(T, L, V, "diffuse")
    assert lo.max() >= 2 * L + 1 - 64 and ref["feasible"].all()
    got = run(cuda, x, None, labels, None, lo=lo)
    check(got, ref, cap=0.1)
    unbanded = R.segment_one(x[0], labels[0])
    away = np.abs(got["duration"][0] - unbanded["duration"]).max()
    print("scale 0.1: duration differs from the unbanded oracle's by", away)
    assert away > 2 * K26_TOL["dur"]
    by_path = run(cuda, x, None, labels, None, path=paths, twice=False)          # ctc_corridor on the device: the same corridor
    for k in got:
        assert np.array_equal(got[k], by_path[k]), k


@pytest.mark.parametrize("T,L,V", LR.MOVING)
def test_moving_window_planted(cuda, T, L, V):
    x, labels, lo, _, ref = moving(T, L, V, "planted")
    c = check(run(cuda, x, None, labels, None, lo=lo), ref)
    assert c["undecided"] <= 0.005 * c["boundaries"]


def test_caller_supplied_and_hostile_corridors(cuda):
    T, L, V, W = 400, 100, 29, 64
    x, labels, _ = LR.planted_case(T, L, V, 3.0)
    n, nb = 2 * L + 1, (T + 15) // 16
    diagonal = (np.arange(nb) * 16 * (n - W) // (T - 16)).astype(np.int32)[None]               # a straight line from 0 to n - W
    ref = LR.segment_batch_banded(x, None, labels, None, diagonal, W)
    check(run(cuda, x, None, labels, None, lo=diagonal), ref, cap=0.1)
    rng = np.random.default_rng(3)
    hostile = diagonal + rng.integers(-9, 10, diagonal.shape).astype(np.int32)                  # odd, decreasing
    hostile[0, 3], hostile[0, 7], hostile[0, 11] = -2 ** 31, 7, 2 ** 31 - 1                     # ... below 0 and beyond n
    hostile[0, 12:] = np.where(np.arange(12, nb) % 2, 2 ** 30, -5)
    clean = LR.sanitise(hostile[0], n, W)[None]
    assert (hostile & 1).any() and (np.diff(hostile[0].astype(np.int64)) < 0).any() and hostile.max() > n and not np.array_equal(clean, hostile)
    got, want = run(cuda, x, None, labels, None, lo=hostile), run(cuda, x, None, labels, None, lo=clean)
    for k in got:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    ref = LR.segment_batch_banded(x, None, labels, None, hostile, W)
    assert not ref["feasible"][0]                        # it jumps to the end at block 11: nothing gets through
    check(got, ref)
    wander = diagonal + (rng.integers(-3, 4, diagonal.shape) * 2).astype(np.int32)              # a hostile corridor that stays feasible
    ref = LR.segment_batch_banded(x, None, labels, None, wander, W)
    assert ref["feasible"][0]
    check(run(cuda, x, None, labels, None, lo=wander), ref, cap=0.1)


def test_bounds_canaries_around_every_buffer(cuda):
    """The library called on views inside larger buffers, with a hostile corridor and a poisoned workspace: the canaries stay, and the
    poison (NaN bit patterns) changes no bit of the result"""
    rng = np.random.default_rng(26)
    B, T, V, Lmax, W, PAD = 3, 300, 29, 90, 64, 64
    NW, NB = (Lmax + 1) // 2, (T + 15) // 16
    lens, ll = [300, 170, 0], [90, 41, 4]
    x = (rng.standard_normal((B, T, V)) * 3).astype(np.float32)
    labels = rng.integers(1, V, (B, Lmax)).astype(np.int64)
    lo = rng.integers(-50, 400, (B, NB)).astype(np.int32)
    lo[1] = LR.corridor(np.minimum(np.arange(T) // 2, 2 * 41), 170, 41, W, nblk=NB)
    il, lt = torch.tensor(lens, dtype=torch.int32, device=cuda), torch.tensor(ll, dtype=torch.int32, device=cuda)
    sizes = [("log_prob", B, torch.float64), ("ok", B, torch.int32), ("start", B * Lmax, torch.int32), ("end", B * Lmax, torch.int32),
             ("duration", B * Lmax, torch.float32), ("log_confidence", B * Lmax, torch.float32), ("word_first", B * NW, torch.int32),
             ("word_count", B * NW, torch.int32), ("word_start", B * NW, torch.int32), ("word_end", B * NW, torch.int32),
             ("word_log_confidence", B * NW, torch.float32), ("n_words", B, torch.int32)]

    def call(poison):
        nbytes = N.helper("v100_ctc_segment_long_workspace_bytes", B, T, Lmax, W)
        ws = torch.full((nbytes + 2 * PAD,), poison, dtype=torch.uint8, device=cuda)
        bufs = [torch.full((n + 2 * PAD,), -77, dtype=dt, device=cuda) for _, n, dt in sizes]
        views = [buf[PAD:PAD + n] for buf, (_, n, _) in zip(bufs, sizes)]
        N.call("v100_ctc_segment_long", torch.from_numpy(x).to(cuda), il, torch.from_numpy(labels).to(cuda), lt,
               torch.from_numpy(lo).to(cuda), ws[PAD:PAD + nbytes], *views, B, T, V, Lmax, W, 0, 1)
        torch.cuda.synchronize()
        for (name, n, _), buf in zip(sizes, bufs):
            assert bool((buf[:PAD] == -77).all()) and bool((buf[PAD + n:] == -77).all()), name
        assert bool((ws[:PAD] == poison).all()) and bool((ws[PAD + nbytes:] == poison).all())
        return {name: v.clone() for (name, _, _), v in zip(sizes, views)}

    a, c = call(0x5A), call(0xFF)                        # 0xFF..: NaNs and exponents of -1
    for name, _, _ in sizes:
        assert torch.equal(bits(a[name]), bits(c[name])), name
    got = {k: v.cpu().numpy().reshape(B, -1) if v.numel() != B else v.cpu().numpy() for k, v in a.items()}
    ref = LR.segment_batch_banded(x, lens, labels, ll, lo, W)
    assert ref["feasible"].tolist() == [False, True, False]
    check(got, ref, cap=0.1)


def test_transcript_edge_cases(cuda):
    """Repeated labels at a window edge, a run of separators across a window move, words that span more labels than a window holds"""
    T, L, V, W = 400, 100, 6, 64
    rng = np.random.default_rng(41)
    labels = rng.integers(2, V, (3, L)).astype(np.int64)
    labels[0, 10:80] = np.repeat(rng.integers(2, V, 35), 2)                   # pairs of equal labels all along: some at every edge
    labels[1, ::9] = 1
    labels[1, 30:38] = 1                                                       # a run of separators
    labels[2, 50] = 1                                                          # two words of 50 and 49 labels; a window holds 32
    x = np.zeros((3, T, V), np.float32)
    paths = []
    for r in range(3):
        n = 2 * L + 1
        dur = np.ones(n, np.int64) + rng.multinomial(T - n, np.full(n, 1.0 / n))
        path = np.repeat(np.arange(n), dur)
        ext = np.zeros(n, np.int64)
        ext[1::2] = labels[r]
        x[r] = rng.standard_normal((T, V))
        x[r, np.arange(T), ext[path]] += 4.0
        paths.append(path)
    lo = np.stack([LR.corridor(p, T, L, W) for p in paths])
    assert all(len(set(lo[r])) >= 8 for r in range(3))
    ref = LR.segment_batch_banded(x, None, labels, None, lo, W)
    assert ref["feasible"].all() and ref["n_words"][2] == 2 and ref["word_count"][2].max() == 50
    check(run(cuda, x, None, labels, None, lo=lo), ref, cap=0.1)
    ref5 = LR.segment_batch_banded(x, None, labels, None, lo, W, blank=0, sep=5)
    check(run(cuda, x, None, labels, None, lo=lo, sep=5), ref5, cap=0.1)
    ns = run(cuda, x, None, labels, None, lo=lo, sep=None)                     # no word level: the label level is the same bits
    base = run(cuda, x, None, labels, None, lo=lo)
    assert "word_first" not in ns and all(np.array_equal(ns[k], base[k]) for k in FIELDS[:6])


def test_batch_rows_and_infeasible_rows(cuda):
    rng = np.random.default_rng(22)
    T, V, L, W = 100, 29, 40, 64
    x = (rng.standard_normal((8, T, V)) * 3).astype(np.float32)
    labels = rng.integers(1, V, (8, L)).astype(np.int64)
    labels[3, 5], labels[4, 7], labels[5, 2] = 0, V, -1                        # a label equal to blank, >= V, < 0
    lens = [100, 0, 155, 17, 100, -3, 100, 60]                                 # zero-length rows, lengths above T and below 0
    ll = [40, 5, 70, 20, 40, 0, 40, 12]                                        # row 3: 17 frames for 20 labels; row 5: T_b = 0 and L_b = 0
    paths = np.stack([np.minimum(np.arange(T) * (2 * max(min(l_, L), 1) + 1) // max(min(max(n_, 0), T), 1), 2 * L) for n_, l_ in zip(lens, ll)])
    lo = np.stack([LR.corridor(paths[b], min(max(lens[b], 0), T), min(ll[b], L), W, nblk=7) for b in range(8)])
    lo[6] = 0                                                                  # a corridor that misses the end: n = 81 > 64
    ref = LR.segment_batch_banded(x, lens, labels, ll, lo, W)
    assert ref["feasible"].tolist() == [True, False, True, False, False, True, False, True]
    got = run(cuda, x, lens, labels, ll, lo=lo)
    check(got, ref, cap=0.1)
    assert got["log_prob"][5] == 0.0 and got["ok"][5] == 1 and got["ok"][1] == 0 and got["n_words"][6] == ref["n_words"][6] > 0
    full = LR.segment_batch_banded(x, None, labels[:, :12], None, lo * 0, W)   # lengths=None: every row T frames and 12 labels
    check(run(cuda, x, None, labels[:, :12], None, lo=lo * 0), full, cap=0.1)
    dev_x, dev_l = torch.from_numpy(x).to(cuda), torch.from_numpy(labels).to(cuda)
    empty = ctc_segment_long(dev_x, None, dev_l[:, :0], None, lo=torch.zeros((8, 7), dtype=torch.int32, device=cuda))
    assert empty.start.shape == (8, 0) and empty.word_first.shape == (8, 0) and not empty.n_words.any() and bool(empty.ok.all())
    want = torch.log_softmax(dev_x.double(), -1)[:, :, 0].sum(1)
    assert torch.allclose(empty.log_prob, want, rtol=K26_TOL["logp"], atol=0)
    before = N.launch_count()
    for bad in (dict(blank=29), dict(blank=-1), dict(band=32), dict(band=96), dict(band=2048)):
        with pytest.raises(RuntimeError, match="limits"):
            ctc_segment_long(dev_x, None, dev_l, None, **bad)
    with pytest.raises(RuntimeError):
        ctc_segment_long(dev_x, None, dev_l[:3], None)
    with pytest.raises(RuntimeError, match="lo must be"):
        ctc_segment_long(dev_x, None, dev_l, None, lo=torch.zeros((8, 6), dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError, match="not both"):
        ctc_segment_long(dev_x, None, dev_l, None, lo=torch.zeros((8, 7), dtype=torch.int32, device=cuda),
                         path=torch.zeros((8, T), dtype=torch.int32, device=cuda))
    assert N.launch_count() == before


def test_exponent_range(cuda):
    """The transcript's labels lie 6,000 nats below every frame's best class: 8,656 bits a frame, 2.6e7 over the 3,000 frames, past
    the 2^24 that an fp32 exponent holds exactly"""
    x, labels = LR.overflow_case()
    T = x.shape[1]
    lo = zeros_lo(1, T)
    ref = LR.segment_batch_banded(x, None, labels, None, lo, 64)
    assert ref["feasible"][0] and -ref["log_prob"][0] / math.log(2) > 2 ** 24
    got = run(cuda, x, None, labels, None, lo=lo)
    check(got, ref, tol=OVERFLOW_TOL, cap=0.2)
    # the labels' durations sum to T_b less the blanks' share, as the oracle's do
    assert ref["duration"][0].sum() < T - 1 and abs(got["duration"][0].sum() - ref["duration"][0].sum()) <= labels.shape[1] * OVERFLOW_TOL["dur"]


def test_one_long_case(cuda):
    T, L, V, W, nats = LR.LONG
    x, labels, path = LR.planted_case(T, L, V, nats)
    lo = LR.corridor(path, T, L, W)[None]
    ref = LR.segment_batch_banded(x, None, labels, None, lo, W)
    assert ref["feasible"][0] and lo.max() == LR.lo_max(2 * L + 1, W)
    c = check(run(cuda, x, None, labels, None, lo=lo, band=W, twice=False), ref, tol=LONG_TOL)
    assert c["boundaries"] >= 2 * L and c["undecided"] == 0


def test_default_path_runs_the_aligner(cuda, monkeypatch):
    """Neither path nor lo: ctc_align_long on the log-softmax of the same logits at align_band, the corridor from its path; equal to
    the explicit path= call bit for bit.  A row the aligner loses comes back with ok = 0."""
    T, L, V = 400, 100, 29
    xs, ls = zip(*(LR.planted_case(T, L, V, 6.0, seed=s)[:2] for s in (1, 2)))
    x, labels = np.concatenate(xs), np.concatenate(ls)
    x[1, :200] = np.random.default_rng(9).standard_normal((200, V)) * 0.1      # row 1: the first half says nothing
    xt, lt = torch.from_numpy(x).to(cuda), torch.from_numpy(labels).to(cuda)
    il, ll = torch.tensor([400, 390], dtype=torch.int32, device=cuda), torch.tensor([100, 96], dtype=torch.int32, device=cuda)
    out = ctc_segment_long(xt, il, lt, ll, band=64)
    al = ctc_align_long(torch.log_softmax(xt, -1), lt, il, ll, band=2048)
    assert bool(al.ok.all())
    want = ctc_segment_long(xt, il, lt, ll, path=al.path, band=64)
    for k, a, c in zip(FIELDS, out, want):
        assert torch.equal(bits(a), bits(c)), k
    lo = ctc_corridor(al.path, il, ll, 64)
    ref = LR.segment_batch_banded(x, [400, 390], labels, [100, 96], lo.cpu().numpy(), 64)
    check(to_np(out), ref, cap=0.1)
    from voice100_amd import decode as D

    def lossy(*args, **kw):                              # what ctc_align_long returns where its band loses row 1: ok 0, a path of zeros
        r = ctc_align_long(*args, **kw)
        keep = torch.tensor([1, 0], dtype=torch.int32, device=cuda)
        return r._replace(ok=r.ok * keep, path=r.path * keep[:, None])
    monkeypatch.setattr(D, "ctc_align_long", lossy)
    g = to_np(ctc_segment_long(xt, il, lt, ll, band=256))                     # (band >= n: the corridor of zeros alone would be feasible)
    assert g["ok"].tolist() == [1, 0] and g["log_prob"][1] == -np.inf and not g["start"][1].any() and not g["duration"][1].any()
    assert np.all(g["log_confidence"][1, :96] == -np.inf) and not g["log_confidence"][1, 96:].any() and g["n_words"][1] > 0
    assert np.all(g["word_log_confidence"][1, :g["n_words"][1]] == -np.inf) and not g["word_end"][1].any()
    monkeypatch.undo()
    keep = torch.tensor([1, 0], dtype=torch.int32, device=cuda)               # the same through path= with the aligner's ok beside it
    h = to_np(ctc_segment_long(xt, il, lt, ll, path=al.path * keep[:, None], path_ok=al.ok * keep, band=256))
    for k in g:
        assert np.array_equal(g[k], h[k]), k
    with pytest.raises(RuntimeError, match="path_ok"):
        ctc_segment_long(xt, il, lt, ll, path_ok=al.ok, band=256)


def test_pipeline_whole_with_confidences(cuda, monkeypatch):
    """Past 4,096 frames: the new keys equal a direct ctc_segment_long call, the old keys are what confidences=False gives"""
    from _beam_stream_cases import LONG, planted
    x = torch.from_numpy(planted(LONG["T"], LONG["V"], LONG["seed"], LONG["peak"])).to(cuda)
    assert x.shape[0] > 4096
    pipe = LongASRPipeline(None, beam_size=4, frame_seconds=0.02, seg_band=64)
    base = pipe.whole(logits=x)
    out = pipe.whole(logits=x, confidences=True)
    for k, v in base.items():
        assert (v == out[k]) if not isinstance(v, torch.Tensor) else torch.equal(bits(v), bits(out[k])), k
    n = int(out["ids_len"])
    assert n > 500 and int(out["ok"]) == 1 and int(out["seg_ok"]) == 1
    al = ctc_align_long(torch.log_softmax(x, -1)[None], out["ids"][None], None, out["ids_len"].reshape(1), band=pipe.band)
    want = ctc_segment_long(x[None], None, out["ids"][None], out["ids_len"].reshape(1), path=al.path, band=64)
    names = {"log_prob": "log_prob", "start": "soft_start", "end": "soft_end", "duration": "duration", "log_confidence": "log_confidence",
             "word_first": "word_first", "word_count": "word_count", "word_start": "word_start", "word_end": "word_end",
             "word_log_confidence": "word_log_confidence", "n_words": "n_words"}
    for k, name in names.items():
        assert torch.equal(bits(out[name]), bits(getattr(want, k)[0])), k
    assert set(out) == set(base) | set(names.values()) | {"seg_ok"}
    conf = torch.exp(out["word_log_confidence"][:int(out["n_words"])])
    assert int(out["n_words"]) > 50 and bool((conf > 0.5).all()) and bool((conf <= 1).all())      # 6 nats on the planted class
    assert bool((out["soft_start"] < out["soft_end"]).all()) and int((out["soft_start"] - out["start"]).abs().max()) <= 1
    with pytest.raises(RuntimeError, match="timed"):
        pipe.whole(logits=x, timed=False, confidences=True)
    # an aligner that loses the path: no finite confidence comes out, although seg_band >= 2 L + 1 makes the corridor of zeros feasible
    from voice100_amd import decode as D
    short, wide = x[:1500].contiguous(), LongASRPipeline(None, beam_size=4, frame_seconds=0.02, seg_band=1024)
    good = wide.whole(logits=short, confidences=True)
    assert int(good["seg_ok"]) == 1 and 2 * int(good["ids_len"]) + 1 <= 1024 and bool(torch.isfinite(good["log_prob"]))
    monkeypatch.setattr(D, "ctc_align_long", lambda *a, **kw: (lambda r: r._replace(ok=r.ok * 0, path=r.path * 0))(ctc_align_long(*a, **kw)))
    lost = wide.whole(logits=short, confidences=True)
    nw = int(lost["n_words"])
    assert int(lost["ok"]) == 0 and int(lost["seg_ok"]) == 0 and float(lost["log_prob"]) == -np.inf and nw == int(good["n_words"]) > 0
    assert not lost["soft_start"].any() and not lost["soft_end"].any() and not lost["duration"].any() and not lost["word_end"].any()
    assert bool((lost["log_confidence"] == -np.inf).all()) and bool((lost["word_log_confidence"][:nw] == -np.inf).all())


def test_transcribe_whole_with_confidences(cuda, tmp_path):
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.audio_io import load_batch, save_wav
    from voice100_amd.mel import MelSpectrogramAudioTransform
    alphabet = "_ abcdefghijklmnopqrstuvwxyz'"
    decode = lambda ids: "".join(alphabet[int(i)] for i in ids)  # noqa: E731
    torch.manual_seed(3)
    model = AudioToTextCTC(64, 32, 29, 32).to(cuda).eval()
    wave = torch.randn(round(16000 * 10.0005), generator=torch.Generator().manual_seed(9)) * 0.1
    path = str(tmp_path / "chapter.wav")
    save_wav(path, wave.clamp(-0.99, 0.99), 16000)
    pipe = LongASRPipeline(model, MelSpectrogramAudioTransform().to(cuda), beam_size=4, keep=200)
    plain, res = pipe.transcribe_whole(path, decode), pipe.transcribe_whole(path, decode, confidences=True)
    out = pipe.whole(load_batch([path], 16000, cuda)[0][0], confidences=True)
    assert res["text"] == plain["text"] and len(res["words"]) == len(plain["words"]) == int(out["n_words"]) > 0
    assert int(out["seg_ok"]) == 1
    for w, (a, c) in enumerate(zip(res["words"], plain["words"])):
        assert set(a) == {"word", "start", "end", "confidence"} and {k: a[k] for k in c} == c
        assert a["confidence"] == pytest.approx(math.exp(float(out["word_log_confidence"][w])), rel=1e-6) and 0 < a["confidence"] <= 1
