"""decode.ctc_beam_search(lm=...) (K25, the fused form of csrc/beam.hip) and ASRPipeline's LM path against the float64 oracle of
tests/_beam_lm_ref.py.

As in tests/test_gpu_beam.py the oracle forks where ranks W and W + 1 of a frame are closer than rounding can resolve, the device must
equal SOME leaf (ids rank by rank up to the leaf's first near-tie, the fused score within 1e-4 * max(1, |score|), and up to that
near-tie also ctc_scores and lm_scores), and at most 10 % of a cell's cases may be undecided (tests/test_beam_lm_cpu.py asserts that
for the oracle alone).  Every result also goes through check(): test_gpu_beam's properties on the CTC scores, falling fused scores, and
score = ctc + alpha lm + beta length."""
import ctypes
import math

import numpy as np
import pytest
import torch

import test_gpu_beam as plain
from _beam_lm_ref import (GPU_SHAPES, SETTINGS, AutomatonLM, accept, beam_search, beam_search_fork, fit_lm, random_automaton, seeded_case,
                          shape_params)
from _beam_ref import REL, TOL, ctc_loglik, log_softmax
from conftest import load_golden, sub
from voice100_amd import _native as N
from voice100_amd.asr import AudioToTextCTC
from voice100_amd.decode import ctc_beam_search
from voice100_amd.infer import ASRPipeline
from voice100_amd.lm import NGramLM

pytestmark = pytest.mark.gpu


def device_lm(dev, lm, blank=0):
    """The LM as the device takes it: an NGramLM (compiled here) or (logp, next, final, start) tables."""
    if isinstance(lm, NGramLM):
        if lm.logp is None:
            lm.compile()
        return NGramLM.from_tables(lm.logp, lm.next, lm.final, lm.start, lm.blank).to(dev)
    return NGramLM.from_tables(*lm[:3], start=lm[3] if len(lm) > 3 else 0, blank=blank).to(dev)


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def check(x, lengths, out, blank, alpha, beta):
    B, T, V = x.shape
    ids, lens, scores, ctc, lm = out
    assert all(a.dtype == np.float32 and a.shape == lens.shape for a in (scores, ctc, lm))
    nbest = ids.shape[1]
    assert ids.dtype == np.int64 and lens.dtype == np.int32 and ids.shape == (B, nbest, T)
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        lp = log_softmax(x[b, :n]) if n else np.zeros((0, V))
        seen = set()
        for r in range(nbest):
            m, s = int(lens[b, r]), float(scores[b, r])
            assert 0 <= m <= n and not np.any(ids[b, r, m:])
            if s == -math.inf:                           # "no hypothesis" only at the end: -inf, -inf, 0
                assert m == 0 and all(float(v) == -math.inf for v in scores[b, r:]) and float(ctc[b, r]) == -math.inf and lm[b, r] == 0
                continue
            hyp = tuple(int(v) for v in ids[b, r, :m])
            assert hyp not in seen and blank not in hyp and all(0 <= v < V for v in hyp)
            seen.add(hyp)
            assert r == 0 or s <= float(scores[b, r - 1])
            exact = ctc_loglik(lp, list(hyp), blank)
            assert float(ctc[b, r]) <= exact + TOL * max(1.0, abs(exact)), (b, r, float(ctc[b, r]), exact)
            whole = float(ctc[b, r]) + alpha * float(lm[b, r]) + beta * m
            assert abs(s - whole) <= 2e-6 * (abs(float(ctc[b, r])) + abs(alpha * float(lm[b, r])) + abs(beta * m) + 1.0)


def run(dev, x, W, nbest, lm, alpha, beta, blank=0, lengths=None, use_eos=True):
    """Two calls on the same input (one launch each, equal bits), the properties, and the five outputs as numpy arrays."""
    xt = torch.from_numpy(x).to(dev)
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    kw = dict(beam_size=W, nbest=nbest, blank=blank, lm=lm, lm_weight=alpha, length_bonus=beta, use_eos=use_eos)
    before = N.launch_count()
    out = ctc_beam_search(xt, lt, **kw)
    assert N.launch_count() - before == 1 and len(out) == 5
    again = ctc_beam_search(xt, lt, **kw)
    for a, c in zip(out, again):
        assert torch.equal(bits(a), bits(c))
    out = tuple(o.cpu().numpy() for o in out)
    check(x, lengths, out, blank, alpha, beta)
    return out


def row_of(out, b):
    ids, lens, scores, ctc, lm = out
    return ([tuple(int(v) for v in ids[b, r, :lens[b, r]]) for r in range(ids.shape[1])], [float(s) for s in scores[b]],
            [float(s) for s in ctc[b]], [float(s) for s in lm[b]])


def against_oracle(leaves, out, what):
    undecided, worst, cases = 0, 0.0, out[0].shape[0]
    for b in range(cases):
        if leaves[b] is None:
            undecided += 1
            continue
        ok, err = accept(leaves[b], *row_of(out, b))
        assert ok, f"{what}, row {b}: no leaf of {len(leaves[b])} matches (best difference {err:.3e}); got {row_of(out, b)}"
        worst = max(worst, err)
    assert undecided <= 0.1 * cases, f"{what}: {undecided} of {cases} cases undecided"
    print(f"{what}: score_rel_err_max {worst:.3e}, undecided {undecided}")
    assert REL >= 8 * worst, f"{what}: the fork threshold {REL} is less than 8 x the device's score error {worst:.3e}"
    return worst


@pytest.mark.parametrize("kind", ["automaton", "fit"])
@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=["a%g-b%g-S%d" % s for s in SETTINGS])
@pytest.mark.parametrize("index", range(len(GPU_SHAPES)), ids=["T%d-V%d-W%d" % s for s in GPU_SHAPES])
def test_seeded_shapes_against_forking_oracle(cuda, index, setting, kind):
    T, V, W = GPU_SHAPES[index]
    alpha, beta, _ = SETTINGS[setting]
    _, nbest, _ = shape_params(T, V, W)
    x, lm, leaves = seeded_case(index, setting, kind)
    out = run(cuda, x, W, nbest, device_lm(cuda, lm), alpha, beta)
    against_oracle(leaves, out, f"T {T} V {V} W {W} alpha {alpha} beta {beta} {kind}")


@pytest.mark.parametrize("index", [0, 1, 2, 6, 9])
def test_neutral_lm_is_the_plain_search(cuda, index):
    T, V, W = GPU_SHAPES[index]
    _, nbest, _ = shape_params(T, V, W)
    x, lm, _ = seeded_case(index, 0, "automaton")
    xt = torch.from_numpy(x).to(cuda)
    want = ctc_beam_search(xt, None, W, nbest)
    assert len(want) == 3
    for a, c in zip(want, ctc_beam_search(xt, None, W, nbest, lm=None, lm_weight=3.0, length_bonus=2.0, use_eos=True)):
        assert torch.equal(bits(a), bits(c))             # without an LM the new keywords are inert
    ids, lens, scores, ctc, lms = ctc_beam_search(xt, None, W, nbest, lm=device_lm(cuda, lm), lm_weight=0.0, length_bonus=0.0,
                                                  use_eos=False)
    assert torch.equal(ids, want[0]) and torch.equal(lens, want[1]) and torch.equal(bits(ctc), bits(want[2]))
    assert torch.equal(bits(scores), bits(ctc))          # the key is the CTC total
    look = AutomatonLM(*lm[:3])
    for b in range(x.shape[0]):                          # and lm_scores is still the LM's sum over the labels
        for r in range(nbest):
            p = tuple(int(v) for v in ids[b, r, :int(lens[b, r])])
            if float(scores[b, r]) > -math.inf:
                exact = sum(look.row(p[:i])[p[i]] for i in range(len(p)))
                assert abs(float(lms[b, r]) - exact) <= TOL * max(1.0, abs(exact))


def test_plain_call_matches_the_plain_oracle(cuda):
    """lm=None through the new signature: the parent's three outputs on a seeded shape (test_gpu_beam pins them; this pins the default)."""
    x, leaves = plain.seeded_case(1)
    T, V, W, _, nbest, _ = plain.SHAPES[1]
    ids, lens, scores = (o.cpu().numpy() for o in ctc_beam_search(torch.from_numpy(x).to(cuda), beam_size=W, nbest=nbest, lm=None))
    plain.against_oracle(x, leaves, ids, lens, scores, "lm=None")


def test_an_lm_that_forbids_a_label(cuda):
    T, V, W, nbest = 24, 8, 4, 4
    logp, nxt, fin = random_automaton(5, V, 11)
    logp[:, 3] = -1e30
    x = (np.random.default_rng(21).standard_normal((8, T, V)) * 3).astype(np.float32)
    x[:, :, 3] += 4.0                                    # the acoustic model likes label 3 best
    free = ctc_beam_search(torch.from_numpy(x).to(cuda), None, W, nbest)
    assert bool((free[0] == 3).any())
    out = run(cuda, x, W, nbest, device_lm(cuda, (logp, nxt, fin)), 1.0, 0.0)
    assert not np.any(out[0] == 3) and np.all(np.isfinite(out[2][:, 0]))
    look = AutomatonLM(logp, nxt, fin)
    against_oracle([beam_search_fork(x[b], W, look, 1.0, 0.0) for b in range(8)], out, "forbidden label")


def test_use_eos_moves_the_ranking(cuda):
    T, V, W, nbest = 12, 8, 8, 8
    logp, nxt, _ = random_automaton(6, V, 5)
    fin = np.full(6, -9.0, dtype=np.float32)
    fin[2] = -0.1                                        # ending in state 2 is strongly preferred
    x = (np.random.default_rng(22).standard_normal((8, T, V)) * 2).astype(np.float32)
    lm, look = device_lm(cuda, (logp, nxt, fin)), AutomatonLM(logp, nxt, fin)
    with_eos = run(cuda, x, W, nbest, lm, 1.0, 0.0, use_eos=True)
    without = run(cuda, x, W, nbest, lm, 1.0, 0.0, use_eos=False)
    against_oracle([beam_search_fork(x[b], W, look, 1.0, 0.0, use_eos=True) for b in range(8)], with_eos, "use_eos")
    against_oracle([beam_search_fork(x[b], W, look, 1.0, 0.0, use_eos=False) for b in range(8)], without, "no eos")
    moved = sum(row_of(with_eos, b)[0][0] != row_of(without, b)[0][0] for b in range(8))
    assert moved >= 1 and any(beam_search(x[b], W, look, 1.0, 0.0, use_eos=True)[0][0] != beam_search(x[b], W, look, 1.0, 0.0, use_eos=False)[0][0]
                              for b in range(8))
    for b in range(8):                                   # the same beam either way: only final differs
        a, c = row_of(with_eos, b), row_of(without, b)
        assert set(a[0]) == set(c[0])
        for p, s in zip(a[0], a[3]):
            assert abs(s - (c[3][c[0].index(p)] + look.final(p))) <= 1e-4


def test_ragged_batch_against_per_row_calls(cuda):
    T, V, W, nbest = 24, 29, 8, 4
    lengths = [0, 1, T, 7, 13, T, 2]
    x = (np.random.default_rng(7).standard_normal((len(lengths), T, V)) * 3).astype(np.float32)
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan                                # nothing beyond a row's length is read
    fit, look = fit_lm(V)
    lm = device_lm(cuda, fit)
    out = run(cuda, x, W, nbest, lm, 0.5, 0.3, lengths=lengths)
    eos0 = look.final(())
    assert out[1][0].tolist() == [0] * nbest and out[3][0].tolist() == [0.0] + [-math.inf] * (nbest - 1)
    assert abs(out[4][0, 0] - eos0) <= 1e-5 and abs(out[2][0, 0] - 0.5 * eos0) <= 1e-5      # no frame: the empty hypothesis and </s>
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        one = run(cuda, np.ascontiguousarray(x[b:b + 1, :n]), W, nbest, lm, 0.5, 0.3)
        assert np.array_equal(out[0][b, :, :n], one[0][0]) and not np.any(out[0][b, :, n:])
        assert all(np.array_equal(out[i][b].view(np.int32), one[i][0].view(np.int32)) for i in range(1, 5))
        leaves = beam_search_fork(x[b, :n], W, look, 0.5, 0.3)
        assert leaves is not None and accept(leaves, *row_of(out, b))[0]
    clamped = run(cuda, np.nan_to_num(x), W, nbest, lm, 0.5, 0.3, lengths=[T + 5] * len(lengths))     # lengths clamp to [0, T]
    full = run(cuda, np.nan_to_num(x), W, nbest, lm, 0.5, 0.3)
    assert all(np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a, c.view(np.int32) if c.dtype == np.float32 else c)
               for a, c in zip(clamped, full))
    assert run(cuda, x, W, nbest, lm, 0.5, 0.3, lengths=[-3] * len(lengths))[1].tolist() == [[0] * nbest] * len(lengths)


@pytest.mark.parametrize("nbest", [1, 2, 5, 8])
def test_nbest_from_one_to_the_beam(cuda, nbest):
    T, V, W = 33, 29, 8
    x, lm, leaves = seeded_case(1, 2, "fit")
    alpha, beta, _ = SETTINGS[2]
    out = run(cuda, x, W, nbest, device_lm(cuda, lm), alpha, beta)
    whole = run(cuda, x, W, W, device_lm(cuda, lm), alpha, beta)
    for i in range(5):                                   # the first nbest of the whole beam
        assert np.array_equal(out[i], whole[i][:, :nbest])
    against_oracle(leaves, out, f"nbest {nbest}")


@pytest.mark.parametrize("blank", [28, 14])
def test_blank_elsewhere(cuda, blank):
    T, V, W, nbest, cases = 33, 29, 8, 4, 6
    x = (np.random.default_rng(90 + blank).standard_normal((cases, T, V)) * 3).astype(np.float32)
    fit, look = fit_lm(V, 3, blank)
    out = run(cuda, x, W, nbest, device_lm(cuda, fit), 1.0, 0.5, blank=blank)
    against_oracle([beam_search_fork(x[i], W, look, 1.0, 0.5, blank) for i in range(cases)], out, f"blank {blank} fit")
    tables = random_automaton(9, V, blank, blank)
    out = run(cuda, x, W, nbest, device_lm(cuda, tables, blank), 2.0, -0.5, blank=blank)
    against_oracle([beam_search_fork(x[i], W, AutomatonLM(*tables), 2.0, -0.5, blank) for i in range(cases)], out, f"blank {blank} automaton")


def test_a_row_of_nans_ends_and_leaves_its_neighbours_alone(cuda):
    T, V, W, nbest = 20, 29, 8, 4
    x = (np.random.default_rng(8).standard_normal((3, T, V)) * 3).astype(np.float32)
    lm = device_lm(cuda, fit_lm(V)[0])
    good = ctc_beam_search(torch.from_numpy(x).to(cuda), None, W, nbest, lm=lm)
    x[1] = np.nan
    out = ctc_beam_search(torch.from_numpy(x).to(cuda), None, W, nbest, lm=lm)
    torch.cuda.synchronize()
    for b in (0, 2):
        assert all(torch.equal(bits(o[b]), bits(g[b])) for o, g in zip(out, good))
    ids, lens = out[:2]
    assert int(lens[1].min()) >= 0 and int(lens[1].max()) <= T and int(ids[1].min()) >= 0 and int(ids[1].max()) < V


def test_a_corrupt_next_table_stays_in_bounds(cuda):
    T, V, W, nbest = 16, 8, 4, 4
    logp, nxt, fin = random_automaton(4, V, 2)
    bad = nxt.copy()
    bad[:, 1::2] = np.array([-7, 2 ** 31 - 1, 4, 10 ** 6], dtype=np.int32)[:, None]
    x = (np.random.default_rng(9).standard_normal((4, T, V)) * 3).astype(np.float32)
    out = run(cuda, x, W, nbest, device_lm(cuda, (logp, bad, fin)), 1.0, 0.0)
    clamped = np.clip(bad, 0, 3).astype(np.int32)        # the device clamps a successor to [0, S)
    want = run(cuda, x, W, nbest, device_lm(cuda, (logp, clamped, fin)), 1.0, 0.0)
    assert all(np.array_equal(a, c) for a, c in zip(out, want))


def test_refusals_raise_without_a_launch(cuda):
    x = torch.zeros((2, 8, 29), device=cuda)
    lm = device_lm(cuda, random_automaton(3, 29, 0))
    before = N.launch_count()
    cpu_lm = NGramLM.from_tables(*random_automaton(3, 29, 0))
    uncompiled = NGramLM.fit([[1, 2, 3]], 29, 2)
    empty = NGramLM.from_tables(*random_automaton(3, 29, 0))
    empty.logp, empty.next, empty.final = (t[:0].to(cuda) for t in (empty.logp, empty.next, empty.final))
    other_blank = device_lm(cuda, random_automaton(3, 29, 0, 5), 5)
    for bad in (device_lm(cuda, random_automaton(3, 30, 0)), cpu_lm, uncompiled, empty, other_blank):
        with pytest.raises(RuntimeError, match="language model"):
            ctc_beam_search(x, lm=bad)
    for kw in ({"beam_size": 65}, {"beam_size": 0}, {"beam_size": 4, "nbest": 5}, {"nbest": 0}, {"blank": 29}, {"lm_weight": math.inf},
               {"length_bonus": math.nan}):
        with pytest.raises(RuntimeError):
            ctc_beam_search(x, lm=lm, **kw)
    for shape in ((2, 8, 129), (2, 4097, 29)):
        with pytest.raises(RuntimeError):
            ctc_beam_search(torch.zeros(shape, device=cuda), lm=lm)
    with pytest.raises(RuntimeError):
        ctc_beam_search(x.cpu(), lm=lm)
    assert N.launch_count() == before
    out = ctc_beam_search(x, beam_size=64, nbest=64, lm=lm)                   # the limits themselves are inside
    assert out[0].shape == (2, 64, 8) and bool(torch.isfinite(out[2][:, 0]).all())


def test_c_level_null_pointers(cuda):
    lib = N.load()
    x = torch.zeros((1, 4, 8), device=cuda)
    lm = device_lm(cuda, random_automaton(2, 8, 0))
    ws = torch.empty((N.helper("v100_ctc_beam_workspace_bytes", 1, 4, 8, 2),), dtype=torch.uint8, device=cuda)
    ids, lens = torch.empty((1, 1, 4), dtype=torch.int64, device=cuda), torch.empty((1, 1), dtype=torch.int32, device=cuda)
    sc, ctc, lms = (torch.empty((1, 1), device=cuda) for _ in range(3))
    ptrs = [t.data_ptr() for t in (x, lens, ws, ids, lens, sc, lm.logp, lm.next, lm.final)]
    tail = [ctc.data_ptr(), lms.data_ptr(), 1, 4, 8, 2, 1, 0, None]
    before = N.launch_count()
    for k in (0, 2, 3, 4, 5, 6, 7, 8):
        args = list(ptrs)
        args[k] = None
        assert lib.v100_ctc_beam_search_lm(*args, 2, 0, 0.5, 0.0, 1, *tail) == 3
    for k in (0, 1):
        t = list(tail)
        t[k] = None
        assert lib.v100_ctc_beam_search_lm(*ptrs, 2, 0, 0.5, 0.0, 1, *t) == 3
    assert lib.v100_ctc_beam_search_lm(*ptrs, 2, 2, 0.5, 0.0, 1, *tail) == 1        # the start state is outside [0, S)
    assert N.launch_count() == before


def test_pipeline_with_an_lm(cuda):
    model = AudioToTextCTC(64, 32, 29, 32)
    model.load_state_dict(sub(load_golden("asr_tiny.npz"), "state/"), strict=True)
    model = model.to(cuda).eval()
    lm = device_lm(cuda, fit_lm(29)[0])
    beam, fused = ASRPipeline(model, beam_size=8, nbest=3), ASRPipeline(model, beam_size=8, nbest=3, lm=lm, lm_weight=0.8, length_bonus=0.4)
    gen = torch.Generator().manual_seed(12)
    frames = (96, 61, 80, 33)
    feats = torch.randn(4, max(frames), 64, generator=gen).to(cuda)
    lengths = torch.tensor(frames, dtype=torch.int32, device=cuda)
    text = torch.randint(1, 29, (4, 9), generator=gen).to(cuda)
    text_len = torch.tensor([9, 4, 7, 1], dtype=torch.int32, device=cuda)
    with torch.no_grad():
        logits, out_len = model(feats), model.output_length(lengths)
    for args, lens in (((feats,), None), ((feats, lengths), out_len)):
        want = ctc_beam_search(logits, lens, 8, 3, lm=lm, lm_weight=0.8, length_bonus=0.4)
        got = fused.nbest(*args)
        assert len(got) == 5 and all(torch.equal(bits(a), bits(c)) for a, c in zip(got, want))
        ids, n = fused(*args)
        assert torch.equal(ids, want[0][:, 0]) and torch.equal(n, want[1][:, 0])
        plain_want = ctc_beam_search(logits, lens, 8, 3)                     # without an LM the pipeline is unchanged
        plain_got = beam.nbest(*args)
        assert len(plain_got) == 3 and all(torch.equal(bits(a), bits(c)) for a, c in zip(plain_got, plain_want))
        assert torch.equal(beam(*args)[0], plain_want[0][:, 0])
    s = fused.score(feats, lengths, text, text_len)
    assert torch.equal(s["ids"], fused(feats, lengths)[0]) and torch.equal(s["chars"], text_len)
    e = fused.evaluate([(feats, lengths, text, text_len)])
    assert e["chars"] == int(text_len.sum()) and e["utterances"] == 4 and e["char_errors"] == int(s["char_errors"].sum())
