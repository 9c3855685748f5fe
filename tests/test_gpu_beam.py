"""decode.ctc_beam_search (K24, csrc/beam.hip) and ASRPipeline's beam path against the float64 oracle of tests/_beam_ref.py.

The oracle forks where ranks W and W + 1 of a frame are closer than rounding can resolve; the device must equal SOME leaf (ids rank by
rank up to the leaf's first near-tie of final scores, scores within 1e-4 * max(1, |score|)).  A case with more than 64 leaves is
undecided and not compared; at most 10 % of a test's cases may be (tests/test_beam_cpu.py asserts that for the oracle alone).  Every
result of every test also goes through check(): distinct hypotheses, falling scores, zero padding, no blank among the ids, score <=
the exact CTC log-likelihood of the labels, and equal bits from a second call."""
import math

import numpy as np
import pytest
import torch

from _beam_ref import REL, SHAPES, TOL, accept, beam_search_fork, brute_force, ctc_loglik, log_softmax, seeded_case
from conftest import load_golden, sub
from voice100_amd import _native as N
from voice100_amd.asr import AudioToTextCTC
from voice100_amd.decode import ctc_beam_search, ctc_greedy_decode
from voice100_amd.infer import ASRPipeline

pytestmark = pytest.mark.gpu


def check(x, lengths, ids, lens, scores, blank):
    """The properties that hold for every result (x [B, T, V]; lengths None or [B]; the three outputs as numpy arrays)."""
    B, T, V = x.shape
    assert ids.dtype == np.int64 and lens.dtype == np.int32 and scores.dtype == np.float32
    nbest = ids.shape[1]
    assert ids.shape == (B, nbest, T) and lens.shape == (B, nbest) and scores.shape == (B, nbest)
    for b in range(B):
        n = T if lengths is None else min(max(int(lengths[b]), 0), T)
        lp = log_softmax(x[b, :n]) if n else np.zeros((0, V))
        seen = set()
        for r in range(nbest):
            m, s = int(lens[b, r]), float(scores[b, r])
            assert 0 <= m <= n and not np.any(ids[b, r, m:])
            if s == -math.inf:
                assert m == 0 and all(float(v) == -math.inf for v in scores[b, r:])       # "no hypothesis" only at the end
                continue
            hyp = tuple(int(v) for v in ids[b, r, :m])
            assert hyp not in seen and blank not in hyp and all(0 <= v < V for v in hyp)
            seen.add(hyp)
            assert r == 0 or s <= float(scores[b, r - 1])
            exact = ctc_loglik(lp, list(hyp), blank)
            assert s <= exact + TOL * max(1.0, abs(exact)), (b, r, s, exact)


def run(dev, x, W, nbest, blank=0, lengths=None):
    """Two calls on the same input (equal bits), the properties, and the outputs as numpy arrays."""
    xt = torch.from_numpy(x).to(dev)
    lt = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    before = N.launch_count()
    out = ctc_beam_search(xt, lt, beam_size=W, nbest=nbest, blank=blank)
    assert N.launch_count() - before == 1                # one launch
    again = ctc_beam_search(xt, lt, beam_size=W, nbest=nbest, blank=blank)
    for a, c in zip(out, again):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, c.view(torch.int32) if c.dtype == torch.float32 else c)
    ids, lens, scores = (o.cpu().numpy() for o in out)
    check(x, lengths, ids, lens, scores, blank)
    return ids, lens, scores


def hyps_of(ids, lens, scores, b):
    return ([tuple(int(v) for v in ids[b, r, :lens[b, r]]) for r in range(ids.shape[1])], [float(s) for s in scores[b]])


def against_oracle(x, leaves, ids, lens, scores, what):
    """Every decided row must equal some leaf; returns the worst relative score difference.  At most 10 % undecided."""
    undecided, worst = 0, 0.0
    for b in range(x.shape[0]):
        if leaves[b] is None:
            undecided += 1
            continue
        ok, err = accept(leaves[b], *hyps_of(ids, lens, scores, b))
        assert ok, f"{what}, row {b}: no leaf of {len(leaves[b])} matches (best score difference {err:.3e}); got {hyps_of(ids, lens, scores, b)}"
        worst = max(worst, err)
    assert undecided <= 0.1 * x.shape[0], f"{what}: {undecided} of {x.shape[0]} cases undecided"
    print(f"{what}: score_rel_err_max {worst:.3e}, undecided {undecided}")
    assert REL >= 8 * worst, f"{what}: the fork threshold {REL} is less than 8 x the device's score error {worst:.3e}"
    return worst


@pytest.mark.parametrize("index", range(len(SHAPES)), ids=["T%d-V%d-W%d" % s[:3] for s in SHAPES])
def test_seeded_shapes_against_forking_oracle(cuda, index):
    T, V, W, scale, nbest, cases = SHAPES[index]
    x, leaves = seeded_case(index)
    ids, lens, scores = run(cuda, x, W, nbest)
    against_oracle(x, leaves, ids, lens, scores, f"T {T} V {V} W {W}")


@pytest.mark.parametrize("T,V,reachable", [(5, 3, 25), (6, 2, 4), (4, 4, 61)])
def test_exhaustive_search_is_the_brute_force_sum(cuda, T, V, reachable):
    rng = np.random.default_rng(100 * T + V)
    x = (rng.standard_normal((3, T, V)) * 2).astype(np.float32)
    ids, lens, scores = run(cuda, x, 64, 64)
    for b in range(3):
        exact = brute_force(log_softmax(x[b]))
        assert len(exact) == reachable
        hyps, sc = hyps_of(ids, lens, scores, b)
        assert all(s == -math.inf for s in sc[reachable:]) and all(s > -math.inf for s in sc[:reachable])    # nothing pruned, nothing impossible
        assert set(hyps[:reachable]) == set(exact)
        for h, s in zip(hyps[:reachable], sc):
            assert abs(s - exact[h]) <= TOL * max(1.0, abs(exact[h])), (h, s, exact[h])
        order = sorted(exact.items(), key=lambda e: -e[1])
        if order[0][1] - order[1][1] > REL * max(1.0, abs(order[0][1])):
            assert hyps[0] == order[0][0]


def test_ragged_batch_reads_nothing_beyond_the_lengths(cuda):
    T, V, W, nbest = 24, 29, 8, 4
    lengths = [0, 1, T, 7, 13, T, 2]
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((len(lengths), T, V)) * 3).astype(np.float32)
    for b, n in enumerate(lengths):
        x[b, n:] = np.nan
    ids, lens, scores = run(cuda, x, W, nbest, lengths=lengths)
    assert lens[0].tolist() == [0] * nbest and scores[0].tolist() == [0.0] + [-math.inf] * (nbest - 1)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        i1, l1, s1 = run(cuda, np.ascontiguousarray(x[b:b + 1, :n]), W, nbest)
        assert np.array_equal(ids[b, :, :n], i1[0]) and not np.any(ids[b, :, n:])
        assert np.array_equal(lens[b], l1[0]) and np.array_equal(scores[b].view(np.int32), s1[0].view(np.int32))
        leaves = beam_search_fork(x[b, :n], W)
        assert leaves is not None and accept(leaves, *hyps_of(ids, lens, scores, b))[0]
    clamped = run(cuda, np.nan_to_num(x), W, nbest, lengths=[T + 5] * len(lengths))       # lengths clamp to [0, T]
    full = run(cuda, np.nan_to_num(x), W, nbest)
    assert all(np.array_equal(a, c) for a, c in zip(clamped[:2], full[:2]))
    assert run(cuda, x, W, nbest, lengths=[-3] * len(lengths))[1].tolist() == [[0] * nbest] * len(lengths)


def test_a_row_of_nans_ends_and_leaves_its_neighbours_alone(cuda):
    T, V, W, nbest = 20, 29, 8, 4
    rng = np.random.default_rng(8)
    x = (rng.standard_normal((3, T, V)) * 3).astype(np.float32)
    good = ctc_beam_search(torch.from_numpy(x).to(cuda), None, W, nbest)
    x[1] = np.nan
    ids, lens, scores = ctc_beam_search(torch.from_numpy(x).to(cuda), None, W, nbest)
    torch.cuda.synchronize()
    for b in (0, 2):
        assert torch.equal(ids[b], good[0][b]) and torch.equal(lens[b], good[1][b]) and torch.equal(scores[b], good[2][b])
    assert int(lens[1].min()) >= 0 and int(lens[1].max()) <= T and int(ids[1].min()) >= 0 and int(ids[1].max()) < V


@pytest.mark.parametrize("blank", [28, 14])
def test_blank_elsewhere(cuda, blank):
    T, V, W, nbest, cases = 33, 29, 8, 4, 6
    x = (np.random.default_rng(90 + blank).standard_normal((cases, T, V)) * 3).astype(np.float32)
    ids, lens, scores = run(cuda, x, W, nbest, blank=blank)
    against_oracle(x, [beam_search_fork(x[i], W, blank) for i in range(cases)], ids, lens, scores, f"blank {blank}")


@pytest.mark.parametrize("W", [1, 16])
def test_peaked_logits_give_the_greedy_transcript(cuda, W):
    B, T, V = 4, 50, 29
    rng = np.random.default_rng(3)
    x = rng.random((B, T, V)).astype(np.float32)
    peak = rng.integers(0, V, (B, T))
    peak[:, 1::3] = peak[:, 0::3][:, :peak[:, 1::3].shape[1]]                # repeats, to be collapsed
    np.put_along_axis(x, peak[..., None], 21.0, axis=2)                      # one class ahead by 20 nats in every frame
    ids, lens, scores = run(cuda, x, W, 1)
    gid, glen = ctc_greedy_decode(torch.from_numpy(x).to(cuda))
    assert np.array_equal(lens[:, 0], glen.cpu().numpy()) and np.array_equal(ids[:, 0], gid.cpu().numpy())


def test_pipeline_beam_path(cuda):
    model = AudioToTextCTC(64, 32, 29, 32)
    model.load_state_dict(sub(load_golden("asr_tiny.npz"), "state/"), strict=True)
    model = model.to(cuda).eval()
    greedy, default, beam = ASRPipeline(model), ASRPipeline(model, beam_size=None), ASRPipeline(model, beam_size=8, nbest=3)
    gen = torch.Generator().manual_seed(12)
    frames = (96, 61, 80, 33)
    feats = torch.randn(4, max(frames), 64, generator=gen).to(cuda)
    lengths = torch.tensor(frames, dtype=torch.int32, device=cuda)
    text = torch.randint(1, 29, (4, 9), generator=gen).to(cuda)
    text_len = torch.tensor([9, 4, 7, 1], dtype=torch.int32, device=cuda)
    with torch.no_grad():
        logits, out_len = model(feats), model.output_length(lengths)
    for args in ((feats,), (feats, lengths)):
        want = ctc_greedy_decode(logits, *((out_len,) if len(args) == 2 else ()))
        for pipe in (greedy, default):                   # beam_size=None is the existing call, bit for bit
            got = pipe(*args)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        ids, n = beam(*args)
        nb_ids, nb_len, nb_sc = beam.nbest(*args)
        Tout = logits.shape[1]
        assert nb_ids.shape == (4, 3, Tout) and nb_len.shape == (4, 3) and nb_sc.shape == (4, 3)
        assert nb_ids.dtype == torch.int64 and nb_len.dtype == torch.int32 and nb_sc.dtype == torch.float32
        assert ids.shape == (4, Tout) and n.shape == (4,)
        assert torch.equal(ids, nb_ids[:, 0, :]) and torch.equal(n, nb_len[:, 0])
        xs = logits.cpu().numpy()
        check(xs, None if len(args) == 1 else out_len.cpu().numpy(), nb_ids.cpu().numpy(), nb_len.cpu().numpy(), nb_sc.cpu().numpy(), 0)
    s_greedy, s_beam = greedy.score(feats, lengths, text, text_len), beam.score(feats, lengths, text, text_len)
    assert set(s_greedy) == set(s_beam)
    assert torch.equal(s_beam["ids"], beam(feats, lengths)[0]) and torch.equal(s_beam["chars"], text_len)
    e_greedy, e_beam = greedy.evaluate([(feats, lengths, text, text_len)]), beam.evaluate([(feats, lengths, text, text_len)])
    assert set(e_greedy) == set(e_beam) and e_beam["chars"] == int(text_len.sum()) and e_beam["utterances"] == 4
    with pytest.raises(RuntimeError):
        greedy.nbest(feats, lengths)


def test_limits(cuda):
    x = torch.zeros((2, 8, 29), device=cuda)
    for kw in ({"beam_size": 65}, {"beam_size": 0}, {"beam_size": 4, "nbest": 5}, {"nbest": 0}, {"blank": 29}, {"blank": -1}):
        with pytest.raises(RuntimeError):
            ctc_beam_search(x, **kw)
    for shape in ((2, 8, 129), (2, 8, 1), (2, 4097, 4)):
        with pytest.raises(RuntimeError):
            ctc_beam_search(torch.zeros(shape, device=cuda))
    with pytest.raises(RuntimeError):
        ctc_beam_search(x.cpu())
    with pytest.raises(RuntimeError):
        ctc_beam_search(x, torch.tensor([8, 8], dtype=torch.int32))
    ids, lens, scores = ctc_beam_search(x, beam_size=64, nbest=64)            # the limits themselves are inside
    assert ids.shape == (2, 64, 8) and bool(torch.isfinite(scores[:, 0]).all())
