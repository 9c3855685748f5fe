"""CPU-side checks of long-form transcription (K31): the numpy mirror of the pause cutter against the independent brute-force checker on
seeded random rows, the C entry points' status codes and the workspace helper, the wrapper's refusals, the batching plan, the
separator rule of the joined text and the record lines."""
import numpy as np
import pytest
import torch

import _cut_points_ref as R


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    return N.load()


def random_row(seed):
    """A row of random short runs and arguments drawn around the rule's edges."""
    rng = np.random.default_rng(seed)
    T = int(rng.integers(1, 400))
    V = int(rng.choice([2, 5, 29]))
    blank = int(rng.choice([0, V - 1]))
    pad = int(rng.integers(0, 4))
    min_frames = int(rng.integers(1, 6))
    max_frames = 2 * pad + 2 * min_frames + int(rng.integers(0, 12))
    min_gap = [None, 1, 2, 5, 9][int(rng.integers(5))]
    p, hold = float(rng.uniform(0.05, 0.7)), int(rng.integers(1, 8))
    spec, t = [], 0
    while t < T:
        k = min(int(rng.integers(1, hold + 1)), T - t)
        spec.append(("s" if rng.random() < p else "n", k))
        t += k
    x = R.pattern(spec, V, blank, seed, noise=float(rng.choice([0.0, 1.0, 6.0])))
    n = T if rng.random() < 0.5 else int(rng.integers(0, T + 1))
    return x, n, dict(blank=blank, max_frames=max_frames, min_gap=min_gap, margin=float(rng.choice([0.0, 0.0, 2.5, -1.0])), pad=pad,
                      min_frames=min_frames)


def test_mirror_keeps_its_promises_on_random_rows():
    forced = plain = 0
    for seed in range(300):
        x, n, kw = random_row(seed)
        s, e, f, cnt = R.mirror(x[None], [n], **kw)
        k = int(cnt[0])
        assert s.shape == (1, k)
        R.check(x, n, s[0], e[0], f[0], **kw)
        forced += bool(f.any())
        plain += k > 0 and not f.any()
    assert forced >= 60 and plain >= 60


def test_mirror_on_the_case_list_and_hand_made_rows():
    cases = R.case_list()
    assert len(cases) == 57
    for name, x, lengths, kw in cases:
        if x.shape[1] > 1000:
            continue                                              # (the long rows are checked in the GPU suite, once)
        s, e, f, cnt = R.mirror(x, lengths, **kw)
        for b in range(x.shape[0]):
            n = x.shape[1] if lengths is None else int(min(max(lengths[b], 0), x.shape[1]))
            k = int(cnt[b])
            R.check(x[b], n, s[b, :k], e[b, :k], f[b, :k], **kw)
    # by hand: s7 n6 s4 n5 s3 n6 s9 with min_gap 4, pad 2: the run of 4 is a cut, the run of 3 is not
    x = R.pattern([("s", 7), ("n", 6), ("s", 4), ("n", 5), ("s", 3), ("n", 6), ("s", 9)])
    s, e, f, cnt = R.mirror(x[None], None, max_frames=40, min_gap=4, pad=2, min_frames=4)
    assert cnt.tolist() == [2] and s.tolist() == [[5, 15]] and e.tolist() == [[15, 33]] and not f.any()
    # the core of 14 frames does not fit C = 12: its only run leaves 5 and 6 frames, the cut goes there
    s, e, f, cnt = R.mirror(x[None], None, max_frames=16, min_gap=4, pad=2, min_frames=4)
    assert s.tolist() == [[5, 15, 24]] and e.tolist() == [[15, 23, 33]] and not f.any()
    # ... and with min_frames 6 the run no longer qualifies (5 < 6 on its left): a forced cut at the first largest margin of [23, 25]
    s, e, f, cnt = R.mirror(x[None], None, max_frames=16, min_gap=4, pad=2, min_frames=6)
    assert cnt.tolist() == [3] and f.tolist() == [[0, 0, 1]] and 23 <= s[0, 2] == e[0, 1] <= 25
    # equal runs at 5, 10 and 15 (the one at 23 lies beyond C = 16): the latest wins, and its two frames are shared one each
    x = R.pattern([("n", 5), ("s", 2), ("n", 3), ("s", 2), ("n", 3), ("s", 2), ("n", 6), ("s", 1), ("n", 5)])
    s, e, f, cnt = R.mirror(x[None], None, max_frames=20, min_gap=5, pad=2, min_frames=4)
    assert s.tolist() == [[0, 16]] and e.tolist() == [[16, 29]] and not f.any()


def test_status_codes_and_workspace(lib):
    ws = lib.v100_ctc_cut_points_workspace_bytes
    assert lib.v100_ctc_cut_points_span() == 64 and lib.v100_ctc_cut_points_pass() == 64 * 512
    al = lambda v: (v + 15) // 16 * 16                            # noqa: E731
    row = lambda T: 16 + 3 * al(4 * T) + al(8 * ((T + 63) // 64)) + 3 * al(4 * (T // 2 + 2))    # noqa: E731
    assert ws(1, 1) == row(1) and ws(3, 65) == 3 * row(65) and ws(4, 90000) == 4 * row(90000)
    assert ws(2, 1 << 20) == 2 * row(1 << 20)
    for bad in ((0, 10), (1, 0), (1, (1 << 20) + 1), (-1, 10)):
        assert ws(*bad) == 0, bad
    one = 16
    cut = lib.v100_ctc_cut_points
    good = dict(B=1, T=10, V=29, blank=0, max_frames=3000, min_gap=25, margin=0.0, pad=5, min_frames=50)
    call = lambda logits=one, ws_=one, n_seg=one, **kw: cut(logits, None, ws_, n_seg, *({**good, **kw}).values(), None)    # noqa: E731
    assert call(logits=None) == 3 and call(ws_=None) == 3 and call(n_seg=None) == 3
    for kw in (dict(B=0), dict(T=0), dict(T=(1 << 20) + 1), dict(V=1), dict(V=129), dict(blank=-1), dict(blank=29), dict(max_frames=1),
               dict(max_frames=4097), dict(pad=-1), dict(min_frames=0), dict(min_gap=-1), dict(max_frames=109), dict(pad=1450, min_frames=51),
               dict(margin=float("nan"))):
        assert call(**kw) == 1, kw
    table = lib.v100_ctc_cut_points_table
    assert table(None, one, one, one, 1, 10, 3, 5, None) == 3 and table(one, one, None, one, 1, 10, 3, 5, None) == 3
    for B, T, S, pad in ((0, 10, 3, 5), (1, 0, 3, 5), (1, 10, 0, 5), (1, 10, 11, 5), (1, 10, 3, -1)):
        assert table(one, one, one, one, B, T, S, pad, None) == 1, (B, T, S, pad)


def test_wrapper_refusals():
    from voice100_amd.decode import ctc_cut_points
    from voice100_amd.infer import LongASRPipeline
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ctc_cut_points(torch.zeros(1, 8, 29))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        LongASRPipeline(None).segments(logits=torch.zeros(8, 29))
    with pytest.raises(RuntimeError, match="no mel"):
        LongASRPipeline(None).transcribe("a.wav", lambda ids: "")
    with pytest.raises(RuntimeError, match="blank"):
        LongASRPipeline(None, blank=3)
    with pytest.raises(RuntimeError, match="max_batch"):
        LongASRPipeline(None, max_batch=0)
    with pytest.raises(RuntimeError, match="language model needs a beam_size"):
        LongASRPipeline(None, lm=object())


def test_wrapper_names_the_limits():
    """The limits need no device, so they are refused first: a CPU tensor inside them gets "GPU tensors only" (above)."""
    from voice100_amd.decode import ctc_cut_points
    x = torch.zeros(1, 8, 29)
    for kw in (dict(blank=29), dict(blank=-1), dict(max_frames=4097), dict(max_frames=1), dict(pad=-1), dict(min_frames=0), dict(min_gap=0),
               dict(max_frames=100, pad=5, min_frames=46), dict(margin=float("nan"))):
        with pytest.raises(RuntimeError, match="are the limits"):
            ctc_cut_points(x, **kw)
    for shape in ((1, 8, 1), (1, 8, 129), (1, 0, 29), (0, 8, 29)):
        with pytest.raises(RuntimeError, match="are the limits"):
            ctc_cut_points(torch.zeros(shape))
    with pytest.raises(RuntimeError, match=r"\[B, T, V\]"):
        ctc_cut_points(torch.zeros(8, 29))
    with pytest.raises(RuntimeError, match="lengths must have"):
        ctc_cut_points(x, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ctc_cut_points(x, min_gap=None, max_frames=4096, pad=0, min_frames=2048)


def test_batch_plan():
    from voice100_amd.infer import batch_plan
    assert batch_plan(0, 4) == []
    assert batch_plan(1, 4) == [(0, 1)] and batch_plan(4, 4) == [(0, 4)] and batch_plan(5, 4) == [(0, 4), (4, 5)]
    assert batch_plan(7, 1) == [(i, i + 1) for i in range(7)]
    for n, m in ((33, 32), (64, 32), (100, 7)):
        plan = batch_plan(n, m)
        assert [i for lo, hi in plan for i in range(lo, hi)] == list(range(n)) and all(0 < hi - lo <= m for lo, hi in plan)
        assert [lo for lo, _ in plan] == list(range(0, n, m))     # the rows whose lengths pad each call
    for bad in ((-1, 4), (3, 0)):
        with pytest.raises(ValueError):
            batch_plan(*bad)


def test_join_ids_separator_rule():
    from voice100_amd.infer import join_ids
    assert join_ids([[3, 4], [5]], 1) == [3, 4, 1, 5]
    assert join_ids([[3, 1], [5]], 1) == [3, 1, 5] and join_ids([[3], [1, 5]], 1) == [3, 1, 5]
    assert join_ids([[3, 1], [1, 5]], 1) == [3, 1, 1, 5]          # both supply one: nothing is added, nothing removed
    assert join_ids([[], [3], [], [4], []], 1) == [3, 1, 4] and join_ids([], 1) == [] and join_ids([[], []], 1) == []
    assert join_ids([[3, 4], [5]], None) == [3, 4, 5]
    assert join_ids([torch.tensor([7, 8]), torch.tensor([9])], 2) == [7, 8, 2, 9]


def test_long_transcript_records_lines():
    from voice100_amd.infer import long_transcript_records
    res = {"utterances": [{"start_s": 0.04, "end_s": 1.5, "score": -0.25, "text": "ab c"}, {"start_s": 1.5, "end_s": 2.0, "score": -3.0, "text": ""}]}
    assert long_transcript_records(res) == ["0.040|1.500|-0.2500|ab c", "1.500|2.000|-3.0000|"]
    assert long_transcript_records({"utterances": []}) == []
