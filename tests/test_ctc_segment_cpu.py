"""K26 without a GPU: the float64 oracle of decode.ctc_segment (tests/_ctc_segment_ref.py) is tested, not trusted -- against an
enumeration of all alignments, against torch's ctc_loss, on planted alignments and on the edge rules -- and the library's host
side (workspace helper, argument and pointer checks, all of which return before a device call) and the Python wrapper's refusal
of CPU tensors."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import _ctc_segment_ref as R


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


def collapse(path, blank):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return out


def enumerate_alignments(logits, labels, blank):
    """p, and per label the onset / last-frame distributions, gamma and sum gamma lp, by brute force over all V^T frame sequences."""
    lp = R.log_softmax(logits)
    T, V = lp.shape
    L = len(labels)
    p = 0.0
    onset, last, gamma = np.zeros((T, L)), np.zeros((T, L)), np.zeros((T, L))
    for path in itertools.product(range(V), repeat=T):
        if collapse(path, blank) != list(labels):
            continue
        w = float(np.exp(sum(lp[t, c] for t, c in enumerate(path))))
        p += w
        i, prev = -1, None                               # which label each frame is spent in
        owner = []
        for c in path:
            if c != blank and c != prev:
                i += 1
            owner.append(i if c != blank else -1)
            prev = c
        for i in range(L):
            frames = [t for t in range(T) if owner[t] == i]
            onset[frames[0], i] += w
            last[frames[-1], i] += w
            for t in frames:
                gamma[t, i] += w
    return p, onset / p, last / p, gamma / p, lp


ENUM_CASES = [(1, 2, [1], 0), (3, 2, [1], 0), (4, 3, [1, 2], 0), (5, 3, [1, 1], 0), (6, 4, [1, 2, 3], 0), (6, 4, [2, 2, 1], 0),
              (6, 3, [1, 2, 1], 0), (6, 4, [3, 3, 3], 0), (5, 4, [0, 2], 1), (6, 3, [0, 0, 2], 1), (6, 4, [1], 0), (5, 4, [3, 1, 3], 2)]


@pytest.mark.parametrize("T,V,labels,blank", ENUM_CASES)
@pytest.mark.parametrize("scale", [0.5, 3.0])
def test_oracle_against_enumeration(T, V, labels, blank, scale):
    rng = np.random.default_rng(1000 * T + 10 * V + len(labels) + int(10 * scale))
    x = rng.standard_normal((T, V)) * scale
    p, onset, last, gamma, lp = enumerate_alignments(x, labels, blank)
    r = R.segment_one(x, labels, blank, sep=None)
    if p == 0.0:
        assert not r["feasible"] and r["log_prob"] == -np.inf
        return
    assert abs(r["log_prob"] - np.log(p)) < 1e-12 * max(1.0, abs(np.log(p)))
    np.testing.assert_allclose(r["onset_cdf"], np.cumsum(onset, 0), atol=1e-12)
    np.testing.assert_allclose(r["last_cdf"], np.cumsum(last, 0), atol=1e-12)
    np.testing.assert_allclose(r["duration"], gamma.sum(0), atol=1e-12)
    lc = np.array([(gamma[:, i] * lp[:, c]).sum() / gamma[:, i].sum() for i, c in enumerate(labels)])
    np.testing.assert_allclose(r["log_confidence"], lc, atol=1e-12)
    for i in range(len(labels)):                         # the medians, from the enumerated distributions
        assert r["start"][i] == int(np.nonzero(np.cumsum(onset[:, i]) >= 0.5 - 1e-13)[0][0]) or r["start_margin"][i] < 1e-12
        assert r["end"][i] == 1 + int(np.nonzero(np.cumsum(last[:, i]) >= 0.5 - 1e-13)[0][0]) or r["end_margin"][i] < 1e-12


def test_oracle_log_prob_is_torch_ctc_loss():
    rng = np.random.default_rng(7)
    for T, V, L, blank in ((17, 5, 4, 0), (40, 29, 12, 0), (64, 29, 20, 3), (9, 3, 9, 0), (33, 128, 10, 0)):
        x = rng.standard_normal((T, V)) * 3
        labels = [int(c) for c in rng.choice([c for c in range(V) if c != blank], L)]
        if L == T:                                       # as many labels as frames: no repeats, one alignment
            labels = [1 + (i % 2) for i in range(L)]
        r = R.segment_one(x, labels, blank)
        lp = torch.log_softmax(torch.from_numpy(x), -1).unsqueeze(1)
        nll = torch.nn.functional.ctc_loss(lp, torch.tensor([labels]), torch.tensor([T]), torch.tensor([L]), blank=blank,
                                           reduction="sum")
        assert abs(r["log_prob"] + float(nll)) < 1e-10 * max(1.0, abs(float(nll)))


def test_boundaries_are_ordered():
    """start[i] < end[i] <= start[i + 1] <= T, durations >= 1, confidences <= 0, over seeded draws of every scale."""
    rng = np.random.default_rng(11)
    for T, L, V in ((1, 1, 2), (2, 1, 3), (17, 5, 29), (63, 20, 29), (65, 32, 71), (129, 40, 128), (40, 37, 5), (30, 30, 4)):
        for scale in (0.1, 3.0, 10.0):
            x = rng.standard_normal((T, V)) * scale
            labels = [int(c) for c in rng.integers(1, V, L)]
            if L == T:
                labels = [1 + (i % (V - 1)) for i in range(L)]
            r = R.segment_one(x, labels, 0, sep=1)
            if not r["feasible"]:
                continue
            s, e = r["start"], r["end"]
            assert np.all(s < e) and np.all(e[:-1] <= s[1:]) and e[-1] <= T and s[0] >= 0
            assert np.all(r["duration"] >= 1 - 1e-9) and np.all(r["log_confidence"] <= 0)
            assert r["duration"].sum() <= T + 1e-9                    # the labels hold at most every frame
            for w in range(len(r["word_first"])):
                f, c = int(r["word_first"][w]), int(r["word_count"][w])
                assert all(l != 1 for l in labels[f:f + c]) and (f == 0 or labels[f - 1] == 1)
                assert f + c == L or labels[f + c] == 1
                assert r["word_start"][w] == s[f] and r["word_end"][w] == e[f + c - 1]
                d = r["duration"][f:f + c]
                assert abs(r["word_log_confidence"][w] - (d * r["log_confidence"][f:f + c]).sum() / d.sum()) < 1e-9


def test_planted_alignments_are_recovered_exactly():
    rng = np.random.default_rng(5)
    for L, V in ((1, 2), (3, 4), (8, 5), (20, 29), (40, 29), (15, 3)):
        x, labels, starts, ends = R.planted(rng, L, V)
        r = R.segment_one(x, labels, 0, sep=1)
        assert r["feasible"]
        assert list(r["start"]) == starts and list(r["end"]) == ends
        assert r["start_margin"].min() > 0.49 and r["end_margin"].min() > 0.49
        assert np.exp(r["log_confidence"]).min() > 0.99
        np.testing.assert_allclose(r["duration"], np.array(ends) - np.array(starts), atol=1e-3)


def test_edge_rules():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((6, 4))
    lp = R.log_softmax(x)
    r = R.segment_one(x[:0], [], 0)                      # no frame, no label
    assert r["feasible"] and r["log_prob"] == 0.0
    r = R.segment_one(x[:0], [1, 2], 0)                  # no frame, labels
    assert not r["feasible"] and r["log_prob"] == -np.inf and list(r["word_first"]) == [1] and list(r["word_count"]) == [1]
    r = R.segment_one(x, [], 0)                          # frames, no label: every frame is blank
    assert r["feasible"] and abs(r["log_prob"] - lp[:, 0].sum()) < 1e-12 and len(r["word_first"]) == 0
    for labels in ([2, 2, 2, 2], [1, 2, 3, 1, 2, 3, 1], [0], [1, 0, 2], [4], [-1], [1, 7]):      # too few frames; blank; out of range
        r = R.segment_one(x, labels, 0)
        assert not r["feasible"] and r["log_prob"] == -np.inf
        assert not r["start"].any() and not r["end"].any() and not r["duration"].any() and np.all(r["log_confidence"] == -np.inf)
        assert np.all(r["word_log_confidence"] == -np.inf) and not r["word_start"].any() and not r["word_end"].any()
    r = R.segment_one(x, [1, 2, 1, 2, 1, 2], 0)          # L = T without repeats: exactly one alignment
    assert r["feasible"] and list(r["start"]) == list(range(6)) and list(r["end"]) == list(range(1, 7))
    assert abs(r["log_prob"] - sum(lp[t, c] for t, c in enumerate([1, 2, 1, 2, 1, 2]))) < 1e-12
    np.testing.assert_allclose(r["duration"], 1.0, atol=1e-12)
    y = x.copy()
    y[:, 3] = -np.inf                                    # a class of probability zero: legal, and fatal only if the labels need it
    assert R.segment_one(y, [1, 2], 0)["feasible"] and not R.segment_one(y, [1, 3], 0)["feasible"]
    r = R.segment_one(x, [1, 2, 1, 3, 1, 1], 0)["word_first"]       # words: maximal runs of labels != sep
    assert list(r) == [1, 3]
    b = R.segment_batch(np.stack([x, x]), [9, -3], np.array([[2, 3, 1, 2], [2, 3, 1, 2]]), [3, 7], 0, 1)      # lengths are clamped
    assert b["feasible"][0] and not b["feasible"][1] and b["n_words"].tolist() == [1, 2]
    assert b["start"][0, 3] == 0 and b["duration"][0, 3] == 0 and b["word_count"][0].tolist() == [2, 0]


def test_library_checks_arguments_before_any_device_call(lib):
    wsb = lib.v100_ctc_segment_workspace_bytes
    assert wsb(32, 512, 100) == 32 * 512 * 100 * 12 and wsb(1, 1, 1) == 12 and wsb(2, 4096, 2047) == 2 * 4096 * 2047 * 12
    for B, T, L in ((0, 512, 100), (1, 0, 100), (1, 4097, 100), (1, 512, 0), (1, 512, 2048), (-1, 512, 100)):
        assert wsb(B, T, L) == -1
    assert lib.v100_ctc_segment_block() >= 1
    one = ctypes.c_void_p(16)
    req = [one, None, one, None, one, one, one, one, one, one]            # logits in_len labels lab_len ws log_prob start end duration log_conf
    word = [one] * 6
    good = (1, 8, 5, 3, 0)                               # B T V Lmax blank

    def call(req=req, word=word, dims=good, sep=1):
        return lib.v100_ctc_segment(*req, *word, *dims, sep, None)

    for bad in ((0, 8, 5, 3, 0), (1, 0, 5, 3, 0), (1, 4097, 5, 3, 0), (1, 8, 1, 3, 0), (1, 8, 129, 3, 0), (1, 8, 5, 0, 0),
                (1, 8, 5, 2048, 0), (1, 8, 5, 3, -1), (1, 8, 5, 3, 5)):
        assert call(dims=bad) == 1, bad
        assert call(word=[None] * 6, dims=bad) == 1, bad
    for k in (0, 2, 4, 5, 6, 7, 8, 9):                   # every required pointer; in_len and lab_len may be NULL
        assert call(req=req[:k] + [None] + req[k + 1:]) == 3, k
    for k in range(6):                                   # the word pointers: all or none
        assert call(word=word[:k] + [None] + word[k + 1:]) == 3, k
        assert call(word=[None] * k + [one] + [None] * (5 - k)) == 3, k


def test_wrapper_refuses_cpu_tensors():
    from voice100_amd import decode
    from voice100_amd.infer import ASRPipeline
    x, lab = torch.zeros(1, 4, 5), torch.ones(1, 2, dtype=torch.long)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        decode.ctc_segment(x, None, lab, None)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        decode.ctc_segment(x, torch.tensor([4]), lab, torch.tensor([2]), sep=None)
    assert decode.CTCSegments._fields == ("log_prob", "start", "end", "duration", "log_confidence", "word_first", "word_count",
                                          "word_start", "word_end", "word_log_confidence", "n_words")
    pipe = ASRPipeline(model=None)                       # no mel and no frame_seconds: the timed methods have no clock
    with pytest.raises(RuntimeError, match="frame_seconds"):
        pipe.segments(x)
    with pytest.raises(RuntimeError):
        pipe.transcribe_timed(["a.wav"], lambda ids: "")
    assert ASRPipeline(model=None, frame_seconds=0.02)._frame_seconds("segments") == 0.02
