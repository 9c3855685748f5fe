"""CPU-side checks of the edit-distance feature (K23): the two host references of tests/_edit_ref.py against one another and against
hand-checked cases, the word splitter against str.split(), the library's exports and its host-side validation (which returns before
anything touches a device), the Python wrappers' refusal of CPU tensors, and ErrorRate.compute()'s arithmetic."""
import ctypes
import math
import os
import random

import numpy as np
import pytest
import torch

from _edit_ref import lev_loop, lev_rows, score_rows, split_words, word_ids

ALPHABET = " abc"                                        # id 0 is the space of the str.split() cross-check


def _pairs(seed, count):
    rng = random.Random(seed)
    for _ in range(count):
        v = rng.choice((2, 3, 29))
        yield ([rng.randrange(v) for _ in range(rng.randint(0, 12))], [rng.randrange(v) for _ in range(rng.randint(0, 12))])


def test_the_two_host_references_agree():
    for a, b in _pairs(0, 3000):
        assert lev_loop(a, b) == lev_rows(a, b), (a, b)


def test_splitter_is_str_split():
    for a, b in _pairs(1, 3000):
        for row in (a, b):
            row = [x % 4 for x in row]
            text = "".join(ALPHABET[x] for x in row)
            assert ["".join(ALPHABET[x] for x in w) for w in split_words(row, 0)] == text.split(), text
    assert split_words([1, 1, 5, 6, 1, 1, 7, 1], 1) == [(5, 6), (7,)]
    assert split_words([1, 1, 1], 1) == [] and split_words([], 1) == []
    assert word_ids([(5, 6), (7,)], [(7,), (5,), (5, 6)]) == ([0, 1], [1, 2, 0])


def test_hand_checked_cases():
    k, s = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    assert lev_loop(k, s) == lev_rows(k, s) == 3
    for n in (0, 1, 7):
        row = list(range(n))
        assert lev_loop([], row) == lev_rows([], row) == n
        assert lev_loop(row, []) == lev_rows(row, []) == n
        assert lev_loop(row, row) == lev_rows(row, row) == 0
    # "the cat sat" against "the cat sat down": one inserted word; 5 inserted characters
    enc = lambda t: [1 if c == " " else ord(c) for c in t]  # noqa: E731
    h, r = np.array([enc("the cat sat") + [0] * 5]), np.array([enc("the cat sat down")])
    assert score_rows(h, [11], r, [16]) == [[5], [11], [16]]
    assert score_rows(h, [11], r, [16], sep=1) == [[1], [3], [4]]
    assert score_rows(h, [99], r, [-3]) == [[16], [16], [0]]                 # lengths clamp to [0, width]


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


def test_library_exports_and_prototypes(lib):
    from voice100_amd import _native as N
    protos = N.parse_header()
    assert hasattr(lib, "v100_edit_distance") and hasattr(lib, "v100_edit_distance_workspace_bytes")
    assert [n for _, n in protos["v100_edit_distance"]] == ["hyp", "hyp_len", "ref", "ref_len", "ws", "dist", "hyp_n", "ref_n", "totals",
                                                            "B", "Th", "Tr", "levels", "sep", "stream"]
    assert protos["v100_edit_distance"][13][0] is ctypes.c_longlong          # the separator is a 64-bit id
    assert lib.v100_edit_distance_workspace_bytes.restype is ctypes.c_longlong


def test_host_side_validation(lib):
    one = ctypes.c_void_p(16)                            # never dereferenced: every call below returns before any device call
    ed = lib.v100_edit_distance
    ok = [one, one, one, one, one, one, one, one, one]   # hyp, hyp_len, ref, ref_len, ws, dist, hyp_n, ref_n, totals
    for k in range(5):                                   # a required input or the workspace is NULL
        args = list(ok)
        args[k] = None
        assert ed(*args, 4, 16, 16, 3, 1, None) == 3
    assert ed(one, one, one, one, one, None, None, None, None, 4, 16, 16, 3, 1, None) == 3       # no output at all
    assert ed(one, one, one, one, one, one, None, one, one, 4, 16, 16, 3, 1, None) == 3          # the per-row outputs go together
    assert ed(*ok, 4, 4097, 16, 3, 1, None) == 1
    assert ed(*ok, 4, 16, 4097, 3, 1, None) == 1
    assert ed(*ok, 0, 16, 16, 3, 1, None) == 1
    assert ed(*ok, 4, 0, 16, 3, 1, None) == 1
    assert ed(*ok, 4, 16, 16, 0, 1, None) == 1 and ed(*ok, 4, 16, 16, 4, 1, None) == 1
    wsb = lib.v100_edit_distance_workspace_bytes
    assert wsb(32, 512, 300) > 0 and wsb(1, 4096, 4096) > 0
    assert wsb(32, 4097, 300) < 0 and wsb(32, 512, 4097) < 0 and wsb(0, 512, 300) < 0 and wsb(32, 0, 300) < 0
    assert wsb(1 << 20, 4096, 4096) > 1 << 32            # a long long, not an int


def test_wrappers_take_gpu_tensors_only():
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.decode import edit_distance, edit_distance_both
    from voice100_amd.infer import ASRPipeline, ErrorRate
    ids, n = torch.zeros(2, 8, dtype=torch.int64), torch.tensor([8, 3], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        edit_distance(ids, n, ids, n)
    with pytest.raises(RuntimeError):
        edit_distance(ids, n, ids, n, sep=1)
    with pytest.raises(RuntimeError):
        edit_distance_both(ids, n, ids, n)
    with pytest.raises(RuntimeError):
        ErrorRate().update(ids, n, ids, n)
    with pytest.raises(RuntimeError):
        ASRPipeline(AudioToTextCTC(64, 32, 29, 32).eval()).score(torch.zeros(2, 64, 64), torch.tensor([64, 40]), ids, n)


def test_error_rate_compute_arithmetic():
    from voice100_amd.infer import ErrorRate
    m = ErrorRate()
    out = m.compute()                                    # nothing scored yet: no reference token
    assert math.isnan(out["cer"]) and math.isnan(out["wer"]) and out["chars"] == out["words"] == out["utterances"] == 0
    m.totals = torch.tensor([[7, 95, 100], [3, 19, 20]], dtype=torch.int64)  # errors, hypothesis tokens, reference tokens
    m.utterances = 4
    out = m.compute()
    assert out == {"cer": 7 / 100, "wer": 3 / 20, "char_errors": 7, "chars": 100, "word_errors": 3, "words": 20, "utterances": 4}
    assert type(out["cer"]) is float and type(out["char_errors"]) is int
    m.totals = torch.tensor([[5, 5, 0], [2, 2, 0]], dtype=torch.int64)       # errors against empty references
    out = m.compute()
    assert math.isnan(out["cer"]) and math.isnan(out["wer"]) and out["char_errors"] == 5 and out["word_errors"] == 2
    m.totals = torch.tensor([[(1 << 40) + 1, 0, 1 << 41], [0, 0, 1]], dtype=torch.int64)      # the totals are 64-bit
    out = m.compute()
    assert out["char_errors"] == (1 << 40) + 1 and out["cer"] == ((1 << 40) + 1) / (1 << 41) and out["wer"] == 0.0
    m.reset()
    assert m.compute()["chars"] == 0 and m.utterances == 0
    p = ErrorRate(sep=None)
    p.totals = torch.tensor([[4, 30, 32]], dtype=torch.int64)
    p.utterances = 2
    assert p.compute() == {"cer": 4 / 32, "char_errors": 4, "chars": 32, "utterances": 2}
