"""CPU-side checks of the CTC prefix beam search feature (K24): the oracle of tests/_beam_ref.py against a brute-force sum over all
alignments, the share of seeded cases the forking oracle leaves undecided (so that the GPU test cannot hide behind them), the
library's exports and its host-side validation (which returns before anything touches a device), and the wrapper's refusal of CPU
tensors."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from _beam_ref import MAX_LEAVES, REL, SHAPES, accept, beam_search, beam_search_fork, brute_force, ctc_loglik, log_softmax, seeded_case


@pytest.mark.parametrize("T,V,reachable", [(5, 3, 25), (6, 2, 4), (4, 4, 61)])
def test_oracle_is_the_brute_force_sum(T, V, reachable):
    for blank in (0, V - 1):
        x = (np.random.default_rng(100 * T + V + blank).standard_normal((T, V)) * 2).astype(np.float32)
        lp = log_softmax(x)
        exact = brute_force(lp, blank)
        final = beam_search(x, 64, blank)                # nothing is pruned: every reachable prefix, with its whole probability
        assert len(exact) == reachable and {p for p, _ in final} == set(exact)
        assert all(abs(s - exact[p]) <= 1e-13 for p, s in final)
        assert all(abs(ctc_loglik(lp, list(p), blank) - s) <= 1e-13 for p, s in exact.items())
        assert [s for _, s in final] == sorted((s for _, s in final), reverse=True)
        assert abs(np.logaddexp.reduce([s for _, s in final])) <= 1e-13        # the probabilities of all prefixes sum to 1
        leaves = beam_search_fork(x, 64, blank)
        assert len(leaves) == 1 and leaves[0] == final
        assert accept(leaves, [p for p, _ in final], [s for _, s in final]) == (True, 0.0)


def test_oracle_hand_checked():
    assert beam_search(np.zeros((0, 5), np.float32), 4) == [((), 0.0)]       # no frame: the empty hypothesis, probability 1
    lp = np.log(np.array([[0.6, 0.4], [0.4, 0.6]]))                          # two frames, one label: "" 0.24, "1" 0.76
    final = dict(beam_search(lp, 4))
    assert math.isclose(final[()], math.log(0.24)) and math.isclose(final[(1,)], math.log(0.76)) and len(final) == 2
    (p, s), = beam_search(lp, 1)                         # one place: "1" is pruned after frame 0 and only comes back as "" + 1
    assert p == (1,) and math.isclose(s, math.log(0.36))
    # the pruned search never reports more than the exact likelihood
    x = (np.random.default_rng(5).standard_normal((30, 9)) * 3).astype(np.float32)
    for p, s in beam_search(x, 3):
        assert s <= ctc_loglik(log_softmax(x), list(p)) + 1e-12
    # a near-tie at the beam's edge forks: two classes of equal probability and one place
    tie = np.log(np.array([[0.2, 0.4, 0.4]]))
    leaves = beam_search_fork(tie, 1)
    assert sorted(leaf[0][0] for leaf in leaves) == [(1,), (2,)]
    assert accept(leaves, [(2,)], [math.log(0.4)])[0] and accept(leaves, [(1,)], [math.log(0.4)])[0]
    assert not accept(leaves, [()], [math.log(0.2)])[0] and not accept(leaves, [(1,)], [math.log(0.4) + 1e-3])[0]
    assert not accept(leaves, [(1,), (2,)], [math.log(0.4)] * 2)[0]          # a hypothesis the beam cannot hold
    assert accept(leaves, [(1,), ()], [math.log(0.4), -math.inf])[0]


def test_seeded_cases_are_decided():
    """At most 10 % of each seeded shape's cases may be undecided (more than MAX_LEAVES leaves)."""
    for i, (T, V, W, scale, nbest, cases) in enumerate(SHAPES):
        x, leaves = seeded_case(i)
        assert x.shape == (cases, T, V) and x.dtype == np.float32
        undecided = sum(leaf is None for leaf in leaves)
        assert undecided <= 0.1 * cases, (SHAPES[i], undecided)
        assert all(leaf is None or 1 <= len(leaf) <= MAX_LEAVES for leaf in leaves)
        for b in range(cases):                           # the plain recursion is one of the leaves
            if leaves[b] is not None:
                plain = beam_search(x[b], W)
                assert accept(leaves[b], [p for p, _ in plain[:nbest]], [s for _, s in plain[:nbest]])[0]
    assert REL == 2e-5


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
    assert hasattr(lib, "v100_ctc_beam_search") and hasattr(lib, "v100_ctc_beam_workspace_bytes")
    assert [n for _, n in protos["v100_ctc_beam_search"]] == ["logits", "lens", "ws", "ids", "ids_len", "scores", "B", "T", "V", "W", "nbest",
                                                              "blank", "stream"]
    assert [t for t, _ in protos["v100_ctc_beam_search"]] == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 6 + [ctypes.c_void_p]
    assert protos["v100_ctc_beam_workspace_bytes"] == [(ctypes.c_int, n) for n in ("B", "T", "V", "W")]
    assert lib.v100_ctc_beam_workspace_bytes.restype is ctypes.c_longlong and lib.v100_ctc_beam_search.restype is ctypes.c_int


def test_workspace_helper(lib):
    wsb = lib.v100_ctc_beam_workspace_bytes
    assert wsb(1, 1, 2, 1) > 0 and wsb(32, 4096, 128, 64) > 0
    for bad in ((0, 8, 29, 4), (1, 0, 29, 4), (1, 4097, 29, 4), (1, 8, 1, 4), (1, 8, 129, 4), (1, 8, 29, 0), (1, 8, 29, 65), (-1, 8, 29, 4)):
        assert wsb(*bad) == -1, bad
    for T in (1, 7, 512, 4096):                          # room for the trie (1 + W T nodes) and a table at load <= 1/2, per utterance
        for W in (1, 3, 16, 64):
            assert wsb(1, T, 29, W) >= 4 * (1 + W * T) + 8 * 2 * W * T
            assert wsb(5, T, 29, W) == 5 * wsb(1, T, 29, W) and wsb(1, T, 29, W) % 16 == 0
    grid = [wsb(1, T, 29, W) for T in (1, 2, 100, 101, 4096) for W in (1, 2, 63, 64)]
    assert all(wsb(1, T + 1, 29, W) >= wsb(1, T, 29, W) for T in (1, 99, 4095) for W in (1, 16, 64))       # monotone in T ...
    assert all(wsb(1, T, 29, W + 1) >= wsb(1, T, 29, W) for T in (1, 99, 4096) for W in (1, 16, 63))       # ... and in W
    assert all(g > 0 for g in grid)
    assert wsb(1 << 12, 4096, 128, 64) > 1 << 32         # a long long, not an int


def test_host_side_validation(lib):
    one = ctypes.c_void_p(16)                            # never dereferenced: every call below returns before any device call
    bs = lib.v100_ctc_beam_search
    ok = [one, one, one, one, one, one]                  # logits, lens, ws, ids, ids_len, scores
    for k in (0, 2, 3, 4, 5):                            # lens may be NULL, the others may not
        args = list(ok)
        args[k] = None
        assert bs(*args, 2, 16, 29, 8, 1, 0, None) == 3
    for B, T, V, W, nbest, blank in ((0, 16, 29, 8, 1, 0), (2, 0, 29, 8, 1, 0), (2, 4097, 29, 8, 1, 0), (2, 16, 1, 8, 1, 0),
                                     (2, 16, 129, 8, 1, 0), (2, 16, 29, 0, 1, 0), (2, 16, 29, 65, 1, 0), (2, 16, 29, 8, 0, 0),
                                     (2, 16, 29, 8, 9, 0), (2, 16, 29, 8, 1, -1), (2, 16, 29, 8, 1, 29)):
        assert bs(*ok, B, T, V, W, nbest, blank, None) == 1, (B, T, V, W, nbest, blank)
    assert bs(None, one, one, one, one, one, 0, 16, 29, 8, 1, 0, None) == 3  # a NULL pointer is reported before the shape


def test_wrapper_takes_gpu_tensors_only():
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.decode import ctc_beam_search
    from voice100_amd.infer import ASRPipeline
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ctc_beam_search(torch.zeros(2, 8, 29))
    with pytest.raises(RuntimeError):
        ASRPipeline(AudioToTextCTC(64, 32, 29, 32).eval(), beam_size=4).nbest(torch.zeros(2, 64, 64))
    pipe = ASRPipeline(AudioToTextCTC(64, 32, 29, 32).eval())
    assert pipe.beam_size is None and pipe.nbest_size == 1                  # the default is the greedy path
