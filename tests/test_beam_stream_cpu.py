"""CPU-side checks of the resumable beam search (K32): the library's exports, the size helpers' documented byte counts, the host-side
validation (which returns before anything touches a device), the wrappers' refusal of CPU tensors, the chunk / length plan of
ctc_beam_search_long against a brute-force loop, and the planted fixture of tests/_beam_stream_cases.py against the scores its
docstring quotes."""
import ctypes
import os

import numpy as np
import pytest
import torch

from _beam_stream_cases import LONG, LONG_SCORES, long_leaves, planted


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


NAMES = ("v100_ctc_beam_stream_workspace_bytes", "v100_ctc_beam_stream_state_bytes", "v100_ctc_beam_stream_push",
         "v100_ctc_beam_stream_push_lm", "v100_ctc_beam_stream_read", "v100_ctc_beam_stream_read_lm")


def test_library_exports_and_prototypes(lib):
    from voice100_amd import _native as N
    protos = N.parse_header()
    assert all(hasattr(lib, n) and n in protos for n in NAMES)
    assert protos[NAMES[0]] == [(ctypes.c_int, n) for n in ("B", "max_frames", "V", "W")]
    assert protos[NAMES[1]] == [(ctypes.c_int, n) for n in ("B", "W")]
    assert [n for _, n in protos[NAMES[2]]] == ["logits", "lens", "ws", "state", "B", "T", "max_frames", "V", "W", "blank", "stream"]
    assert [n for _, n in protos[NAMES[4]]] == ["ws", "state", "ids", "ids_len", "scores", "B", "max_frames", "V", "W", "nbest", "width",
                                                "stream"]
    assert all(getattr(lib, n).restype is ctypes.c_longlong for n in NAMES[:2]) and all(getattr(lib, n).restype is ctypes.c_int
                                                                                        for n in NAMES[2:])


def test_size_helpers_give_the_documented_bytes(lib):
    wsb, stb = lib.v100_ctc_beam_stream_workspace_bytes, lib.v100_ctc_beam_stream_state_bytes
    for F in (1, 7, 4096, 4097, 90000):
        for W in (1, 4, 16, 64):
            P = 64
            while P < 2 * W * F:
                P *= 2
            assert wsb(1, F, 29, W) == 8 * P + 4 * ((1 + W * F + 3) & ~3), (F, W)
            assert wsb(3, F, 29, W) == 3 * wsb(1, F, 29, W) and wsb(1, F, 29, W) % 16 == 0
            assert stb(1, W) == (32 + 40 * W + 15) & ~15 and stb(5, W) == 5 * stb(1, W)
    assert 30e6 <= wsb(1, 90000, 29, 16) <= 50e6         # the docstring's 30-minute recording at beam 16
    assert wsb(1, 4096, 29, 16) == lib.v100_ctc_beam_workspace_bytes(1, 4096, 29, 16)    # one call's region, at its largest
    assert wsb(1, (1 << 19) - 1, 29, 64) > 1 << 29 and wsb(1, (1 << 21) - 1, 29, 16) > 0            # the limits are inside ...
    for bad in ((0, 8, 29, 4), (1, 0, 29, 4), (1, 8, 1, 4), (1, 8, 129, 4), (1, 8, 29, 0), (1, 8, 29, 65), (-1, 8, 29, 4),
                (1, 1 << 19, 29, 64), (1, 1 << 21, 29, 16), (1, 1 << 25, 29, 1)):                  # ... W max_frames = 2^25 is not
        assert wsb(*bad) == -1, bad
    for bad in ((0, 4), (1, 0), (1, 65), (-2, 4)):
        assert stb(*bad) == -1, bad


def test_host_side_validation(lib):
    one = ctypes.c_void_p(16)                            # never dereferenced: every call below returns before any device call
    push, push_lm, read, read_lm = (getattr(lib, n) for n in NAMES[2:])
    for k in (0, 2, 3):                                  # logits, lens, ws, state: lens may be NULL
        args = [one] * 4
        args[k] = None
        assert push(*args, 2, 16, 100, 29, 8, 0, None) == 3
    for k in (0, 2, 3, 4, 5, 6):
        args = [one] * 7
        args[k] = None
        assert push_lm(*args, 3, 0, 0.5, 0.0, 2, 16, 100, 29, 8, 0, None) == 3
    for k in range(5):
        args = [one] * 5
        args[k] = None
        assert read(*args, 2, 100, 29, 8, 1, 16, None) == 3
    for k in range(8):                                   # ws, state, ids, ids_len, scores, lm_final | ctc_scores, lm_scores
        args = [one] * 8
        args[k] = None
        assert read_lm(*args[:6], 3, 0, 0.5, 0.0, 1, *args[6:], 2, 100, 29, 8, 1, 16, None) == 3
    for B, T, F, V, W, blank in ((0, 16, 100, 29, 8, 0), (2, 0, 100, 29, 8, 0), (2, 4097, 5000, 29, 8, 0), (2, 16, 0, 29, 8, 0),
                                 (2, 16, 1 << 22, 29, 8, 0), (2, 16, 100, 1, 8, 0), (2, 16, 100, 129, 8, 0), (2, 16, 100, 29, 0, 0),
                                 (2, 16, 100, 29, 65, 0), (2, 16, 100, 29, 8, -1), (2, 16, 100, 29, 8, 29)):
        assert push(one, one, one, one, B, T, F, V, W, blank, None) == 1, (B, T, F, V, W, blank)
        assert push_lm(*[one] * 7, 3, 0, 0.5, 0.0, B, T, F, V, W, blank, None) == 1
    for S, start, alpha in ((0, 0, 0.5), (3, 3, 0.5), (3, -1, 0.5), (3, 0, float("nan")), (3, 0, float("inf"))):
        assert push_lm(*[one] * 7, S, start, alpha, 0.0, 2, 16, 100, 29, 8, 0, None) == 1
        assert read_lm(*[one] * 6, S, start, alpha, 0.0, 1, one, one, 2, 100, 29, 8, 1, 16, None) == 1
    for nbest, width in ((0, 16), (9, 16), (1, 0)):
        assert read(*[one] * 5, 2, 100, 29, 8, nbest, width, None) == 1
        assert read_lm(*[one] * 6, 3, 0, 0.5, 0.0, 1, one, one, 2, 100, 29, 8, nbest, width, None) == 1
    assert push(None, one, one, one, 0, 16, 100, 29, 8, 0, None) == 3       # a NULL pointer is reported before the shape


def test_wrappers_take_gpu_tensors_only():
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.decode import CTCBeamStream, ctc_beam_search_long
    from voice100_amd.infer import LongASRPipeline
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        CTCBeamStream(2, 29, device="cpu")
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        ctc_beam_search_long(torch.zeros(2, 8, 29))
    model = AudioToTextCTC(64, 32, 29, 32).eval()
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        LongASRPipeline(model, beam_size=4).whole(logits=torch.zeros(8, 29))
    with pytest.raises(RuntimeError, match="greedily"):
        LongASRPipeline(model).whole(logits=torch.zeros(8, 29))


@pytest.mark.parametrize("T,chunk", [(1, 1), (10, 1), (10, 3), (10, 10), (10, 4096), (4200, 333), (4200, 4096), (8192, 4096), (4097, 4096)])
def test_chunk_plan_against_a_brute_force_loop(T, chunk):
    from voice100_amd.decode import beam_chunk_lengths, beam_chunk_plan
    plan = beam_chunk_plan(T, chunk)
    lengths = [0, 1, T // 2, T - 1, T, T + 5, -3]
    lens = torch.tensor(lengths, dtype=torch.int32)
    got = torch.stack([beam_chunk_lengths(lens, start, frames) for start, frames in plan]).tolist()
    owner = [None] * T                                   # the brute force: frame by frame, which chunk holds it
    for j, (start, frames) in enumerate(plan):
        assert 1 <= frames <= chunk and (frames == chunk or j == len(plan) - 1)
        for t in range(start, start + frames):
            assert owner[t] is None
            owner[t] = j
    assert None not in owner and owner == sorted(owner)
    for r, n in enumerate(lengths):
        want = [0] * len(plan)
        for t in range(min(max(n, 0), T)):               # the frames that one call on the whole row would run
            want[owner[t]] += 1
        assert [row[r] for row in got] == want, (n, want)
    for bad in ((0, 4), (8, 0), (8, 4097)):
        with pytest.raises(ValueError):
            beam_chunk_plan(*bad)


def test_planted_fixture_gives_the_quoted_scores():
    x = planted(LONG["T"], LONG["V"], LONG["seed"], LONG["peak"])
    assert x.shape == (4200, 8) and x.dtype == np.float32
    for leaves, want in zip(long_leaves(), LONG_SCORES):
        assert leaves is not None and len(leaves) == 1                       # decided, one leaf each
        assert abs(leaves[0][0][1] - want) <= 0.005, (leaves[0][0][1], want)
