"""CPU-side checks of the synthesis scores (K27): the float64 oracle of tests/_dtw_ref.py against brute-force enumeration of every
monotone path (cost, path and the tie rule), the library's exports and its host-side validation (which returns before anything
touches a device), the Python wrappers' refusal of CPU tensors, and the arithmetic of mcd_db and SynthesisScore.compute()."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from _dtw_ref import (backtrace, brute_force, dtw_matrix, local_distance, margin, rates_of, score_batch, score_pair, tie_rule_path,
                      totals_of)

SHAPES = [(n, m) for n in range(1, 6) for m in range(1, 6)]


def test_oracle_against_every_path_on_integer_data():
    """Small integers: ties are everywhere (hundreds of cheapest paths in a 5 x 5 case), every sum is exact, and the oracle's path
    must be the one the tie rule picks among the cheapest."""
    rng = np.random.RandomState(0)
    tied = 0
    for n, m in SHAPES:
        for _ in range(6):
            d = rng.randint(0, 3, (n, m)).astype(np.float64)
            C, mv = dtw_matrix(d)
            best, paths = brute_force(d)
            tied += len(paths) > 1
            assert C[-1, -1] == best, (n, m, d)
            assert backtrace(mv) == tie_rule_path(paths), (n, m, d)
    assert tied > 50                                     # the tie rule was exercised


def test_oracle_against_every_path_on_random_data():
    rng = np.random.RandomState(1)
    for n, m in SHAPES:
        for _ in range(3):
            x, y = rng.randn(n, 3).astype(np.float32), rng.randn(m, 3).astype(np.float32)
            d = local_distance(x, y)
            assert np.allclose(d[0, 0], np.linalg.norm(x[0].astype(np.float64) - y[0]))
            best, paths = brute_force(d)
            r = score_pair(x, y)
            assert r["cost"] == best and len(paths) == 1 and r["path"] == paths[0], (n, m)   # each path is summed from its start, as C is
            assert max(n, m) <= r["path_len"] <= n + m - 1
            assert r["margin"] > 0 or min(n, m) == 1


def test_oracle_hand_checked_cases():
    x = np.array([[0.0], [1.0], [1.0], [3.0]], np.float32)
    y = np.array([[0.0], [1.0], [3.0]], np.float32)
    r = score_pair(x, y, f0x=[100.0, 0.0, 200.0, 29.0], f0y=[100.0, 100.0, 30.0], f0_floor=30.0)
    assert r["cost"] == 0.0 and r["path"] == [(0, 0), (1, 1), (2, 1), (3, 2)] and r["path_len"] == 4
    # pairs: (100,100) voiced; (0,100) one voiced; (200,100) voiced, one octave = 1200 cents; (29,30) one voiced
    assert (r["voiced"], r["vuv_errors"], r["f0_sq_cents"], r["f0_sq_hz"]) == (2, 2, 1200.0 ** 2, 100.0 ** 2)
    assert r["margin"] == np.inf                         # every C on the path is 0 and no two predecessors tie there ...
    t = score_pair(np.zeros((2, 1), np.float32), np.zeros((2, 1), np.float32))
    assert t["path"] == [(0, 0), (1, 1)] and t["margin"] == 0.0          # ... here they do: a tie, decided for the diagonal
    s = score_pair(x, y, skip=0, dtw=False)
    assert s["path"] == [(0, 0), (1, 1), (2, 2)] and s["cost"] == 2.0
    e = score_batch(np.zeros((2, 3, 2), np.float32), [0, 9], np.ones((2, 4, 2), np.float32), [4, -1])
    assert [q["path_len"] for q in e] == [0, 0] and e[0]["cost"] == 0.0  # lengths clamp to [0, width]; an empty side gives zeros
    u = score_pair(np.array([[5.0, 1.0], [5.0, 2.0]], np.float32), np.array([[-7.0, 1.0]], np.float32), skip=1)
    assert u["cost"] == 1.0 and u["path"] == [(0, 0), (1, 0)]            # the skipped dimension does not count
    rows = [r, s]
    assert totals_of(rows) == [7.0, 2.0, 2.0, 2.0, 1200.0 ** 2, 100.0 ** 2]
    C, _ = dtw_matrix(np.array([[1.0, 2.0], [3.0, 1.0]]))
    assert C.tolist() == [[1.0, 3.0], [4.0, 2.0]] and margin(C, [(0, 0), (1, 1)]) == (3.0 - 1.0) / 2.0


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
    assert hasattr(lib, "v100_dtw_score") and hasattr(lib, "v100_dtw_workspace_bytes")
    assert [n for _, n in protos["v100_dtw_score"]] == ["x", "x_len", "y", "y_len", "f0x", "f0y", "ws", "cost", "path_len", "voiced",
                                                        "vuv_errors", "f0_sq_cents", "f0_sq_hz", "path", "totals", "B", "Tx", "Ty", "D",
                                                        "skip", "f0_floor", "mode", "stream"]
    assert protos["v100_dtw_score"][20][0] is ctypes.c_float
    assert [n for _, n in protos["v100_dtw_workspace_bytes"]] == ["B", "Tx", "Ty", "D", "want_path"]
    assert lib.v100_dtw_workspace_bytes.restype is ctypes.c_longlong


def test_host_side_validation(lib):
    one = ctypes.c_void_p(16)                            # never dereferenced: every call below returns before any device call
    score = lib.v100_dtw_score
    # x, x_len, y, y_len, f0x, f0y, ws, cost, path_len, voiced, vuv_errors, f0_sq_cents, f0_sq_hz, path, totals
    ok = [one] * 15
    shape = (4, 16, 16, 25, 1, 30.0, 0, None)            # B, Tx, Ty, D, skip, f0_floor, mode, stream

    def call(args, shp=shape):
        return score(*args, *shp)
    for k in (0, 2, 6):                                  # x, y or the workspace is NULL
        args = list(ok)
        args[k] = None
        assert call(args) == 3
    for k in (4, 5):                                     # one f0 track without the other
        args = list(ok)
        args[k] = None
        assert call(args) == 3
    for k in range(7, 13):                               # the six per-row outputs go together
        args = list(ok)
        args[k] = None
        assert call(args) == 3
    assert call(ok[:7] + [None] * 8) == 3                # no output at all
    assert call(ok[:7] + [None] * 6 + [one, one]) == 3   # a path without the per-row outputs
    # the lengths, the f0 tracks, the path and either side of the outputs are optional: these reach the shape check, which refuses
    bad = (4, 4097, 16, 25, 1, 30.0, 0, None)
    assert call([one, None, one, None, None, None, one] + [one] * 6 + [None, None], bad) == 1
    assert call(ok[:7] + [None] * 7 + [one], bad) == 1
    assert call(ok, (4, 4097, 16, 25, 1, 30.0, 0, None)) == 1
    assert call(ok, (4, 16, 4097, 25, 1, 30.0, 0, None)) == 1
    assert call(ok, (0, 16, 16, 25, 1, 30.0, 0, None)) == 1
    assert call(ok, (4, 0, 16, 25, 1, 30.0, 0, None)) == 1 and call(ok, (4, 16, 0, 25, 1, 30.0, 0, None)) == 1
    assert call(ok, (4, 16, 16, 65, 0, 30.0, 0, None)) == 1              # Du = 65
    assert call(ok, (4, 16, 16, 66, 1, 30.0, 0, None)) == 1
    assert call(ok, (4, 16, 16, 25, 25, 30.0, 0, None)) == 1 and call(ok, (4, 16, 16, 25, -1, 30.0, 0, None)) == 1    # 0 <= skip < D
    assert call(ok, (4, 16, 16, 25, 1, 30.0, 2, None)) == 1 and call(ok, (4, 16, 16, 25, 1, 30.0, -1, None)) == 1     # the mode
    wsb = lib.v100_dtw_workspace_bytes
    assert wsb(32, 1000, 1100, 25, 0) > 0 and wsb(1, 4096, 4096, 64, 1) > wsb(1, 4096, 4096, 64, 0) > 0
    assert wsb(32, 4097, 300, 25, 0) == -1 and wsb(32, 512, 4097, 25, 0) == -1 and wsb(0, 512, 300, 25, 0) == -1
    assert wsb(32, 0, 300, 25, 0) == -1 and wsb(32, 300, 0, 25, 1) == -1 and wsb(32, 300, 300, 0, 0) == -1
    assert wsb(64, 4096, 4096, 25, 1) > 1 << 32          # a long long, not an int


def test_wrappers_take_gpu_tensors_only():
    from voice100_amd.metrics import SynthesisScore, dtw_score
    x, n = torch.zeros(2, 8, 25), torch.tensor([8, 3], dtype=torch.int32)
    f0 = torch.zeros(2, 8)
    with pytest.raises(RuntimeError):
        dtw_score(x, n, x, n)
    with pytest.raises(RuntimeError):
        dtw_score(x, None, x, None, f0, f0, skip=1, dtw=False)
    with pytest.raises(RuntimeError):
        SynthesisScore().update(f0, x, n, f0, x, n)
    from voice100_amd.infer import TTSPipeline, TTSPipelineV2
    assert callable(TTSPipeline.score) and callable(TTSPipeline.evaluate)
    assert callable(TTSPipelineV2.score) and callable(TTSPipelineV2.evaluate)


def test_mcd_db_arithmetic():
    from voice100_amd.metrics import mcd_db
    k = 10.0 / math.log(10.0) * math.sqrt(2.0)
    assert mcd_db(3.0, 4) == k * 3.0 / 4 and math.isnan(mcd_db(0.0, 0))
    assert abs(k - 6.1418515) < 1e-6                     # the constant every MCD paper quotes
    out = mcd_db(torch.tensor([3.0, 0.0, 5.0], dtype=torch.float64), torch.tensor([4, 0, 1], dtype=torch.int32))
    assert out.dtype == torch.float64 and out[0] == k * 3.0 / 4 and math.isnan(float(out[1])) and out[2] == k * 5.0


def test_synthesis_score_compute_arithmetic():
    from voice100_amd.metrics import SynthesisScore
    m = SynthesisScore()
    out = m.compute()                                    # nothing scored yet: every denominator is 0
    assert all(math.isnan(out[k]) for k in ("mcd", "f0_rmse_cents", "f0_rmse_hz", "vuv_error"))
    assert out["frames"] == out["voiced_frames"] == out["utterances"] == 0
    m.totals = torch.tensor([200.0, 150.0, 120.0, 10.0, 120.0 * 2500.0, 120.0 * 16.0], dtype=torch.float64)
    m.utterances = 3
    out = m.compute()
    assert out == {"mcd": 10.0 / math.log(10.0) * math.sqrt(2.0) * 150.0 / 200.0, "f0_rmse_cents": 50.0, "f0_rmse_hz": 4.0,
                   "vuv_error": 0.05, "frames": 200, "voiced_frames": 120, "utterances": 3}
    assert type(out["mcd"]) is float and type(out["frames"]) is int
    assert out == rates_of(m.totals.tolist(), 3)
    m.totals = torch.tensor([50.0, 10.0, 0.0, 50.0, 0.0, 0.0], dtype=torch.float64)         # no pair with both frames voiced
    out = m.compute()
    assert math.isnan(out["f0_rmse_cents"]) and math.isnan(out["f0_rmse_hz"]) and out["vuv_error"] == 1.0 and out["voiced_frames"] == 0
    m.totals = torch.tensor([float((1 << 50) + 1), 1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)   # counts are exact below 2^53
    assert m.compute()["frames"] == (1 << 50) + 1
    m.reset()
    assert m.compute()["frames"] == 0 and m.utterances == 0
