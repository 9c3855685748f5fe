"""decode.mbr_nbest (K35) without a GPU: the float64 oracle of tests/_mbr_ref.py against a brute-force definition, the arithmetic of its
bounds, the condition on the case list that makes the GPU test's ranking comparison exact, the refusals of mbr_nbest, of the pipelines
and of the C ABI before any device call, and the kernels' bodies -- compiled as a plain host program from tools/mbr_host.cpp, no
sanitizer here -- against the oracle on the whole case list."""
import ctypes
import functools
import itertools
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _mbr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_distance(a, b):
    """the definition: the least number of insertions, deletions and substitutions, by recursion on the last tokens"""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
    return d(len(a), len(b))


def test_levenshtein_against_the_definition():
    rows = [tuple(r) for n in range(4) for r in itertools.product((1, 2), repeat=n)]
    for a, b in itertools.product(rows, rows):
        assert R.levenshtein(a, b) == brute_distance(a, b), (a, b)
    assert R.levenshtein("aaa", "aa") == 1 and R.levenshtein("abab", "ab") == 2 and R.levenshtein("kitten", "sitting") == 3
    rng = np.random.default_rng(0)
    for n, m in ((150, 140), (129, 200), (300, 1)):      # the numpy rows against the textbook loop
        a, b = rng.integers(0, 4, n).tolist(), rng.integers(0, 4, m).tolist()
        assert n * m > 1 << 14 or m == 1
        prev = list(range(m + 1))
        for i in range(1, n + 1):
            cur = [i] + [0] * m
            for j in range(1, m + 1):
                cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
            prev = cur
        assert R.levenshtein(a, b) == prev[m]


def test_split_tokens():
    assert R.split_tokens([1, 1, 5, 6, 1, 1, 7, 1, 9], 8, 1) == [(5, 6), (7,)]
    assert R.split_tokens([1, 1], 2, 1) == [] == R.split_tokens([5], 0, 1) == R.split_tokens([5], -3, None)
    assert R.split_tokens([1, 5, 1], 3, None) == [(1,), (5,), (1,)]


def test_the_oracle_by_hand():
    ids, lens, scores = R.flip_case()
    ref = R.oracle(ids, lens, scores)
    assert ref["dist"].tolist() == [[[0, 4, 4], [4, 0, 1], [4, 1, 0]]] and ref["n_tokens"].tolist() == [[4, 4, 4]]
    assert ref["posterior"][0] == pytest.approx([0.4, 0.3, 0.3], rel=1e-6)
    assert ref["risk"][0] == pytest.approx([2.4, 1.9, 1.9], rel=1e-6) and ref["expected_len"][0] == pytest.approx(4.0, rel=1e-6)
    assert ref["order"].tolist() == [[1, 2, 0]]          # the MBR choice is not the best score; the tie keeps the given order
    # an absent hypothesis, a reference, the id level
    ids, lens = R.pack([[[5, 1, 6], [5, 6], [5, 1, 7]]])
    scores = np.array([[0.0, -math.inf, math.log(0.5)]], dtype=np.float32)
    ref = R.oracle(ids, lens, scores, sep=None, ref=np.array([[5, 1, 6, 9]]), ref_len=np.array([3]))
    assert ref["dist"].tolist() == [[[0, -1, 1], [-1, -1, -1], [1, -1, 0]]] and ref["ref_dist"].tolist() == [[0, -1, 1]]
    assert ref["ref_n"].tolist() == [3] and ref["order"].tolist() == [[0, 2, 1]] and ref["n_tokens"].tolist() == [[3, 0, 3]]
    assert ref["posterior"][0] == pytest.approx([2 / 3, 0.0, 1 / 3]) and ref["risk"][0, 1] == math.inf
    assert ref["risk"][0, [0, 2]] == pytest.approx([1 / 3, 2 / 3])
    none = R.oracle(ids, lens, np.full((1, 3), np.nan, dtype=np.float32))
    assert none["order"].tolist() == [[0, 1, 2]] and not none["posterior"].any() and np.all(none["risk"] == math.inf) and np.all(none["dist"] == -1)
    # the risk is the definition, term by term, for every case of the list
    for name, ids, lens, scores, kw in R.case_list()[:8]:
        ref = R.oracle(ids, lens, scores, **kw)
        for b in range(ids.shape[0]):
            live = np.isfinite(ref["risk"][b])
            want = (ref["dist"][b][:, live] * ref["posterior"][b][live]).sum(axis=1)
            assert ref["risk"][b][live] == pytest.approx(want[live], rel=1e-12), name
            assert ref["posterior"][b].sum() == pytest.approx(1.0 if live.any() else 0.0, rel=1e-12)


def test_bounds():
    assert R.bound(0.0) == 2.0 ** -149 and R.bound(1.0) == 2.0 ** -23 + 2.0 ** -149 and R.bound(-4.0) == R.bound(4.0)
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(0, 5000, 1000), 10.0 ** rng.uniform(-44, 0, 1000), [0.0, 1e-45, 2.0 ** -149, 2.0 ** -126]])
    assert np.all(np.abs(x.astype(np.float32).astype(np.float64) - x) <= R.bound(x) / 2)      # one fp32 rounding is half the bound


def test_case_list_is_well_separated():
    names = set()
    flips = 0
    for name, ids, lens, scores, kw in R.case_list():
        assert name not in names and ids.dtype == np.int64 and lens.dtype == np.int32 and scores.dtype == np.float32
        names.add(name)
        ref = R.oracle(ids, lens, scores, **kw)
        assert R.well_separated(ref) == [], name
        flips += int(np.any(ref["order"][:, 0] != 0))
        assert R.check(name, {**{k: ref[k] for k in ("order", "dist", "ref_dist", "ref_n", "expected_len")},
                              **gathered(ref, ids, lens, scores)}, ref, ids, lens, scores)[0] == []
    assert len(names) >= 25 and flips >= 3
    assert {ids.shape[1] for _, ids, _, _, _ in R.case_list()} >= {1, 2, 3, 64}


def gathered(ref, ids, lens, scores):
    rows, order = np.arange(ids.shape[0])[:, None], ref["order"].astype(np.int64)
    return {"ids": ids[rows, order], "lens": lens[rows, order], "scores": scores[rows, order], "n_tokens": ref["n_tokens"][rows, order],
            "risk": ref["risk"][rows, order].astype(np.float32), "posterior": ref["posterior"][rows, order].astype(np.float32)}


def test_check_sees_a_wrong_result():
    name, ids, lens, scores, kw = R.case_list()[2]
    ref = R.oracle(ids, lens, scores, **kw)
    good = {**{k: ref[k] for k in ("order", "dist", "ref_dist", "ref_n", "expected_len")}, **gathered(ref, ids, lens, scores)}
    for k, change in (("risk", lambda a: a * np.float32(1 + 2.0 ** -21)), ("dist", lambda a: a + np.eye(3, dtype=np.int32)),
                      ("order", lambda a: a[:, ::-1]), ("posterior", lambda a: a + np.float32(1e-6))):
        assert R.check(name, {**good, k: change(good[k].copy())}, ref, ids, lens, scores)[0] != [], k


def test_mbr_nbest_refuses_cpu_tensors_and_bad_arguments():
    from voice100_amd.decode import MBR, mbr_nbest
    assert MBR._fields == R.FIELDS
    ids, lens, scores = (torch.from_numpy(a) for a in R.flip_case())
    with pytest.raises(RuntimeError, match="mbr_nbest: GPU tensors only"):
        mbr_nbest(ids, lens, scores)
    with pytest.raises(RuntimeError, match="mbr_nbest: GPU tensors only"):
        mbr_nbest(ids, lens, scores, ref=ids[:, 0], ref_len=lens[:, 0])


def test_pipelines_refuse_bad_mbr_arguments():
    from voice100_amd.infer import ASRPipeline, LongASRPipeline
    for make in (lambda **kw: ASRPipeline(None, **kw), lambda **kw: LongASRPipeline(None, **kw)):
        with pytest.raises(RuntimeError, match="mbr needs a beam_size"):
            make(mbr="word")
        with pytest.raises(RuntimeError, match="must be None"):
            make(mbr="char", beam_size=8)
        with pytest.raises(RuntimeError, match="mbr_scale"):
            make(mbr="word", beam_size=8, mbr_scale=-1.0)
        with pytest.raises(RuntimeError, match="mbr_scale"):
            make(mbr="id", beam_size=8, mbr_scale=math.nan)
        with pytest.raises(RuntimeError, match="mbr_size = 9 <= beam_size = 8"):
            make(mbr="word", beam_size=8, mbr_size=9)
        p = make(mbr="id", beam_size=8, mbr_scale=2)
        p = getattr(p, "asr", p)
        assert (p.mbr, p.mbr_scale, p.mbr_size) == ("id", 2.0, 8)
        p = make(beam_size=8)
        p = getattr(p, "asr", p)
        assert (p.mbr, p.mbr_size) == (None, None)
    with pytest.raises(RuntimeError, match="nbest = 4 <= mbr_size = 2"):
        ASRPipeline(None, beam_size=8, nbest=4, mbr="word", mbr_size=2)
    assert ASRPipeline(None, beam_size=8, nbest=2, mbr="word", mbr_size=5).mbr_size == 5


def test_abi_limits_before_any_device_call():
    from voice100_amd import _native as N
    lib = N.load()
    protos = N.parse_header()
    assert protos["v100_nbest_mbr_workspace_bytes"].restype is ctypes.c_longlong and len(protos["v100_nbest_mbr"]) == 25
    assert protos["v100_nbest_mbr"][23] == (ctypes.c_double, "scale")
    size = lib.v100_nbest_mbr_workspace_bytes
    for shape in ((0, 2, 8, 0), (1, 0, 8, 0), (1, 65, 8, 0), (1, 2, 0, 0), (1, 2, 4097, 0), (1, 2, 8, -1), (1, 2, 8, 4097)):
        assert size(*shape) == -1, shape
    # tokens, the table (load <= 1/2), the counts and the word bounds of every row, the reference's included
    assert size(1, 2, 8, 0) == 4 * 16 + 4 * 128 + 4 * 68 + 4 * 16
    assert size(3, 16, 512, 600) == 3 * (4 * 17 * 600 + 4 * 32768 + 4 * 68 + 4 * 17 * 600)
    assert size(1, 64, 4096, 4096) == 4 * 65 * 4096 * 2 + 4 * (1 << 20) + 4 * 68
    one = ctypes.c_void_p(16)                            # never dereferenced: every call below returns before any device call
    call = lambda a, B=1, nbest=2, T=8, Tr=0, scale=1.0: lib.v100_nbest_mbr(*a, B, nbest, T, Tr, 1, 1, scale, None)      # noqa: E731
    ok = [one, one, one, None, None] + [one] * 12
    for k in (0, 1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16):
        assert call(ok[:k] + [None] + ok[k + 1:]) == 3, k
    with_ref = [one] * 17
    assert call(with_ref[:3] + [None] + with_ref[4:], Tr=4) == 3 and call(with_ref[:4] + [None] + with_ref[5:], Tr=4) == 3
    assert call(with_ref[:14] + [None] + with_ref[15:], Tr=4) == 3 and call(with_ref[:15] + [None] + with_ref[16:], Tr=4) == 3
    no_ref_out = ok[:14] + [None, None] + ok[16:]
    for kw in (dict(B=0), dict(nbest=0), dict(nbest=65), dict(T=0), dict(T=4097), dict(Tr=4), dict(scale=-0.5), dict(scale=math.inf),
               dict(scale=math.nan)):
        assert call(no_ref_out, **kw) == 1, kw
    assert call(with_ref, Tr=0) == 1 and call(with_ref, Tr=4097) == 1


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    return None


def test_host_program_against_the_oracle(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler (CXX, c++, g++, clang++) on this machine")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import mbr_host
    finally:
        sys.path.pop(0)
    exe = str(tmp_path / "mbr_host")
    mbr_host.build(cxx, exe)
    assert mbr_host.run_cases(exe, str(tmp_path), R.case_list()) == []
    assert subprocess.run([exe, "--adversarial"], capture_output=True).returncode == 0
