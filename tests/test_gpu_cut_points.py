"""decode.ctc_cut_points (K31, csrc/cut_points.hip) on the GPU: the tables must EQUAL the numpy mirror tests/_cut_points_ref.py on a case
list built around the kernel's seams (the 64-frame word, the pass of its run scan, many passes), degenerate rows, ties and forced cuts;
the independent checker's promises must hold on every row; the greedy decode of the segments, concatenated, must be the greedy decode
of the row wherever no cut is forced; two calls give equal bits; nothing but zeros lies beyond n_seg."""
import functools

import numpy as np
import pytest
import torch

import _cut_points_ref as R

pytestmark = pytest.mark.gpu

SPAN, PASS = 64, 32768                                    # what the case list was built for; checked against the library below
N_CASES = 57


@functools.lru_cache(maxsize=None)
def cases():
    return R.case_list(SPAN, PASS)


@functools.lru_cache(maxsize=None)
def expected(i):
    name, x, lengths, kw = cases()[i]
    return R.mirror(x, lengths, **kw)


def run(x, lengths, kw, dev):
    from voice100_amd.decode import ctc_cut_points
    lens = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).to(dev)
    return ctc_cut_points(torch.from_numpy(x).to(dev), lens, **kw)


def test_case_list_matches_the_kernels_tiles(cuda):
    from voice100_amd import _native as N
    assert N.helper("v100_ctc_cut_points_span") == SPAN and N.helper("v100_ctc_cut_points_pass") == PASS
    assert len(cases()) == N_CASES
    lengths = {c[1].shape[1] for c in cases()}
    assert {1, 2, 63, 64, 65, PASS - 1, PASS, PASS + 1} <= lengths and max(lengths) > 2 * PASS


@pytest.mark.parametrize("i", range(N_CASES))
def test_equals_the_mirror_and_keeps_its_promises(cuda, i):
    from voice100_amd.decode import ctc_greedy_decode
    name, x, lengths, kw = cases()[i]
    B, T, V = x.shape
    got = run(x, lengths, kw, cuda)
    again = run(x, lengths, kw, cuda)
    s, e, f, n = (t.cpu().numpy() for t in got)
    rs, re, rf, rn = expected(i)
    assert s.dtype == e.dtype == f.dtype == n.dtype == np.int32
    assert np.array_equal(n, rn), (name, n, rn)
    assert s.shape == rs.shape and np.array_equal(s, rs) and np.array_equal(e, re) and np.array_equal(f, rf), name
    for a, b in zip(got, again):
        assert torch.equal(a, b), name
    blank, margin = kw.get("blank", 0), kw.get("margin", 0.0)
    xd = torch.from_numpy(x).to(cuda)
    for b in range(B):
        nn = T if lengths is None else int(min(max(int(lengths[b]), 0), T))
        k = int(n[b])
        assert not s[b, k:].any() and not e[b, k:].any() and not f[b, k:].any(), name
        R.check(x[b], nn, s[b, :k], e[b, :k], f[b, :k], **kw)
        if nn == 0 or f[b, :k].any() or margin < 0:
            continue
        if nn <= 12000:
            whole, whole_len = ctc_greedy_decode(xd[b:b + 1, :nn].clone(), blank=blank)   # (a clone: kernels take aligned storage)
            whole = whole[0, :int(whole_len[0])].cpu()
        else:                                             # ctc_greedy_decode stops at 12000 frames: its rule in stock ops (no ties here)
            best = torch.unique_consecutive(xd[b, :nn].argmax(-1))
            whole = best[best != blank].cpu()
        if k == 0:
            assert whole.numel() == 0, name
            continue
        st, en = got.start[b, :k].long(), got.end[b, :k].long()
        width = int((en - st).max())
        idx = (st[:, None] + torch.arange(width, device=cuda)[None]).clamp_max(nn - 1)
        ids, ids_len = ctc_greedy_decode(xd[b][idx], (en - st).int(), blank=blank)
        keep = torch.arange(ids.shape[1], device=cuda)[None] < ids_len[:, None]
        assert torch.equal(ids[keep].cpu(), whole), name


def test_forced_and_unforced_rows_are_both_covered():
    """The list must exercise both ends of the rule: rows whose greedy decode is compared, and rows with forced cuts."""
    forced = [int(expected(i)[2].sum()) for i in range(N_CASES)]
    assert sum(1 for v in forced if v == 0) >= 15 and sum(1 for v in forced if v > 0) >= 15
    assert max(int(expected(i)[3].max()) for i in range(N_CASES)) > 2000
