"""v100_ir_stack_wgrad_plan2 (host arithmetic only, no GPU): which blocks of a stack park the operands of their two 1x1 weight
gradients in the regions a tier-1 flush has left dead, where the backward walk flushes them in one small-tile launch, and that
none of it costs a byte."""
import ctypes
import os

import pytest

from test_wgrad_group_plan_cpu import ENCODER, _desc, _plan


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


def _plan2(lib, cfgs, B, T, have_x16=1, min_problem=32, min_flush=192, min_small=96, **kw):
    n = len(cfgs)
    out = (ctypes.c_longlong * (3 * n + 2))()
    assert lib.v100_ir_stack_wgrad_plan2(_desc(cfgs, B, T, **kw), have_x16, min_problem, min_flush, min_small, out) == 0
    return [tuple(out[3 * i:3 * i + 3]) for i in range(n)], out[3 * n], out[3 * n + 1]


def test_bench_descriptor_parks_the_narrow_blocks_in_the_wide_blocks_regions(lib):
    tier1, total1, shared1, _ = _plan(lib, ENCODER, 32, 1024)
    blocks, total, shared = _plan2(lib, ENCODER, 32, 1024)
    assert [b[0] for b in blocks] == [0, 1, 1, 1, 1, 0, 0, 0, 0]
    # the walk runs 8 .. 0: the opener cannot join, so the one flush falls behind block 1: 3 x (16 + 16) + 32 + 16 workgroups
    assert [b[2] for b in blocks] == [0, 144, 0, 0, 0, 0, 0, 0, 0]
    assert (total, shared) == (total1, shared1)
    # borrowed regions: 256-aligned, disjoint, each inside ONE region of blocks 5-8 (da3 + da1 of the block, bf16, T = 512)
    wide = [(b[1], b[1] + 32 * 512 * 512 * 2 + 32 * 2048 * 512 * 2) for b in tier1 if b[0]]
    assert len(wide) == 4 and all(hi <= total for _, hi in wide)
    size = {i: 32 * ENCODER[i][2] * 512 * 2 + 32 * ENCODER[i][1] * 512 * 2 for i in (1, 2, 3, 4)}
    spans = sorted((blocks[i][1], blocks[i][1] + size[i]) for i in size)
    assert all(b[1] == -1 for b in blocks if not b[0])
    for lo, hi in spans:
        assert lo % 256 == 0 and any(wlo <= lo and hi <= whi for wlo, whi in wide)
    for (_, hi), (lo, _) in zip(spans, spans[1:]):
        assert hi <= lo


def test_threshold_above_the_pending_workgroups_flushes_per_problem(lib):
    blocks, _, _ = _plan2(lib, ENCODER, 32, 1024, min_small=145)
    assert [b[0] for b in blocks] == [0, 1, 1, 1, 1, 0, 0, 0, 0] and [b[2] for b in blocks] == [0, -144, 0, 0, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("cfgs,B,T,bf16,level,min_small", [(ENCODER[:5], 32, 1024, 1, 5, 96), (ENCODER, 32, 1024, 0, 0, 96),
                                                           (ENCODER, 32, 1024, 1, 3, 96), (ENCODER, 32, 2272, 1, 5, 96),
                                                           (ENCODER, 48, 1024, 1, 5, 96), (ENCODER, 32, 1024, 1, 5, 0)])
def test_no_flushed_region_or_threshold_zero_defers_nothing(lib, cfgs, B, T, bf16, level, min_small):
    """narrow blocks only, fp32, storage below level 4, rows past 512 outputs, more utterances than the finished gradient takes:
    no tier-1 flush leaves a region; threshold 0: tier 2 is off.  Nothing defers and the totals are tier 1's."""
    _, total1, shared1, _ = _plan(lib, cfgs, B, T, bf16=bf16, level=level)
    blocks, total, shared = _plan2(lib, cfgs, B, T, min_small=min_small, bf16=bf16, level=level)
    assert not any(b[0] for b in blocks) and not any(b[2] for b in blocks) and all(b[1] == -1 for b in blocks)
    assert (total, shared) == (total1, shared1)
