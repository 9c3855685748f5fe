"""v100_ir_stack_wgrad_plan (host arithmetic only, no GPU): which blocks of a stack leave their two 1x1 weight gradients to a
grouped launch, where the backward walk flushes them, and where their operands live in the backward workspace."""
import ctypes
import os

import pytest

ENCODER = ((64, 256, 256, 11, 2, 0), (256, 1024, 256, 19, 1, 1), (256, 1024, 256, 27, 1, 1), (256, 1024, 256, 35, 1, 1),
           (256, 1024, 512, 51, 1, 0), (512, 2048, 512, 59, 1, 1), (512, 2048, 512, 67, 1, 1), (512, 2048, 512, 75, 1, 1),
           (512, 2048, 512, 83, 1, 0))
WIDE = (512, 2048, 512, 59, 1, 1)


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


def _desc(cfgs, B, T, bf16=1, level=5, shadow=0):
    n = len(cfgs)
    return (ctypes.c_int * (6 + 6 * n))(n, B, T, bf16, level, shadow, *[v for c in cfgs for v in c])


def _plan(lib, cfgs, B, T, have_x16=1, min_problem=32, min_flush=192, **kw):
    n = len(cfgs)
    desc = _desc(cfgs, B, T, **kw)
    out = (ctypes.c_longlong * (3 * n + 2))()
    assert lib.v100_ir_stack_wgrad_plan(desc, have_x16, min_problem, min_flush, out) == 0
    stack = (ctypes.c_longlong * (8 * n + 6))()
    assert lib.v100_ir_stack_plan(desc, stack) >= 0
    blocks = [tuple(out[3 * i:3 * i + 3]) for i in range(n)]
    return blocks, out[3 * n], out[3 * n + 1], stack[8 * n + 1]


def _parent_bwd_ws(lib, cfgs, B, T, bf16, level):
    """bwd_ws_bytes as planned before there were per-block regions: the largest per-block workspace + two gradient buffers"""
    al = lambda v: (v + 255) & ~255
    ws = dx = 0
    for cin, hid, cout, k, s, res in cfgs:
        sh = [B, cin, hid, cout, T, k, s, res, bf16, 1 | (2 if bf16 == 1 and level >= 4 else 0), 0]
        if bf16 == 1 and level and lib.v100_ir_act16_supported((ctypes.c_int * 11)(*sh)):
            sh[10] = level
        ws = max(ws, lib.v100_ir_bwd_workspace_bytes((ctypes.c_int * 11)(*sh)))
        dx = max(dx, B * cin * T * 4)
        T = (T + 2 * ((k - 1) // 2) - k) // s + 1
    return al(ws) + 2 * al(dx) + 256


def test_bench_descriptor_defers_the_wide_blocks_and_flushes_once(lib):
    blocks, total, shared, planned = _plan(lib, ENCODER, 32, 1024)
    assert [b[0] for b in blocks] == [0, 0, 0, 0, 0, 1, 1, 1, 1]
    # the walk runs 8 .. 0: the one flush falls behind block 5 with all 8 x 32 tiles, one per CU
    assert [b[2] for b in blocks] == [0, 0, 0, 0, 0, 256, 0, 0, 0]
    assert total == planned                                   # what functional.py allocates (v100_ir_stack_plan) is this plan's size
    assert shared == _parent_bwd_ws(lib, ENCODER, 32, 1024, 1, 5)
    # regions: behind the shared part, disjoint, inside the workspace, each da3 + da1 of its block (bf16, T = 512 after the opener)
    regs = sorted(b[1] for b in blocks if b[0])
    size = 32 * 512 * 512 * 2 + 32 * 2048 * 512 * 2
    assert all(b[1] == -1 for b in blocks if not b[0]) and regs[0] == shared
    for a, b in zip(regs, regs[1:] + [total]):
        assert a % 256 == 0 and a + size <= b


def test_three_wide_blocks_flush_grouped_two_fall_back(lib):
    blocks, total, shared, _ = _plan(lib, (WIDE,) * 3, 32, 512)
    assert [b[0] for b in blocks] == [1, 1, 1] and [b[2] for b in blocks] == [192, 0, 0]
    blocks, total, shared, _ = _plan(lib, (WIDE,) * 2, 32, 512)
    assert [b[0] for b in blocks] == [1, 1] and [b[2] for b in blocks] == [-128, 0]       # < 0: the per-problem launches
    # without a shadow of the stack's input the first block stays on the per-block path (its expand gradient reads fp32 x)
    blocks, _, _, _ = _plan(lib, (WIDE,) * 3, 32, 512, have_x16=0)
    assert [b[0] for b in blocks] == [0, 1, 1] and [b[2] for b in blocks] == [-128, 0, 0]      # (too few: they wait for the walk's end)
    # five wide blocks: four fill the chip, the fifth waits for the end of the walk
    blocks, _, _, _ = _plan(lib, (WIDE,) * 5, 32, 512)
    assert [b[2] for b in blocks] == [-64, 256, 0, 0, 0]


def test_thresholds_are_arguments(lib):
    cfgs = ((256, 1024, 256, 35, 1, 1), (256, 1024, 256, 5, 1, 1), (256, 1024, 64, 5, 1, 0), (64, 256, 256, 5, 1, 0), (256, 1024, 256, 5, 1, 1))
    blocks, total, shared, planned = _plan(lib, cfgs, 3, 72, have_x16=0, min_problem=1, min_flush=32)
    assert [b[0] for b in blocks] == [0, 1, 0, 0, 1]          # 256 -> 64 and 64 -> 256 have no whole tiles; block 0 has no shadow to read
    assert [b[2] for b in blocks] == [0, 32, 0, 0, 0]         # 16 tiles wait across the two ineligible blocks
    assert planned == shared < total                          # (v100_ir_stack_plan: the process-wide defaults, nothing defers)
    blocks, total, shared, planned = _plan(lib, cfgs, 3, 72)
    assert not any(b[0] for b in blocks) and total == shared == planned


@pytest.mark.parametrize("cfgs,B,T,bf16,level", [(ENCODER, 32, 1024, 0, 0), (ENCODER, 32, 1024, 1, 3), (ENCODER[:5], 32, 1024, 1, 5),
                                                 (ENCODER, 32, 1136 * 2, 1, 5), (ENCODER, 48, 1024, 1, 5)])
def test_no_eligible_block_plans_what_the_parent_plans(lib, cfgs, B, T, bf16, level):
    """fp32, storage below level 4, narrow blocks only, rows past the finished-gradient kernel's 512 outputs, more utterances than
    it takes: nothing defers and the workspace is the parent's to the byte"""
    blocks, total, shared, planned = _plan(lib, cfgs, B, T, bf16=bf16, level=level)
    assert not any(b[0] for b in blocks) and not any(b[2] for b in blocks)
    assert total == shared == planned == _parent_bwd_ws(lib, cfgs, B, T, bf16, level)
