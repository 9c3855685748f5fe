"""The host side of the two grouped weight-gradient launchers (no GPU): the status codes both table forms return before any
device call, and that the two planner entry points read one plan."""
import ctypes
import os

import pytest

from test_wgrad_group_plan_cpu import ENCODER, _plan
from test_wgrad_group2_plan_cpu import _plan2

FIVE = ((256, 1024, 256, 35, 1, 1), (256, 1024, 256, 5, 1, 1), (256, 1024, 64, 5, 1, 0), (64, 256, 256, 5, 1, 0), (256, 1024, 256, 5, 1, 1))


@pytest.fixture(scope="module")
def lib():
    from voice100_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return N.load()


@pytest.mark.parametrize("name", ["v100_pw_wgrad_group", "v100_pw_wgrad_group_small"])
def test_table_launchers_refuse_before_any_device_call(lib, name):
    fn = getattr(lib, name)
    good = (3, 256, 256, 72, 3, 0, 1, 1 | 4)                  # a project gradient both tiers take
    tables = lambda ptrs, dims: ((ctypes.c_void_p * len(ptrs))(*ptrs), (ctypes.c_int * len(dims))(*dims))
    ptrs, dims = tables([16] * 5 * 17, good * 17)             # (operands are never dereferenced on the host)
    assert fn(1, None, dims, None) == 3 and fn(1, ptrs, None, None) == 3
    assert fn(0, ptrs, dims, None) == 1 and fn(17, ptrs, dims, None) == 1
    ptrs, dims = tables([16] * 5 + [16, 16, 16, 16, None], good * 2)
    assert fn(2, ptrs, dims, None) == 3                       # dW of the second problem is NULL
    ptrs, dims = tables([16] * 15, good + (3, 192, 256, 72, 3, 0, 1, 1 | 4) + good)
    assert fn(3, ptrs, dims, None) == 1                       # M = 192: whole tiles of neither tier
    ptrs, dims = tables([16] * 5 + [16, 16, 16, 16, None], (3, 192, 256, 72, 3, 0, 1, 1 | 4) + good)
    assert fn(2, ptrs, dims, None) == 1                       # problem by problem: the first one's shape before the second one's NULL


@pytest.mark.parametrize("cfgs,B,T,kw", [(ENCODER, 32, 1024, {}), (FIVE, 3, 72, dict(have_x16=0, min_problem=1, min_flush=32))])
def test_both_planner_entry_points_read_one_plan(lib, cfgs, B, T, kw):
    tier1, total1, shared1, _ = _plan(lib, cfgs, B, T, **kw)
    assert any(b[0] for b in tier1)
    for min_small in (96, 1, 0):
        blocks, total, shared = _plan2(lib, cfgs, B, T, min_small=min_small, **kw)
        assert (total, shared) == (total1, shared1)
        assert not any(b[0] and t[0] for b, t in zip(blocks, tier1))          # a block waits for one tier
        if min_small == 0:
            assert not any(b[0] for b in blocks) and not any(b[2] for b in blocks) and all(b[1] == -1 for b in blocks)
