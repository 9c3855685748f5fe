"""The grouped 1x1 weight-gradient launch on 128 x 128 tiles (v100_pw_wgrad_group_small) against the per-problem entry point it
replaces and against float64, as tests/test_gpu_wgrad_group.py does for the 256 x 128 launch:

  * every dW must equal v100_pw_wgrad_io on the same inputs BIT FOR BIT;
  * and stay within the bar tests/test_gpu_io_oracle.py applies to that entry point against float64;
  * outputs are NaN-filled first, so a tile no workgroup wrote shows.

Then the stack executor with both tiers of deferral forced at a small shape: the wide blocks' gradients flush grouped, the narrow
blocks' then wait in the regions that flush left dead and go in ONE small-tile launch."""
import ctypes

import pytest
import torch

from test_gpu_io_oracle import close
from test_gpu_wgrad_group import EXPAND, IO, PROJECT, WGRAD_TOL, _native, _run_stack

pytestmark = pytest.mark.gpu

_cache = {}


def _problem(cuda, mode, B, M, K, T, S=None):
    """test_gpu_wgrad_group._problem with this launch's eligibility test (its own asserts whole 256 x 128 tiles): inputs, the
    per-problem result and the float64 reference, computed once, shared by every list and left unchanged"""
    from test_gpu_io_oracle import affine_relu6, bf, store16
    key = (mode, B, M, K, T, S)
    if key in _cache:
        return _cache[key]
    N = _native()
    g = torch.Generator().manual_seed(M * 3 + T + 7 * K + B + mode)
    rnd = lambda *s: torch.randn(*s, generator=g).to(cuda)
    g16, gs = store16(rnd(B, M, T))
    x16, xs = store16(rnd(B, K, T))
    xa, xb = (torch.rand(K, generator=g).to(cuda) + 0.5, rnd(K)) if mode == PROJECT else (None, None)
    if S is None:
        S = N.helper("v100_pw_wgrad_splits", B, M, K)
    assert N.helper("v100_pw_wgrad_group_small_supported", B, M, K, T, S, 0, mode, IO) == 1
    assert N.helper("v100_pw_wgrad_group_small_tiles", M, K, mode) == (M // 128) * (K // 128)
    partial = torch.empty(S, M, K, device=cuda)
    want = torch.full((M, K), float("nan"), device=cuda)
    N.call("v100_pw_wgrad_io", g16, None, None, None, None, 0, x16, xa, xb, mode, partial, want, S, B, M, K, T, IO)
    xop = bf(affine_relu6(xs, xa, xb).float()).double() if mode == PROJECT else xs
    ref = torch.einsum("bmt,bkt->mk", gs, xop)
    ent = _cache[key] = dict(G=g16, X=x16, xa=xa, xb=xb, dims=(B, M, K, T, S, 0, mode, IO), want=want, ref=ref)
    return ent


def _run_small(cuda, probs):
    N = _native()
    outs = [torch.full_like(p["want"], float("nan")) for p in probs]
    ptr = lambda t: None if t is None else t.data_ptr()
    ptrs = (ctypes.c_void_p * (5 * len(probs)))(*[v for p, o in zip(probs, outs) for v in (ptr(p["G"]), ptr(p["X"]), ptr(p["xa"]), ptr(p["xb"]), ptr(o))])
    dims = (ctypes.c_int * (8 * len(probs)))(*[v for p in probs for v in p["dims"]])
    N.call("v100_pw_wgrad_group_small", len(probs), ptrs, dims)
    return outs


# (mode, B, M, K, T, S).  The tile is 128 x 128 in both modes: (M, K) in {(128, 128), (256, 128), (128, 256), (256, 256)} = one, two
# (either way) and four tiles; B in {1, 3, 5}; T = 8 (one step, a tail), 64 (one whole step), 72 / 200 (steps + a tail).
# S, the reference's split count: S = B, S = 1 (no fold before the end), S that does not divide B (5 = 3 + 2, 3 = 2 + 1, 5 over
# 4 = 2 + 2 + 1 + 0), and None: the library's own, S = B * TS at these few tiles (every utterance's steps cut in TS chunks, empty
# ones where TS exceeds the steps); (PROJECT, 3, 128, 256, 200, 6) names S = B * TS outright.
P = [(PROJECT, 1, 128, 128, 8, 1), (PROJECT, 3, 256, 256, 64, 2), (PROJECT, 5, 256, 128, 72, 4), (PROJECT, 3, 128, 256, 200, None),
     (EXPAND, 1, 128, 128, 8, None), (EXPAND, 3, 256, 256, 64, 3), (EXPAND, 5, 128, 256, 72, 2), (EXPAND, 3, 256, 128, 200, 1),
     (PROJECT, 5, 128, 256, 64, 5), (EXPAND, 5, 256, 128, 64, 3), (PROJECT, 5, 256, 256, 200, None), (EXPAND, 3, 128, 128, 72, None),
     (PROJECT, 3, 128, 256, 200, 6), (EXPAND, 3, 256, 256, 72, 3)]
LISTS = [[P[0]], [P[4]], [P[2]], [P[6]], [P[8]], [P[9]], [P[10]], [P[11]], [P[12]], [P[13]],   # one problem: with and without a tail
         [P[1], P[5]], [P[3], P[7]], [P[8], P[9]],                                         # two: the modes mixed; [8, 9]: no tail anywhere
         [P[0], P[5], P[2], P[7], P[9]], [P[4], P[1], P[6], P[3], P[10]]]                  # five: modes, B, T, S and tile counts mixed


@pytest.mark.parametrize("idx", range(len(LISTS)))
def test_small_group_equals_per_problem_and_float64(cuda, idx):
    probs = [_problem(cuda, *p) for p in LISTS[idx]]
    for p, got, spec in zip(probs, _run_small(cuda, probs), LISTS[idx]):
        assert torch.equal(got, p["want"]), spec
        close(got, p["ref"], f"small grouped wgrad {spec}", tol=WGRAD_TOL)


def test_full_list_of_mixed_tile_counts_fills_every_xcd(cuda):
    """WG_GROUP_MAX = 16 problems, B = 3: 128 x 128 and 256 x 128 (one and two tiles) in both modes, alternating, S = the library's
    own, B, 2 and 1.  24 tiles: three slots on every XCD.  T = 72 (the tail kernel), then T = 64 (the kernel without the masks)."""
    for T in (72, 64):
        specs = [(mode, 3, M, 128, T, S) for S in (None, 3, 2, 1) for M in (128, 256) for mode in (PROJECT, EXPAND)]
        assert len(specs) == 16
        probs = [_problem(cuda, *p) for p in specs]
        for p, got, spec in zip(probs, _run_small(cuda, probs), specs):
            assert torch.equal(got, p["want"]), spec


def test_ineligible_problems_are_refused(cuda):
    N = _native()
    ok = lambda *a: N.helper("v100_pw_wgrad_group_small_supported", *a)
    assert ok(3, 128, 128, 72, 3, 0, PROJECT, IO) == 1
    assert ok(3, 128, 128, 72, 6, 0, EXPAND, IO) == 1         # S = 2 B: every utterance's steps in two chunks
    assert ok(3, 128, 128, 72, 4, 0, PROJECT, IO) == 0        # S > B that is no multiple of B: no such reference
    assert ok(3, 192, 128, 72, 3, 0, PROJECT, IO) == 0        # not whole 128 x 128 tiles
    assert ok(3, 128, 64, 72, 3, 0, EXPAND, IO) == 0
    assert ok(3, 256, 256, 72, 3, 2, EXPAND, 7) == 0          # a transformed G
    assert ok(3, 256, 256, 72, 3, 0, EXPAND, 1) == 0          # fp32-stored X
    assert N.helper("v100_pw_wgrad_group_small_tiles", 192, 128, PROJECT) == 0
    p = dict(_problem(cuda, PROJECT, 3, 256, 256, 64, 2))
    p["dims"] = (3, 256, 256, 64, 4, 0, PROJECT, IO)
    with pytest.raises(RuntimeError):
        _run_small(cuda, [p])


@pytest.mark.parametrize("level", [4, 5])
def test_stack_with_both_tiers_is_bit_identical(cuda, level):
    """Two wide blocks above three narrow ones, B = 3, T = 72, tier-1 thresholds (16, 64), tier-2 threshold 1: blocks 4 and 3 defer
    and flush grouped behind block 3 (128 tiles); blocks 2 and 1 then park da3 / da1 in the two freed regions and flush in ONE
    small-tile launch behind block 1 (block 0 reads the fp32 input and stays): four split-K launches and their four reductions
    become one launch.  With the tier-2 threshold above the 80 pending workgroups the same problems go through the per-problem
    launches.  Level 4 against the per-block path, level 5 against the same stack call with both tiers off."""
    from voice100_amd import functional as F_
    from voice100_amd.layers import InvertedResidual
    N = _native()
    F_.set_matmul_precision("bf16")
    keep = F_.get_activation_storage()
    F_.set_activation_storage(level)
    try:
        torch.manual_seed(5)
        cfgs = ((256, 1024, 256, 35, True), (256, 1024, 256, 5, True), (256, 1024, 512, 5, False), (512, 2048, 512, 5, True),
                (512, 2048, 512, 5, True))
        net = torch.nn.Sequential(*[InvertedResidual(a, b, kernel_size=k, use_residual=r) for a, h, b, k, r in cfgs]).to(cuda)
        g = torch.Generator().manual_seed(72)
        x = torch.randn(3, 256, 72, generator=g).to(cuda)
        gy = torch.randn(3, 512, 72, generator=g).to(cuda)
        desc = (ctypes.c_int * (6 + 30))(5, 3, 72, 1, level, 0, *[v for a, h, b, k, r in cfgs for v in (a, h, b, k, 1, int(r))])
        out = (ctypes.c_longlong * 17)()
        assert N.helper("v100_ir_stack_wgrad_plan", desc, 0, 16, 64, out) == 0
        assert [out[3 * i] for i in range(5)] == [0, 0, 0, 1, 1] and [out[3 * i + 2] for i in range(5)] == [0, 0, 0, 128, 0]
        wide = [out[3 * i + 1] for i in (3, 4)]
        assert N.helper("v100_ir_stack_wgrad_plan2", desc, 0, 16, 64, 1, out) == 0
        assert [out[3 * i] for i in range(5)] == [0, 1, 1, 0, 0] and [out[3 * i + 2] for i in range(5)] == [0, 80, 0, 0, 0]
        assert all(out[3 * i + 1] >= min(wide) for i in (1, 2))
        assert N.helper("v100_ir_stack_wgrad_plan2", desc, 0, 16, 64, 81, out) == 0
        assert [out[3 * i + 2] for i in range(5)] == [0, -80, 0, 0, 0]
        if level == 4:
            ref = _run_stack(net, x, gy, "blocks")
        try:
            F_.set_wgrad_group2_threshold(0)
            if level == 5:
                F_.set_wgrad_group_thresholds(10 ** 6, 10 ** 6)      # both tiers off
                ref = _run_stack(net, x, gy, "stack")
            F_.set_wgrad_group_thresholds(16, 64)
            l0 = N.launch_count()
            tier1 = _run_stack(net, x, gy, "stack")                  # tier 2 off
            base = N.launch_count() - l0
            F_.set_wgrad_group2_threshold(1)
            l0 = N.launch_count()
            got = _run_stack(net, x, gy, "stack")
            assert N.launch_count() - l0 == base - (4 * 2 - 1)
            F_.set_wgrad_group2_threshold(81)
            l0 = N.launch_count()
            late = _run_stack(net, x, gy, "stack")
            assert N.launch_count() - l0 == base
        finally:
            F_.set_wgrad_group_thresholds()
            F_.set_wgrad_group2_threshold()
        for a in (tier1, got, late):
            assert torch.equal(a[0], ref[0])
            for k in ref[1]:
                assert torch.equal(a[1][k], ref[1][k]), k
    finally:
        F_.set_wgrad_group_thresholds()
        F_.set_wgrad_group2_threshold()
        F_.set_activation_storage(keep)
        F_.set_matmul_precision("fp32")
