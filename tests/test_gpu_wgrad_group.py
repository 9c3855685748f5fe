"""The grouped 1x1 weight-gradient launch (v100_pw_wgrad_group: several problems, one tile per workgroup through the whole
contraction, no split-K slabs) against the per-problem entry point it replaces and against float64.

  * every dW must equal v100_pw_wgrad_io on the same inputs BIT FOR BIT: the workgroup walks the contraction in the order of the
    reference's splits and sums their partial tiles in slab order;
  * and stay within the bar tests/test_gpu_io_oracle.py applies to that entry point against float64 (its `close`, with the
    tolerance test_pw_wgrad_io_vs_float64 passes to it);
  * outputs are NaN-filled first, so a tile no workgroup wrote shows.

Then the stack executor with deferral forced at a small shape (the thresholds are arguments of the planner and a process-wide
setting of the executor) against the per-block path and against itself without deferral."""
import copy
import ctypes

import pytest
import torch

from test_gpu_io_oracle import affine_relu6, bf, close, store16

pytestmark = pytest.mark.gpu

WGRAD_TOL = 3e-4                    # what test_pw_wgrad_io_vs_float64 passes to close() for both gradients
PROJECT, EXPAND = 1, 0              # x_mode: relu6(xa x + xb) on load, 256 x 128 tile | plain X (the finished gradient da1), 128 x 256 tile
IO = 1 | 4                          # WG_IO_G | WG_IO_X


def _native():
    from voice100_amd import _native as N
    N.load()
    return N


_cache = {}


def _problem(cuda, mode, B, M, K, T, S=None):
    """inputs, the per-problem result and the float64 reference of one problem (S: the reference's split count, None = the
    library's own choice): computed once, shared by every list it appears in and left unchanged"""
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
    assert N.helper("v100_pw_wgrad_group_supported", B, M, K, T, S, 0, mode, IO) == 1
    partial = torch.empty(S, M, K, device=cuda)
    want = torch.full((M, K), float("nan"), device=cuda)
    N.call("v100_pw_wgrad_io", g16, None, None, None, None, 0, x16, xa, xb, mode, partial, want, S, B, M, K, T, IO)
    xop = bf(affine_relu6(xs, xa, xb).float()).double() if mode == PROJECT else xs
    ref = torch.einsum("bmt,bkt->mk", gs, xop)
    ent = _cache[key] = dict(G=g16, X=x16, xa=xa, xb=xb, dims=(B, M, K, T, S, 0, mode, IO), want=want, ref=ref)
    return ent


def _run_group(cuda, probs):
    N = _native()
    outs = [torch.full_like(p["want"], float("nan")) for p in probs]
    ptr = lambda t: None if t is None else t.data_ptr()
    ptrs = (ctypes.c_void_p * (5 * len(probs)))(*[v for p, o in zip(probs, outs) for v in (ptr(p["G"]), ptr(p["X"]), ptr(p["xa"]), ptr(p["xb"]), ptr(o))])
    dims = (ctypes.c_int * (8 * len(probs)))(*[v for p in probs for v in p["dims"]])
    N.call("v100_pw_wgrad_group", len(probs), ptrs, dims)
    return outs


# (mode, B, M, K, T, S).  M, K in {(256, 128), (256, 256), (128, 256), (512, 256)} as the mode's tile allows (project 256 x 128,
# expand 128 x 256: one, two and four tiles); B in {1, 3, 5}; T = 8 (one step, a tail), 64 (one whole step), 72 / 200 (steps + tail).
# S, the reference's split count: S = B (an utterance a split), S = 1 (no fold before the end), S that does not divide B -- ceil(B / S)
# utterances a split, the last short (5 = 3 + 2, 3 = 2 + 1) or empty (5 over 4 = 2 + 2 + 1 + 0) -- and None: what
# v100_pw_wgrad_splits gives at these few tiles, S = B * TS with every utterance's steps cut in TS chunks (empty ones where
# TS exceeds the steps).
P = [(PROJECT, 1, 256, 128, 8, 1), (PROJECT, 3, 256, 256, 64, 2), (PROJECT, 5, 512, 256, 72, 4), (PROJECT, 3, 256, 128, 200, None),
     (EXPAND, 1, 128, 256, 8, None), (EXPAND, 3, 256, 256, 64, 3), (EXPAND, 5, 512, 256, 72, 2), (EXPAND, 3, 128, 256, 200, 1),
     (PROJECT, 5, 256, 256, 64, 5), (EXPAND, 5, 128, 256, 64, 3), (PROJECT, 5, 256, 128, 200, None), (EXPAND, 3, 256, 256, 72, None)]
LISTS = [[P[0]], [P[4]], [P[2]], [P[6]], [P[8]], [P[9]], [P[10]], [P[11]],                 # one problem: with and without a tail
         [P[1], P[5]], [P[3], P[7]], [P[8], P[9]],                                         # two: the modes mixed; [8, 9]: no tail anywhere
         [P[0], P[5], P[2], P[7], P[9]], [P[4], P[1], P[6], P[3], P[10]]]                  # five: modes, B, T, S and tile counts mixed


@pytest.mark.parametrize("idx", range(len(LISTS)))
def test_group_equals_per_problem_and_float64(cuda, idx):
    probs = [_problem(cuda, *p) for p in LISTS[idx]]
    for p, got, spec in zip(probs, _run_group(cuda, probs), LISTS[idx]):
        assert torch.equal(got, p["want"]), spec
        close(got, p["ref"], f"grouped wgrad {spec}", tol=WGRAD_TOL)


def test_full_list_of_mixed_tile_counts_fills_every_xcd(cuda):
    """WG_GROUP_MAX = 16 problems, B = 3: eight project gradients of 256 x 128 and 512 x 128 (one and two tiles), eight expand
    gradients of 128 x 256 and 128 x 512, the modes alternating, S = the library's own, B, 2 and 1.  24 tiles: three slots on every
    XCD, so a problem's slot0 is past 0 on each.  T = 72 (the tail kernel), then T = 64 (the kernel without the masks)."""
    for T in (72, 64):
        specs = [(mode, 3, M, K, T, S) for S in (None, 3, 2, 1) for M2 in (1, 2)
                 for mode, M, K in ((PROJECT, 256 * M2, 128), (EXPAND, 128, 256 * M2))]
        assert len(specs) == 16
        probs = [_problem(cuda, *p) for p in specs]
        for p, got, spec in zip(probs, _run_group(cuda, probs), specs):
            assert torch.equal(got, p["want"]), spec


def test_ineligible_problems_are_refused(cuda):
    N = _native()
    ok = lambda *a: N.helper("v100_pw_wgrad_group_supported", *a)
    assert ok(3, 256, 128, 72, 3, 0, PROJECT, IO) == 1
    assert ok(3, 256, 128, 72, 6, 0, PROJECT, IO) == 1        # S = 2 B: every utterance's steps in two chunks
    assert ok(3, 256, 128, 72, 4, 0, PROJECT, IO) == 0        # S > B that is no multiple of B: no such reference
    assert ok(3, 128, 256, 72, 3, 0, PROJECT, IO) == 0        # not whole 256 x 128 tiles
    assert ok(3, 256, 128, 72, 3, 0, EXPAND, IO) == 0         # not whole 128 x 256 tiles
    assert ok(3, 256, 256, 72, 3, 2, EXPAND, 7) == 0          # a transformed G
    assert ok(3, 256, 256, 72, 3, 0, EXPAND, 1) == 0          # fp32-stored X
    p = dict(_problem(cuda, PROJECT, 3, 256, 256, 64, 2))
    p["dims"] = (3, 256, 256, 64, 4, 0, PROJECT, IO)
    with pytest.raises(RuntimeError):
        _run_group(cuda, [p])


def _run_stack(net, x, gy, how):
    from voice100_amd import functional as F_
    net = copy.deepcopy(net).train()
    x = x.clone().requires_grad_(True)
    y = net(x) if how == "blocks" else F_.ir_stack_train(list(net), x)
    (y * gy).sum().backward()
    return x.grad, {k: p.grad for k, p in net.named_parameters()}


@pytest.mark.parametrize("level,min_flush", [(4, 32), (5, 32), (4, 64)])
def test_stack_with_deferred_gradients_is_bit_identical(cuda, level, min_flush):
    """256 -> 256 blocks (hidden 1024: 8 + 8 tiles) around two that cannot defer (256 -> 64 and 64 -> 256: no whole tiles), B = 3,
    T = 72, thresholds (1, 32): blocks 4 and 1 defer, their 32 tiles wait across the two others and go in ONE grouped launch of
    four problems behind block 1; block 0 reads the fp32 input and stays as it is.  Thresholds (1, 64): the same deferral, but the
    32 tiles are too few and go through the per-problem launches where the walk ends.  Level 4 against the per-block path; level 5
    (16-bit gradient stream inside a stack call: not the per-block arithmetic) against the same stack call without deferral."""
    from voice100_amd import functional as F_
    from voice100_amd.layers import InvertedResidual
    N = _native()
    F_.set_matmul_precision("bf16")
    keep = F_.get_activation_storage()
    F_.set_activation_storage(level)
    try:
        torch.manual_seed(5)
        cfgs = ((256, 256, 35, True), (256, 256, 5, True), (256, 64, 5, False), (64, 256, 5, False), (256, 256, 5, True))
        net = torch.nn.Sequential(*[InvertedResidual(a, b, kernel_size=k, use_residual=r) for a, b, k, r in cfgs]).to(cuda)
        g = torch.Generator().manual_seed(72)
        x = torch.randn(3, 256, 72, generator=g).to(cuda)
        gy = torch.randn(3, 256, 72, generator=g).to(cuda)
        ref = _run_stack(net, x, gy, "blocks" if level == 4 else "stack")
        desc = (ctypes.c_int * (6 + 30))(5, 3, 72, 1, level, 0, *[v for a, b, k, r in cfgs for v in (a, 4 * a, b, k, 1, int(r))])
        out = (ctypes.c_longlong * 17)()
        assert N.helper("v100_ir_stack_wgrad_plan", desc, 0, 1, min_flush, out) == 0
        assert [out[3 * i] for i in range(5)] == [0, 1, 0, 0, 1]
        assert [out[3 * i + 2] for i in range(5)] == ([0, 32, 0, 0, 0] if min_flush == 32 else [-32, 0, 0, 0, 0])
        F_.set_wgrad_group_thresholds(1, min_flush)
        try:
            l0 = N.launch_count()
            got = _run_stack(net, x, gy, "stack")
            launches = N.launch_count() - l0
        finally:
            F_.set_wgrad_group_thresholds()
        l0 = N.launch_count()
        again = _run_stack(net, x, gy, "stack")
        # grouped: four split-K launches and their four reductions became one launch; per problem: the same launches, later
        assert N.launch_count() - l0 == launches + (7 if min_flush == 32 else 0)
        for a, b in ((got, ref), (again, ref)):
            assert torch.equal(a[0], b[0])
            for k in b[1]:
                assert torch.equal(a[1][k], b[1][k]), k
    finally:
        F_.set_wgrad_group_thresholds()
        F_.set_activation_storage(keep)
        F_.set_matmul_precision("fp32")
