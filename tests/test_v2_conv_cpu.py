"""Host-only helpers behind the v2 conv path (K1 taps, K11): the route and regime facts tests/test_gpu_v2_conv_oracle.py relies on --
which shapes the tap-addressed GEMMs accept, how the weight gradient is split, how many LayerNorm slabs a backward writes.
Needs the built library, no GPU."""
import os

import pytest

# (B, M, cx, ntap, T, Tx) of every tap-addressed GEMM of tts_en_base at the recipe's step (B = 128, L = 400: Conv1d 1024 -> 512 k5,
# the two ConvTranspose1d phases, Conv1d 512 -> 512 k5 at T = 799) and of asr_en_base v2's stride-1 block (B = 32, T = 512);
# forward and, with M and cx swapped, backward-data.  Tx as functional.py allocates it.
MODEL_TAP_GEMMS = [(128, 512, 1024, 5, 400, 404), (128, 1024, 512, 5, 400, 404),
                   (128, 512, 512, 3, 400, 404), (128, 512, 512, 2, 400, 404),
                   (128, 512, 512, 5, 799, 804), (32, 512, 512, 5, 512, 516)]


def _lib():
    from voice100_amd import _native as N
    import __graft_entry__
    if not os.path.exists(N.LIB_PATH):
        __graft_entry__.build()
    N.load()
    return N


def splits_rule(B, M, K):
    """v100_pw_wgrad_splits restated: enough (128 x 128 tile, split) workgroups for 512, capped by the batch; when even one split per
    utterance leaves the chip idle, every utterance's t range is cut into TS = 2, 4 or 8 chunks as well -> (S, TS), TS = 0 for S <= B"""
    tiles = -(-M // 128) * -(-K // 128)
    S = -(-512 // tiles)
    if S <= B:
        return max(S, 1), 0
    TS = 1
    while TS < 8 and tiles * B * TS * 2 <= 256:
        TS *= 2
    return B * TS, TS


def test_taps_supported_at_model_shapes_and_refusals():
    N = _lib()
    ok = lambda *a: N.helper("v100_pw_taps_supported", *a)
    for B, M, cx, ntap, T, Tx in MODEL_TAP_GEMMS:
        for prec in (0, 1, 2):
            assert ok(B, M, cx, ntap, T, Tx, prec) == 1, (B, M, cx, ntap, T, Tx, prec)
    for cx in (24, 96, 100, 32):                      # 16-bit operands: a k-tile of 64 must not straddle two taps
        assert ok(2, 64, cx, 5, 100, 104, 0) == 1
        assert ok(2, 64, cx, 5, 100, 104, 1) == 0 and ok(2, 64, cx, 5, 100, 104, 2) == 0
    for prec in (0, 1, 2):
        assert ok(2, 64, 64, 0, 100, 104, prec) == 0 and ok(2, 64, 64, 9, 100, 104, prec) == 0      # 1 <= ntap <= 8
        assert ok(2, 64, 64, 8, 100, 108, prec) == 1
        assert ok(2, 64, 64, 5, 100, 99, prec) == 0                                                   # Tx < T
        assert ok(0, 64, 64, 5, 100, 104, prec) == 0 and ok(2, 0, 64, 5, 100, 104, prec) == 0 and ok(2, 64, 64, 5, 0, 104, prec) == 0


def test_wgrad_splits_follow_the_rule():
    N = _lib()
    from test_gpu_v2_conv_oracle import TAP_SHAPES, MODEL_LAYERS
    S = lambda B, M, K: N.helper("v100_pw_wgrad_splits", B, M, K)
    for B, M, cx, ntap, T, Tx in MODEL_TAP_GEMMS:
        s, ts = splits_rule(B, M, ntap * cx)
        assert S(B, M, ntap * cx) == s and ts == 0 and s <= B, (B, M, cx, ntap)     # the models' layers: batch-split regime
    for name, B, M, cx, T, shifts, lpad in MODEL_LAYERS:
        assert (B, M, cx, len(shifts), T, (T + max(shifts) + 3) // 4 * 4) in MODEL_TAP_GEMMS, name
    seen = set()
    for B, M, cx, T, shifts, lpad, extra, ts in TAP_SHAPES:
        K = len(shifts) * cx
        assert (S(B, M, K), ts) == splits_rule(B, M, K), (B, M, cx, T)
        assert ts == 0 or T % (ts * 64) != 0
        seen.add(ts)
    assert seen == {0, 2, 4, 8}                        # both regimes, every chunk count
    for B in (1, 2, 3, 5, 16, 32, 128):
        for M in (1, 29, 64, 128, 129, 300, 512, 1024):
            for K in (8, 64, 128, 192, 320, 1024, 2560, 5120):
                s, ts = splits_rule(B, M, K)
                assert S(B, M, K) == s and s >= 1 and (s <= B or (s % B == 0 and s // B in (1, 2, 4, 8))), (B, M, K)


def test_ln_num_parts():
    N = _lib()
    for B, T in [(1, 1), (1, 32), (1, 33), (2, 31), (3, 64), (128, 799), (32, 512), (7, 65)]:
        assert N.helper("v100_ln_num_parts", B, T) == B * ((T + 31) // 32), (B, T)
