"""The conv half of the v2 models -- the dense k-tap Conv1d and the k5/s2 ConvTranspose1d as tap-addressed GEMMs (K1 taps), their
im2col / col2im and tap-stacked routes, and the fused channel LayerNorm + GELU (K11) -- checked ELEMENTWISE against plain torch in
float64 on the operands as each kernel defines them, at small ragged shapes and at the shapes the models run:

  * bf16 / fp16 mode: A and X (for a backward GEMM: the incoming gradient) are rounded once to that format; fp32 mode rounds nothing;
  * products are exact, accumulation fp32 (reference: float64, computed on the device as tests/test_gpu_io_oracle.py does).

Bars (the project's own): GEMM outputs max |got - ref| <= 2e-4 * max(1, max |ref|), weight gradients 3e-4 (test_gpu_io_oracle.py),
the fp32 path 1e-4 (TOL of test_gpu_kernels.py), bias gradients 2e-6 * B * T (test_chan_passes_io_vs_float64), LayerNorm + GELU the
bars of test_layer_norm_gelu_kernel_edges.  Every element counts.  Run with -s for the worst error over its bar of every comparison."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from test_gpu_io_oracle import bf, close, col      # the helper shapes of the 1x1 oracle file (bf: one bf16 rounding)

pytestmark = pytest.mark.gpu

DT = {0: None, 1: torch.bfloat16, 2: torch.float16}
PREC = {"fp32": 0, "bf16": 1, "fp16": 2}
GEMM_TOL = {0: 1e-4, 1: 2e-4, 2: 2e-4}
WGRAD_TOL = {0: 1e-4, 1: 3e-4}
SENTINEL = 3.0e4            # large and FINITE in every format: a stray G column may meet a zero of the padding, never a sample


def _native():
    from voice100_amd import _native as N
    N.load()
    return N


def rd(t, prec):
    """the operand as the GEMM sees it, as float64: rounded once to bf16 / fp16, or untouched in fp32 mode"""
    if prec == 1:
        return bf(t).double()
    return t.to(DT[prec]).double() if prec else t.double()


def check(got, ref, what, tol):
    """`close` of test_gpu_io_oracle.py (all elements, finite, max |err| <= tol * max(1, max |ref|)) after printing worst / bar"""
    got, ref = got.detach(), ref.detach()
    bound = tol * max(1.0, float(ref.double().abs().max()))
    worst = float((got.double() - ref.double()).abs().max())
    print(f"[v2-conv-oracle] {what}: worst/bar = {worst / bound:.4f} (worst {worst:.3e}, bar {bound:.3e})")
    close(got, ref, what, tol=tol)


def check_abs(got, ref, what, bound):
    worst = float((got.double() - ref.double()).abs().max())
    print(f"[v2-conv-oracle] {what}: worst/bar = {worst / bound:.4f} (worst {worst:.3e}, bar {bound:.3e})")
    assert torch.isfinite(got).all() and worst <= bound, f"{what}: max err {worst:.3e} > {bound:.3e}"


def splits_rule(B, M, K):
    """v100_pw_wgrad_splits restated (csrc/pointwise.hip): -> (S, TS), TS = 0 in the batch-split regime"""
    tiles = -(-M // 128) * -(-K // 128)
    S = -(-512 // tiles)
    if S <= B:
        return max(S, 1), 0
    TS = 1
    while TS < 8 and tiles * B * TS * 2 <= 256:
        TS *= 2
    return B * TS, TS


# ------------------------------------------------------------------------------------------------------------------------------
# a. v100_pad_copy + v100_pw_gemm_taps + v100_pw_wgrad_taps at kernel level
# ------------------------------------------------------------------------------------------------------------------------------
def run_taps(cuda, prec, B, M, cx, T, shifts, lpad=0, extra=0, g_off=1, ts=None, wgrad=True, what=""):
    """One (shape, precision): Xp through v100_pad_copy (checked exactly), the GEMM with its three epilogues (plain, bias, +R) into a
    NaN-filled Y, and (prec < 2, wgrad) the weight gradient with G inside a wider sentinel-filled buffer at an odd offset.
    Tx = T + max shift rounded up to 4 (+ extra): extra = 0 is the smallest legal Tx.  ts: the expected regime of
    v100_pw_wgrad_splits -- 0 for S <= B, else S = B * ts -- asserted from the helper's return value before the comparison."""
    N = _native()
    ntap, K = len(shifts), len(shifts) * cx
    tx = (T + max(shifts) + 3) // 4 * 4 + extra
    assert N.helper("v100_pw_taps_supported", B, M, cx, ntap, T, tx, prec) == 1, what
    g = torch.Generator(device=cuda).manual_seed(M * 7 + cx + 3 * T + ntap)
    rnd = lambda *s: torch.randn(*s, generator=g, device=cuda)
    sh = (ctypes.c_int * ntap)(*shifts)
    # Xp: rows longer than what is copied, copy starts at column 1; 64 floats of NaN slack behind it that nothing stored may depend on
    x = rnd(B, cx, T + 3)
    flat = torch.full((B * cx * tx + 64,), float("nan"), device=cuda)
    xp = flat[:B * cx * tx].view(B, cx, tx)
    N.call("v100_pad_copy", x, xp, B, cx, T + 3, 1, 1, T, tx, lpad)
    ref_xp = torch.zeros(B, cx, tx, device=cuda)
    ref_xp[:, :, lpad:lpad + T] = x[:, :, 1:1 + T]
    assert torch.equal(xp, ref_xp), what + " pad_copy"
    assert bool(torch.isnan(flat[B * cx * tx:]).all()), what + " pad_copy wrote behind Xp"
    A = rnd(M, K) / K ** 0.5
    A16 = A.to(DT[prec]) if prec else None
    Ad, xpd = rd(A, prec), rd(ref_xp, prec)

    def taps(fn):
        return [fn(i, xpd[:, :, s:s + T]) for i, s in enumerate(shifts)]
    ref = sum(taps(lambda i, xs: torch.einsum("mc,bct->bmt", Ad[:, i * cx:(i + 1) * cx], xs)))
    bias, R = rnd(M), rnd(B, M, T) * 2
    for name, b_, r_, want in (("plain", None, None, ref), ("bias", bias, None, ref + col(bias)), ("+R", None, R, ref + R.double())):
        Y = torch.full((B, M, T), float("nan"), device=cuda)
        if prec == 2 and r_ is not None:
            with pytest.raises(RuntimeError):          # fp16 = inference: store (+ bias) only; refused on the host before any launch
                N.call("v100_pw_gemm_taps", A, A16, xp, Y, b_, r_, B, M, cx, T, tx, ntap, sh, prec)
            continue
        N.call("v100_pw_gemm_taps", A, A16, xp, Y, b_, r_, B, M, cx, T, tx, ntap, sh, prec)
        check(Y, want, f"{what} gemm {name}", GEMM_TOL[prec])
    assert bool(torch.isnan(flat[B * cx * tx:]).all())
    if not wgrad or prec == 2:
        return
    G = rnd(B, M, T)
    tg = g_off + T + 4
    assert g_off % 2 == 1 and tg > g_off + T
    Gp = torch.full((B, M, tg), SENTINEL, device=cuda)
    Gp[:, :, g_off:g_off + T] = G
    S = N.helper("v100_pw_wgrad_splits", B, M, K)
    assert (S, ts) == splits_rule(B, M, K), (what, S, ts)
    if ts:
        assert S == B * ts and S > B and T % (ts * 64) != 0, (what, S)      # t-split regime, chunks of uneven length
    else:
        assert 1 <= S <= B, (what, S)
    partial = torch.full((S, M, K), float("nan"), device=cuda)               # workspace: every slab must be written before it is summed
    dW = torch.full((M, K), float("nan"), device=cuda)
    N.call("v100_pw_wgrad_taps", Gp, tg, g_off, xp, partial, dW, S, B, M, cx, T, tx, ntap, sh, prec)
    Gd = rd(G, prec)
    ref_dw = torch.cat(taps(lambda i, xs: torch.einsum("bmt,bct->mc", Gd, xs)), dim=1)
    check(dW, ref_dw, f"{what} wgrad S={S}", WGRAD_TOL[prec])


# (B, M, cx, T, shifts, lpad, extra, ts).  k-tiles = ntap * cx / 64; BM is the bf16 / fp16 kernel's row tile (256 from M >= 256).
TAP_SHAPES = [
    # BM = 128; 2 taps, 2 k-tiles (even), a tap change every k-tile; T % 4 = 1; smallest Tx; t-split TS = 8
    (2, 64, 64, 77, (1, 0), 1, 0, 8),
    # BM = 256 with ONE m-tile; 3 unsorted taps, 3 k-tiles (odd); T % 128 = 1; TS = 8
    (3, 256, 64, 129, (2, 0, 1), 1, 0, 8),
    # BM = 256, partial last m-tile (300 = 256 + 44); 8 taps, odd shifts (16-byte loads at 4-byte alignment); T % 128 = 127; Tx above
    # the minimum; TS = 2
    (3, 300, 128, 127, (5, 0, 3, 1, 7, 2, 6, 4), 4, 4, 2),
    # BM = 256, two full m-tiles; 5 taps, 5 k-tiles (odd); T % 4 = 2; TS = 4
    (5, 512, 64, 130, (0, 1, 2, 3, 4), 2, 0, 4),
    # BM = 256, three m-tiles with a partial last one (640 = 2 * 256 + 128); 7 taps, 7 k-tiles (odd); T % 128 = 1; TS = 4
    (2, 640, 64, 513, (6, 3, 0, 5, 2, 4, 1), 3, 0, 4),
    # T = 1 (BM = 128, M off the tile); TS = 8
    (2, 129, 64, 1, (0, 1, 2), 1, 0, 8),
    # T smaller than the largest shift; TS = 8
    (2, 40, 64, 3, (7, 0, 5), 3, 0, 8),
    # cx = 512: the tap changes every 8 k-tiles, 40 k-tiles (even); M = 256; TS = 2
    (2, 256, 512, 130, (0, 1, 2, 3, 4), 2, 0, 2),
    # cx = 1024: the tap changes every 16 k-tiles, 48 k-tiles; BM = 128; T % 4 = 1; TS = 4
    (2, 128, 1024, 77, (1, 3, 0), 1, 0, 4),
    # cx = 192: 9 k-tiles (odd), a tap change every 3; BM = 128; T % 128 = 127; TS = 8
    (2, 128, 192, 255, (3, 1, 2), 1, 4, 8),
    # batch-split regime S <= B at a small shape (40 tiles -> S = 13 <= 16)
    (16, 256, 512, 100, (4, 2, 0, 1, 3), 2, 4, 0),
]


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("B,M,cx,T,shifts,lpad,extra,ts", TAP_SHAPES)
def test_tap_gemm_and_wgrad_vs_float64(cuda, B, M, cx, T, shifts, lpad, extra, ts, prec):
    run_taps(cuda, prec, B, M, cx, T, shifts, lpad, extra, 1 + 2 * (T % 3), ts, what=f"p{prec} B{B} M{M} cx{cx} T{T} ntap{len(shifts)}")


# One case per layer at the recipes' step shapes.  tts_en_base at B = 128, L = 400 (tools/bench_tts_v2.py): Conv1d 1024 -> 512 k5 at
# T = 400, the two phases of ConvTranspose1d 512 -> 512 (3 and 2 taps, T = 400, Tx = 404: exactly what functional.py allocates), Conv1d
# 512 -> 512 k5 at T = 799; asr_en_base v2's stride-1 block 512 -> 512 k5 at B = 32, T = 512 (32 x 1024 frames behind the stride-2
# opener: tests/test_gpu_models.py).  Each: forward GEMM + weight gradient (G pitch / offset as the caller passes them), then the
# backward-data GEMM (M and cx swapped, taps reversed).  All are in the batch-split regime S <= B.
MODEL_LAYERS = [
    ("tts conv 1024->512 T400", 128, 512, 1024, 400, (0, 1, 2, 3, 4), 2),
    ("tts convT even phase", 128, 512, 512, 400, (2, 1, 0), 1),
    ("tts convT odd phase", 128, 512, 512, 400, (2, 1), 1),
    ("tts conv 512->512 T799", 128, 512, 512, 799, (0, 1, 2, 3, 4), 2),
    ("asr v2 conv 512->512 T512", 32, 512, 512, 512, (0, 1, 2, 3, 4), 2),
]


@pytest.mark.parametrize("prec", [0, 1, 2])
@pytest.mark.parametrize("name,B,M,cx,T,shifts,lpad", MODEL_LAYERS)
def test_tap_gemm_model_layers_vs_float64(cuda, name, B, M, cx, T, shifts, lpad, prec):
    run_taps(cuda, prec, B, M, cx, T, shifts, lpad, 0, 1, 0, what=f"p{prec} {name} fwd")
    if prec < 2:
        run_taps(cuda, prec, B, cx, M, T, tuple(reversed(shifts)), lpad, 0, 1, 0, wgrad=False, what=f"p{prec} {name} bwd-data")


# ------------------------------------------------------------------------------------------------------------------------------
# b. functional.conv1d_dense / conv_transpose1d_k5s2, forward and backward, with the route each case takes asserted first
# ------------------------------------------------------------------------------------------------------------------------------
class Spy:
    """records the entry points that go through voice100_amd._native.call"""

    def __init__(self, monkeypatch):
        N = _native()
        self.names = []
        real = N.call

        def call(name, *args):
            self.names.append(name)
            return real(name, *args)
        monkeypatch.setattr(N, "call", call)

    def take(self):
        out, self.names = self.names, []
        return out


DATA_GRAD = {"v100_pw_gemm_taps", "v100_pw_gemm", "v100_col2im"}     # a backward that needs no dx launches none of these


def run_conv(cuda, monkeypatch, precision, transpose, B, cin, cout, k, stride, pad, T, bias, route, what):
    """route: "taps" (tap-addressed GEMMs, no copy) or "copy" (im2col / col2im for Conv1d, tap-stacked copies + v100_pw_gemm for
    ConvTranspose1d).  Reference: float64 F.conv1d / F.conv_transpose1d on the rounded x, w and (backward) dy."""
    from voice100_amd import functional as F_
    prec = PREC[precision]
    spy = Spy(monkeypatch)
    g = torch.Generator(device=cuda).manual_seed(cin * 5 + cout + 3 * T + k)
    rnd = lambda *s: torch.randn(*s, generator=g, device=cuda)
    x, w_, b_ = rnd(B, cin, T), (rnd(cin, cout, k) if transpose else rnd(cout, cin, k)) / (cin * k) ** 0.5, (rnd(cout) if bias else None)

    def fwd(xd, wd, bd):
        if transpose:
            return F_.conv_transpose1d_k5s2(xd, wd, bd, precision=precision)
        return F_.conv1d_dense(xd, wd, bd, stride=stride, padding=pad, precision=precision)

    def route_ok(names, gemm=True):
        if route == "taps":
            fast, slow = {"v100_pw_gemm_taps", "v100_pw_wgrad_taps"}, {"v100_im2col", "v100_col2im", "v100_pw_gemm", "v100_pw_wgrad"}
        else:
            fast, slow = {"v100_pw_gemm", "v100_pw_wgrad"}, {"v100_pw_gemm_taps", "v100_pw_wgrad_taps"}
            if not transpose:
                assert "v100_im2col" in names, (what, names)
        assert fast & set(names) and not slow & set(names), (what, route, names)

    xr, wr = rd(x, prec).requires_grad_(True), rd(w_, prec).requires_grad_(True)
    yr = F.conv_transpose1d(xr, wr, None, stride=2, padding=2) if transpose else F.conv1d(xr, wr, None, stride=stride, padding=pad)
    yref = yr.detach() + (col(b_) if bias else 0)
    if prec == 2:                                    # fp16: an inference precision, forward only
        with torch.no_grad():
            y = fwd(x, w_, b_)
        route_ok(spy.take())
        assert y.shape == yr.shape
        check(y, yref, what + " y", GEMM_TOL[prec])
        return
    xd, wd = x.clone().requires_grad_(True), w_.clone().requires_grad_(True)
    bd = b_.clone().requires_grad_(True) if bias else None
    y = fwd(xd, wd, bd)
    route_ok(spy.take())
    assert y.shape == yr.shape
    check(y, yref, what + " y", GEMM_TOL[prec])
    dy = rnd(*y.shape)
    y.backward(dy)
    route_ok(spy.take())
    dxr, dwr = torch.autograd.grad(yr, (xr, wr), rd(dy, prec))
    check(xd.grad, dxr, what + " dx", GEMM_TOL[prec])
    check(wd.grad, dwr, what + " dw", WGRAD_TOL[prec])
    if bias:
        check_abs(bd.grad, dy.double().sum((0, 2)), what + " db", 2e-6 * B * y.shape[2])
    # needs_input_grad[0] == False: the same dw / db bit for bit, and no data-gradient launch
    w2 = w_.clone().requires_grad_(True)
    b2 = b_.clone().requires_grad_(True) if bias else None
    y2 = fwd(x, w2, b2)
    spy.take()
    y2.backward(dy)
    names = spy.take()
    assert not DATA_GRAD & set(names), (what, names)
    assert torch.equal(y2, y) and torch.equal(w2.grad, wd.grad) and (not bias or torch.equal(b2.grad, bd.grad)), what


# (B, cin, cout, k, stride, pad, T, bias, route in fp32, route in bf16 / fp16).  Conv1dDenseFn takes the tap-addressed GEMMs for "same"
# stride-1 convolutions of <= 8 taps whose forward and backward-data GEMMs both fit: in bf16 / fp16 that needs cin % 64 == 0 (and
# cout % 64 == 0 for training).  An even k cannot satisfy 2 * pad == k - 1, so 8 taps are reached at kernel level only (TAP_SHAPES).
CONV_CASES = [
    (3, 64, 128, 3, 1, 1, 77, True, "taps", "taps"),          # tap route, k = 3
    (2, 128, 192, 5, 1, 2, 130, True, "taps", "taps"),        # tap route, k = 5
    (2, 64, 64, 7, 1, 3, 300, False, "taps", "taps"),         # tap route, k = 7
    (32, 64, 512, 5, 2, 2, 256, False, "copy", "copy"),       # copy route: stride 2 -- the asr_en_base v2 opener, T even
    (32, 64, 512, 5, 2, 2, 101, False, "copy", "copy"),       # ... T odd
    (2, 64, 64, 5, 1, 1, 50, True, "copy", "copy"),           # copy route: pad != (k - 1) / 2
    (2, 64, 64, 9, 1, 4, 100, True, "copy", "copy"),          # copy route: a "same" convolution of 9 > 8 taps
    (4, 96, 64, 5, 1, 2, 260, True, "taps", "copy"),          # copy route in bf16 / fp16 only: cin = 96 is no multiple of 64
]


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B,cin,cout,k,stride,pad,T,bias,route32,route16", CONV_CASES)
def test_conv1d_dense_vs_float64(cuda, monkeypatch, B, cin, cout, k, stride, pad, T, bias, route32, route16, precision):
    route = route32 if precision == "fp32" else route16
    run_conv(cuda, monkeypatch, precision, False, B, cin, cout, k, stride, pad, T, bias, route,
             f"{precision} conv {cin}->{cout} k{k} s{stride} p{pad} B{B} T{T} [{route}]")


# ConvTranspose1d(k5, s2, p2): (B, cin, cout, L, bias, force_copy)
CONVT_CASES = [(2, 64, 128, 1, True, False), (3, 64, 64, 2, False, False), (2, 128, 64, 3, True, False), (2, 128, 64, 401, False, False),
               (2, 64, 64, 401, True, False),                                             # tap route, L = 1, 2, 3, 401, with / without bias
               (2, 96, 64, 1, True, False), (2, 96, 64, 2, False, False), (3, 96, 128, 130, True, False),   # tap-stacked in bf16 / fp16: cin = 96
               (2, 64, 64, 1, False, True), (2, 64, 128, 2, True, True), (2, 128, 64, 130, True, True)]      # tap-stacked: USE_TAP_GEMM = False


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("B,cin,cout,L,bias,force_copy", CONVT_CASES)
def test_conv_transpose1d_k5s2_vs_float64(cuda, monkeypatch, B, cin, cout, L, bias, force_copy, precision):
    from voice100_amd import functional as F_
    if force_copy:
        monkeypatch.setattr(F_, "USE_TAP_GEMM", False)
    route = "copy" if force_copy or (precision != "fp32" and cin % 64 != 0) else "taps"
    run_conv(cuda, monkeypatch, precision, True, B, cin, cout, 5, 2, 2, L, bias, route,
             f"{precision} convT {cin}->{cout} B{B} L{L} [{route}{' forced' if force_copy else ''}]")


# ------------------------------------------------------------------------------------------------------------------------------
# c. LayerNorm over channels + exact GELU (K11) against float64
# ------------------------------------------------------------------------------------------------------------------------------
# near-constant columns: 1 + NEAR_CONST * randn.  fp32 torch on the CPU against float64, worst of out / dy / dgamma / dbeta as a
# fraction of the bar at (4, 512, 130) | (2, 257, 33): scale 1e-3 0.41 | 0.52, 2e-3 0.27 | 0.22, 3e-3 0.23 | 0.14, 5e-3 0.13 | 0.11,
# 1e-2 0.06 | 0.04.  3e-3 is the first under a quarter but within seed-to-seed spread of it; 5e-3 is the smallest measured scale
# that holds the quarter rule with a factor of two to spare (the other families: benign 0.002, offset 0.045, tails 0.001).
NEAR_CONST = 5e-3
LN_FAMILIES = ["benign", "offset", "tails", "near_const"]
# (B, C, T): NI = ceil(C / 32) selects the kernel's register width -- <= 8 (C <= 256), <= 16 (C <= 512), else 32
LN_SHAPES = [(1, 1, 1),            # B = 1, T = 1, C = 1
             (2, 1, 33),           # C = 1; T % 32 = 1
             (3, 32, 64),          # one full channel pass; T % 32 = 0
             (2, 33, 31),          # C = 32 + 1; T % 32 = 31, T % 4 = 3
             (2, 256, 95),         # last C of NI = 8; T % 32 = 31
             (2, 257, 33),         # first C of NI = 16; T % 32 = 1
             (4, 512, 130),        # last C of NI = 16; T % 4 = 2
             (2, 513, 63),         # first C of NI = 32; T % 32 = 31
             (2, 1024, 65),        # the cap; T % 32 = 1
             (128, 512, 799)]      # tts_en_base's blocks at the recipe's batch


LN_QUARTER_SHAPES = {(4, 512, 130), (2, 257, 33)}


def ln_inputs(family, B, C, T, gen):
    r = torch.randn(B, C, T, generator=gen)
    ga, be = torch.rand(C, generator=gen) + 0.5, torch.randn(C, generator=gen) * 0.3
    if family == "benign":
        y = 2 * r + 0.5
    elif family == "offset":          # a large common offset: a one-pass E[x^2] - E[x]^2 variance is off by ~3e-4 in rstd here
        y = r + 100
    elif family == "tails":           # |z| passes 10: both tails of erf and of the exp in GELU's derivative
        y, ga = 4 * r, ga * 3
    else:
        y = 1 + NEAR_CONST * r
    return y, ga, be, torch.randn(B, C, T, generator=gen)


def ln_ref(y, ga, be, go, dtype, device):
    yy, g, b = (t.to(device=device, dtype=dtype).clone().requires_grad_(True) for t in (y, ga, be))
    out = F.gelu(F.layer_norm(yy.transpose(1, 2), (y.shape[1],), g, b, 1e-5).transpose(1, 2))
    (out * go.to(device=device, dtype=dtype)).sum().backward()
    return out.detach(), yy.grad, g.grad, b.grad


LN_BARS = (("out", 1e-4, 1e-5), ("dy", 2e-4, 1e-4), ("dgamma", 2e-4, 1e-3), ("dbeta", 2e-4, 1e-3))   # (tensor, bar, floor of rel_err)


def ln_rel(a, b, floor):
    """conftest.rel_err, on whatever device the tensors are"""
    a, b = a.double(), b.double().to(a.device)
    return float((a - b).abs().max()) / max(float(b.abs().max()), floor)


@pytest.mark.parametrize("family", LN_FAMILIES)
@pytest.mark.parametrize("B,C,T", LN_SHAPES)
def test_layer_norm_gelu_vs_float64(cuda, B, C, T, family):
    from voice100_amd import functional as F_
    N = _native()
    gen = torch.Generator().manual_seed(C * 3 + T + LN_FAMILIES.index(family))
    y, ga, be, go = ln_inputs(family, B, C, T, gen)
    ref = ln_ref(y, ga, be, go, torch.float64, cuda)
    what = f"ln_gelu {family} ({B}, {C}, {T})"
    # the bar stands for this family only if fp32 torch (CPU) on the same inputs is within a quarter of it against float64: asserted
    # at the two shapes the rule was measured at, printed elsewhere (at C = 1 fp32 torch is no yardstick: its backward cancels terms
    # of size rstd = 1 / sqrt(eps) = 316 and is off by 6e-5 where the exact gradient, and the kernel's formula, give 0)
    if B * C * T <= 300000:
        cpu = ln_ref(y, ga, be, go, torch.float32, "cpu")
        for (name, bar, floor), c_, r_ in zip(LN_BARS, cpu, ref):
            e = ln_rel(c_.to(cuda), r_, floor)
            print(f"[v2-conv-oracle] {what} fp32-torch {name}: err/bar = {e / bar:.4f}")
            if (B, C, T) in LN_QUARTER_SHAPES:
                assert e <= bar / 4, (what, name, e)
    # regime: the slab count of the backward and the register width the launcher picks for this C
    parts = N.helper("v100_ln_num_parts", B, T)
    assert parts == B * -(-T // 32)
    ni = -(-C // 32)
    assert (8 if ni <= 8 else 16 if ni <= 16 else 32) == {1: 8, 32: 8, 33: 8, 256: 8, 257: 16, 512: 16, 513: 32, 1024: 32}[C]
    yd, gd, bd = (t.to(cuda).requires_grad_(True) for t in (y, ga, be))
    out = F_.layer_norm_gelu(yd, gd, bd, 1e-5)
    out.backward(go.to(cuda))
    got = (out.detach(), yd.grad, gd.grad, bd.grad)
    for (name, bar, floor), g_, r_ in zip(LN_BARS, got, ref):
        assert torch.isfinite(g_).all(), (what, name)
        e = ln_rel(g_, r_, floor)
        print(f"[v2-conv-oracle] {what} {name}: worst/bar = {e / bar:.4f}")
        assert e < bar, f"{what} {name}: rel_err {e:.3e} >= {bar}"
    # the backward is deterministic (fixed-order slab sum): a second run is bit-identical
    yd2, gd2, bd2 = (t.to(cuda).requires_grad_(True) for t in (y, ga, be))
    F_.layer_norm_gelu(yd2, gd2, bd2, 1e-5).backward(go.to(cuda))
    assert torch.equal(yd2.grad, yd.grad) and torch.equal(gd2.grad, gd.grad) and torch.equal(bd2.grad, bd.grad), what


def test_layer_norm_gelu_refuses_more_than_1024_channels(cuda):
    from voice100_amd import functional as F_
    with pytest.raises(RuntimeError):                  # refused on the host (C > 32 rows x 32 registers), nothing is launched
        F_.layer_norm_gelu(torch.zeros(1, 1025, 4, device=cuda), torch.ones(1025, device=cuda), torch.zeros(1025, device=cuda), 1e-5)
