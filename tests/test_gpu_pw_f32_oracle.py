"""The fp32-STORAGE 1x1 entry points v100_pw_gemm and v100_pw_wgrad, operand modes 0 (fp32) and 1 (bf16), checked ELEMENT BY ELEMENT
against float64 on the operands as the kernels define them (the conventions of tests/test_gpu_io_oracle.py):

  * a transformed X (or G) is formed in fp32 with the kernel's own fused operations -- relu6f(fmaf(v, a, b)) or
    fmaf(v, a, fmaf(v2, b, c)): pw_x_transform, csrc/pointwise_common.h:66-70 -- and, in bf16 mode, rounded once to nearest-even:
    the GEMM stages pack16(pw_x_transform(...)) (csrc/pointwise_bf16_gemm8.h:88-96), the weight gradient pack_bf16 of both operands
    (csrc/pointwise_bf16_wgrad.h:59-64; pack_bf16 is one v_cvt_pk_bf16_f32, csrc/common.h:72-78), the small-K VALU kernel f2bf of X
    (csrc/pointwise.hip:243-246); fp32 mode rounds nothing (pointwise_f32.hip:59, :165-166);
  * A is rounded once: the caller's bf16 copy;
  * products are exact, accumulation fp32 (reference: float64); the epilogues are relu6f(fmaf(y, ea, eb)), fmaf(y, ea, eb) + R,
    the mask [0 < fmaf(R, ea, eb) < 6] on the fp32 pre (csrc/pointwise_common.h:151-161).

Bars, every element: max |got - ref| <= 1e-4 * max(1, max |ref|) in fp32 mode, 2e-4 in bf16 mode; weight gradients 1e-4 / 3e-4; the
epilogue statistics in the form test_dwconv_io_vs_float64 uses for `st`.  Y, stats, partial and dW are NaN-filled with NaN slack around
them, the inputs sit directly in front of NaN slack; every slab row must come back finite.  Run with -s for worst / bar."""
import pytest
import torch

from test_gpu_dw_f32_oracle import Buf
from test_gpu_io_oracle import affine2, affine_relu6, bf, col, fma32
from test_gpu_v2_conv_oracle import splits_rule

pytestmark = pytest.mark.gpu

GEMM_TOL = {0: 1e-4, 1: 2e-4}
WGRAD_TOL = {0: 1e-4, 1: 3e-4}


def _native():
    from voice100_amd import _native as N
    N.load()
    return N


def judge(what, got, ref, tol):
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), f"{what}: not every element was written"
    bound = tol * max(1.0, float(ref.abs().max()))
    worst = float((got - ref).abs().max())
    print(f"[pw-f32-oracle] {what}: worst/bar = {worst / bound:.4f} (worst {worst:.3e}, bar {bound:.3e})")
    assert worst <= bound, f"{what}: max err {worst:.3e} > {bound:.3e}"


def judge_stats(what, st, y, second, tol):
    """st [parts, M, 2]: every part written; the sums over the parts against (sum y, sum y * second) per output channel"""
    assert bool(torch.isfinite(st).all()), f"{what}: a slab row was not written"
    s = st.double().sum(0)
    for j, (ref, mag) in enumerate(((y.sum((0, 2)), y.abs().sum((0, 2))), ((y * second).sum((0, 2)), (y * second).abs().sum((0, 2))))):
        bound = tol * max(1.0, float(mag.max()))
        worst = float((s[:, j] - ref).abs().max())
        print(f"[pw-f32-oracle] {what} sum{j}: worst/bar = {worst / bound:.4f}")
        assert worst <= bound, f"{what} sum{j}: {worst:.3e} > {bound:.3e}"


def spread_of(n, device):
    """magnitudes 10^(-3 .. 3) over n channels"""
    return 10.0 ** torch.linspace(-3, 3, n, device=device) if n > 1 else torch.ones(1, device=device)


# (B, M, K, T, all): all = False runs the plain and the bias store only
GEMM_SHAPES = [(2, 40, 24, 200, True), (1, 2, 8, 33, True),
               (2, 130, 7, 64, True),          # K % 4 != 0
               (2, 129, 64, 131, True),        # T % 4 != 0, a partial tile in M and in T
               (3, 128, 64, 256, True),
               (2, 256, 192, 128, True),       # an odd k-tile count
               (2, 512, 29, 512, False),       # the small-K VALU kernel
               (1, 260, 320, 129, True)]
SPREAD_SHAPES = {(2, 40, 24, 200), (2, 129, 64, 131)}
GEMM_CASES = [(B, M, K, T, al, "benign") for B, M, K, T, al in GEMM_SHAPES] + \
             [(B, M, K, T, al, "spread") for B, M, K, T, al in GEMM_SHAPES if (B, M, K, T) in SPREAD_SHAPES]


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("B,M,K,T,all_modes,family", GEMM_CASES)
def test_pw_gemm_f32_storage_vs_float64(cuda, B, M, K, T, all_modes, family, bf16):
    N = _native()
    g = torch.Generator(device=cuda).manual_seed(M * 7 + K + 3 * T + bf16)
    rnd = lambda *s: torch.randn(*s, generator=g, device=cuda)         # noqa: E731
    uni = lambda *s: torch.rand(*s, generator=g, device=cuda)          # noqa: E731
    A, X, X2 = rnd(M, K) / K ** 0.5, rnd(B, K, T), rnd(B, K, T)
    if family == "spread":
        A = A * spread_of(M, cuda)[:, None]
        X, X2 = X * spread_of(K, cuda)[None, :, None], X2 * spread_of(K, cuda).flip(0)[None, :, None]
    xa, xb, xc = uni(K) + 0.5, rnd(K), rnd(K) * 0.1
    ea, eb, bias, R = uni(M) + 0.5, rnd(M), rnd(M), rnd(B, M, T) * 3
    # the clamp epilogue's scale: in `spread` it undoes the row's magnitude, as the BatchNorm it folds does (gamma / std).  With a
    # scale of order 1 an output inside (0, 6) is the difference of terms of size 1e3: its fp32 rounding error (measured: 8e-4, where
    # the plain store of the same accumulators is at 7e-4 of ITS bar) is no fault of the kernel, and the 1e-4 * max(1, 6) bar of the
    # clamped tensor cannot be met by any fp32 accumulation
    ea2 = ea / (spread_of(M, cuda) * spread_of(K, cuda).square().mean().sqrt()) if family == "spread" else ea.clone()
    parts = N.helper("v100_pw_num_parts", B, T)
    ins = {k: Buf(tuple(v.shape), cuda, v) for k, v in dict(A=A, X=X, X2=X2, xa=xa, xb=xb, xc=xc, ea=ea, ea2=ea2, eb=eb, bias=bias, R=R).items()}
    Abf = Buf((M, K), cuda, A.to(torch.bfloat16), dtype=torch.bfloat16) if bf16 else None
    i = {k: b.t for k, b in ins.items()}
    tol = GEMM_TOL[bf16]
    rd = (lambda t: bf(t.float()).double()) if bf16 else (lambda t: t.double())
    Ad = rd(A)
    xop = {0: X.double(), 1: affine_relu6(X.double(), xa, xb), 2: affine2(X.double(), X2.double(), xa, xb, xc)}
    base = {m: torch.einsum("mk,bkt->bmt", Ad, rd(v)) for m, v in xop.items()}
    what0 = f"{'bf16' if bf16 else 'fp32'} {family} ({B}, {M}, {K}, {T})"

    def run(x_mode, epi, use_bias=False):
        Y, st = Buf((B, M, T), cuda), Buf((parts, M, 2), cuda)
        N.call("v100_pw_gemm", i["A"], Abf.t if bf16 else None, i["X"], i["X2"], i["xa"], i["xb"], i["xc"], x_mode, Y.t,
               i["bias"] if use_bias else None, i["ea2"] if epi == 2 else i["ea"], i["eb"], i["R"], epi, st.t, B, M, K, T, bf16)
        torch.cuda.synchronize()
        for b in list(ins.values()) + [Y, st] + ([Abf] if bf16 else []):
            assert b.slack_intact(), f"{what0} x{x_mode} e{epi}: the NaN slack around a tensor was written"
        if epi not in (1, 4):
            assert bool(torch.isnan(st.t).all()), f"{what0} x{x_mode} e{epi}: stats written by an epilogue without statistics"
        return Y.t, st.t

    y, _ = run(0, 0, use_bias=True)
    judge(f"{what0} store + bias", y, base[0] + col(bias), tol)
    y, _ = run(0, 0)
    judge(f"{what0} store", y, base[0], tol)
    if not all_modes:
        return
    y, st = run(1, 1)
    judge(f"{what0} x1 stats-store", y, base[1], tol)
    judge_stats(f"{what0} x1 stats", st, base[1], base[1], tol)
    y, _ = run(0, 2)
    judge(f"{what0} affine+relu6", y, (base[0] * col(ea2) + col(eb)).clamp(0, 6), tol)
    y, _ = run(1, 3)
    judge(f"{what0} x1 affine+R", y, base[1] * col(ea) + col(eb) + R.double(), tol)
    y, st = run(0, 4)
    pre = fma32(R.double(), col(ea), col(eb))
    ref = base[0] * ((pre > 0) & (pre < 6)).double()
    judge(f"{what0} mask", y, ref, tol)
    judge_stats(f"{what0} mask stats", st, ref, R.double(), tol)
    y, _ = run(2, 5)
    judge(f"{what0} x2 +R", y, base[2] + R.double(), tol)


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("B,M,K,T", [(3, 40, 24, 200), (2, 29, 130, 77), (2, 130, 260, 129), (4, 256, 64, 512)])
def test_pw_wgrad_f32_storage_vs_float64(cuda, B, M, K, T, bf16):
    N = _native()
    g = torch.Generator(device=cuda).manual_seed(M + 5 * K + T + bf16)
    rnd = lambda *s: torch.randn(*s, generator=g, device=cuda)         # noqa: E731
    Gt, G2, X = rnd(B, M, T), rnd(B, M, T), rnd(B, K, T)
    ga, gb, gc = rnd(M), rnd(M) * 0.2, rnd(M) * 0.1
    xa, xb = torch.rand(K, generator=g, device=cuda) + 0.5, rnd(K)
    S = N.helper("v100_pw_wgrad_splits", B, M, K)
    assert S == splits_rule(B, M, K)[0], (S, splits_rule(B, M, K))
    ins = {k: Buf(tuple(v.shape), cuda, v) for k, v in dict(G=Gt, G2=G2, X=X, ga=ga, gb=gb, gc=gc, xa=xa, xb=xb).items()}
    i = {k: b.t for k, b in ins.items()}
    rd = (lambda t: bf(t.float()).double()) if bf16 else (lambda t: t.double())
    what0 = f"{'bf16' if bf16 else 'fp32'} wgrad ({B}, {M}, {K}, {T}) S={S}"
    for g_mode, x_mode in ((0, 0), (2, 1)):
        partial, dW = Buf((S, M, K), cuda), Buf((M, K), cuda)
        if g_mode == 0:
            N.call("v100_pw_wgrad", i["G"], None, None, None, None, 0, i["X"], None, None, 0, partial.t, dW.t, S, B, M, K, T, bf16)
            gop, xop = Gt.double(), X.double()
        else:
            N.call("v100_pw_wgrad", i["G"], i["G2"], i["ga"], i["gb"], i["gc"], 2, i["X"], i["xa"], i["xb"], 1, partial.t, dW.t, S, B, M, K,
                   T, bf16)
            gop, xop = affine2(Gt.double(), G2.double(), ga, gb, gc), affine_relu6(X.double(), xa, xb)
        torch.cuda.synchronize()
        for b in list(ins.values()) + [partial, dW]:
            assert b.slack_intact(), f"{what0} g{g_mode} x{x_mode}: the NaN slack around a tensor was written"
        assert bool(torch.isfinite(partial.t).all()), f"{what0} g{g_mode} x{x_mode}: a slab was not written"
        judge(f"{what0} g{g_mode} x{x_mode}", dW.t, torch.einsum("bmt,bkt->mk", rd(gop), rd(xop)), WGRAD_TOL[bf16])
