"""Kernel-level parity (GPU): each C-ABI entry point against the CPU oracle / torch fp32 on
seeded inputs.  Tolerance: <= 1e-4 relative (max-abs error / max-abs reference), fp32 paths;
bf16 GEMM operands: <= 2e-2.  The per-element float64 checks of the fp32-storage depthwise and 1x1 kernels, in every launch regime,
are tests/test_gpu_dw_f32_oracle.py and tests/test_gpu_pw_f32_oracle.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-4


def _native():
    from voice100_amd import _native as N
    return N


def _dw_ref(x, w, stride, pad):
    return F.conv1d(x, w[:, None, :], stride=stride, padding=pad, groups=x.shape[1])


DW_CASES = [  # (B, C, T, K, stride, force_generic)
    (3, 5, 700, 83, 1, 0), (2, 4, 1024, 59, 1, 0), (2, 3, 513, 19, 1, 0), (2, 6, 96, 11, 1, 0),
    (2, 4, 1000, 11, 2, 0), (1, 3, 61, 11, 2, 0), (2, 3, 300, 7, 1, 0), (2, 3, 130, 13, 1, 0),
    (2, 3, 257, 35, 1, 1), (1, 2, 40, 5, 1, 0), (4, 2, 2048, 51, 1, 0), (2, 2, 1023, 33, 1, 0),
]


@pytest.mark.parametrize("B,C,T,K,stride,generic", DW_CASES)
def test_dwconv_forward_train_and_eval(cuda, B, C, T, K, stride, generic):
    N = _native()
    g = torch.Generator().manual_seed(K * 1000 + T)
    x = torch.randn(B, C, T, generator=g)
    w = torch.randn(C, K, generator=g) * 0.2
    s = torch.rand(C, generator=g) + 0.5
    sh = torch.randn(C, generator=g)
    pad = (K - 1) // 2
    h = torch.clamp(x * s[None, :, None] + sh[None, :, None], 0, 6)
    ref = _dw_ref(h, w, stride, pad)
    Tout = ref.shape[2]
    G = N.helper("v100_dw_num_groups", B, C)
    xd, wd, sd, shd = (t.to(cuda) for t in (x, w, s, sh))
    y = torch.empty(B, C, Tout, device=cuda)
    st = torch.zeros(G, C, 2, device=cuda)
    N.call("v100_dwconv", xd, None, wd, sd, shd, None, 1, y, None, None, None, 0, st, G, B, C, T, Tout, K, stride, pad, 0, 1, generic)
    assert rel_err(y, ref) < TOL
    stats = st.sum(0).cpu()
    assert rel_err(stats[:, 0], ref.sum((0, 2)), floor=1e-2) < 1e-3
    assert rel_err(stats[:, 1], (ref * ref).sum((0, 2))) < 1e-4
    # eval: plain input, folded BN + ReLU6 epilogue
    oa, ob = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    ref2 = torch.clamp(_dw_ref(x, w, stride, pad) * oa[None, :, None] + ob[None, :, None], 0, 6)
    y2 = torch.empty_like(y)
    N.call("v100_dwconv", xd, None, wd, None, None, None, 0, y2, None, oa.to(cuda), ob.to(cuda), 1, None, G, B, C, T, Tout, K, stride, pad, 0, 1, generic)
    assert rel_err(y2, ref2) < TOL


@pytest.mark.parametrize("B,C,T,K,stride", [(2, 4, 600, 83, 1), (3, 3, 520, 27, 1), (2, 4, 1000, 11, 2), (2, 3, 77, 11, 2),
                                           (2, 2, 90, 9, 1), (2, 3, 1023, 65, 1)])
def test_dwconv_backward_data_and_weight(cuda, B, C, T, K, stride):
    """The fused backward kernels against autograd through conv(relu6(bn-affine(a1))) with a BN-backward-shaped
    incoming gradient (da2 = p*dz2 + q*a2 + r)."""
    N = _native()
    g = torch.Generator().manual_seed(K + T)
    pad = (K - 1) // 2
    a1 = torch.randn(B, C, T, generator=g) * 2
    w = (torch.randn(C, K, generator=g) * 0.2)
    s1, t1 = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    a1g = a1.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    h1 = torch.clamp(a1g * s1[None, :, None] + t1[None, :, None], 0, 6)
    a2 = _dw_ref(h1, wg, stride, pad)
    Tout = a2.shape[2]
    dz2 = torch.randn(B, C, Tout, generator=g)
    p, q, r = torch.randn(C, generator=g), torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    da2 = p[None, :, None] * dz2 + q[None, :, None] * a2.detach() + r[None, :, None]
    a2.backward(da2)
    pre = a1 * s1[None, :, None] + t1[None, :, None]
    dh1_ref = a1g.grad / s1[None, :, None]           # undo the affine's chain factor: kernel returns dz1 = dh1 * mask
    mask = ((pre > 0) & (pre < 6)).float()
    G = N.helper("v100_dw_num_groups", B, C)
    dev = lambda t: t.to(cuda).contiguous()
    dz1 = torch.empty(B, C, T, device=cuda)
    st = torch.zeros(G, C, 2, device=cuda)
    N.call("v100_dwconv", dev(dz2), dev(a2.detach()), dev(w), dev(p), dev(q), dev(r), 2, dz1, dev(a1), dev(s1), dev(t1), 2, st, G,
           B, C, Tout, T, K, 1, K - 1 - pad, 1, stride, 0)
    assert rel_err(dz1, dh1_ref * mask) < TOL
    stats = st.sum(0).cpu()
    assert rel_err(stats[:, 0], (dh1_ref * mask).sum((0, 2)), floor=1e-2) < 1e-3
    assert rel_err(stats[:, 1], (dh1_ref * mask * a1).sum((0, 2)), floor=1e-2) < 1e-3
    partial = torch.empty(G, C, K, device=cuda)
    dw = torch.empty(C, K, device=cuda)
    N.call("v100_dwconv_wgrad", dev(dz2), dev(a2.detach()), dev(p), dev(q), dev(r), 2, dev(a1), dev(s1), dev(t1), 1, partial, dw,
           G, B, C, T, Tout, K, stride, pad, 0)
    assert rel_err(dw, wg.grad) < TOL
    N.call("v100_dwconv_wgrad", dev(dz2), dev(a2.detach()), dev(p), dev(q), dev(r), 2, dev(a1), dev(s1), dev(t1), 1, partial, dw,
           G, B, C, T, Tout, K, stride, pad, 1)
    assert rel_err(dw, wg.grad) < TOL


GEMM_CASES = [(2, 40, 24, 200), (3, 128, 64, 256), (1, 29, 512, 130), (2, 260, 256, 1023), (2, 256, 1024, 512), (1, 2, 8, 33),
              (2, 512, 320, 128), (1, 128, 192, 256),     # odd k-tile counts on both block-tile heights
              (2, 512, 29, 512), (3, 130, 7, 64)]         # K <= 32: plain / bias stores take the small-K VALU kernel (vocabulary-head data gradient)


@pytest.mark.parametrize("B,M,K,T", GEMM_CASES)
@pytest.mark.parametrize("bf16", [0, 1])
def test_pw_gemm_modes(cuda, B, M, K, T, bf16):
    N = _native()
    g = torch.Generator().manual_seed(M * 7 + K)
    tol = 2e-2 if bf16 else TOL
    A = torch.randn(M, K, generator=g) / K ** 0.5
    X = torch.randn(B, K, T, generator=g)
    X2 = torch.randn(B, K, T, generator=g)
    xa, xb, xc = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g), torch.randn(K, generator=g) * 0.1
    ea, eb = torch.rand(M, generator=g) + 0.5, torch.randn(M, generator=g)
    bias = torch.randn(M, generator=g)
    R = torch.randn(B, M, T, generator=g) * 3
    dev = lambda t: t.to(cuda).contiguous()
    Ad = dev(A)
    Abf = Ad.to(torch.bfloat16) if bf16 else None
    parts = N.helper("v100_pw_num_parts", B, T)

    def run(x_mode, epi, use_bias=False):
        Y = torch.full((B, M, T), float("nan"), device=cuda)
        st = torch.zeros(parts, M, 2, device=cuda)
        N.call("v100_pw_gemm", Ad, Abf, dev(X), dev(X2), dev(xa), dev(xb), dev(xc), x_mode, Y, dev(bias) if use_bias else None,
               dev(ea), dev(eb), dev(R), epi, st, B, M, K, T, bf16)
        return Y.cpu(), st.sum(0).cpu()

    xf = {0: X, 1: torch.clamp(X * xa[None, :, None] + xb[None, :, None], 0, 6),
          2: xa[None, :, None] * X + xb[None, :, None] * X2 + xc[None, :, None]}
    base = {m: torch.einsum("mk,bkt->bmt", A, v) for m, v in xf.items()}
    y, _ = run(0, 0, use_bias=True)
    assert rel_err(y, base[0] + bias[None, :, None]) < tol
    # no bias: full tiles take the lean epilogue (16-byte stores).  ELEMENTWISE bound against a reference on the operands as the
    # kernel rounds them -- an L2 norm hides a few wrong elements (a store-data hazard once corrupted 0.15 % of them)
    y, _ = run(0, 0)
    rnd = (lambda t: t.to(torch.bfloat16).to(torch.float32)) if bf16 else (lambda t: t)
    exact = torch.einsum("mk,bkt->bmt", rnd(A).double(), rnd(X).double()).float()
    assert float((y - exact).abs().max()) < 2e-4 * max(1.0, float(exact.abs().max()))
    y, st = run(1, 1)
    assert rel_err(y, base[1]) < tol
    assert rel_err(st[:, 0], base[1].sum((0, 2)), floor=1.0) < 10 * tol and rel_err(st[:, 1], (base[1] ** 2).sum((0, 2))) < 10 * tol
    y, _ = run(0, 2)
    assert rel_err(y, torch.clamp(base[0] * ea[None, :, None] + eb[None, :, None], 0, 6)) < tol
    y, _ = run(1, 3)
    assert rel_err(y, base[1] * ea[None, :, None] + eb[None, :, None] + R) < tol
    y, st = run(0, 4)
    pre = R * ea[None, :, None] + eb[None, :, None]
    ref = base[0] * ((pre > 0) & (pre < 6)).float()
    assert rel_err(y, ref) < tol
    assert rel_err(st[:, 0], ref.sum((0, 2)), floor=1.0) < 10 * tol and rel_err(st[:, 1], (ref * R).sum((0, 2)), floor=1.0) < 10 * tol
    y, _ = run(2, 5)
    assert rel_err(y, base[2] + R) < tol


@pytest.mark.parametrize("B,M,K,T", [(3, 40, 24, 200), (4, 256, 64, 512), (2, 29, 130, 77), (2, 130, 260, 1023)])
@pytest.mark.parametrize("bf16", [0, 1])
def test_pw_wgrad(cuda, B, M, K, T, bf16):
    N = _native()
    g = torch.Generator().manual_seed(M + K + T)
    tol = 2e-2 if bf16 else TOL
    Gt = torch.randn(B, M, T, generator=g)
    G2 = torch.randn(B, M, T, generator=g)
    ga, gb, gc = torch.randn(M, generator=g), torch.randn(M, generator=g) * 0.2, torch.randn(M, generator=g) * 0.1
    X = torch.randn(B, K, T, generator=g)
    xa, xb = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    dev = lambda t: t.to(cuda).contiguous()
    S = N.helper("v100_pw_wgrad_splits", B, M, K)
    partial = torch.empty(S, M, K, device=cuda)
    dW = torch.empty(M, K, device=cuda)
    N.call("v100_pw_wgrad", dev(Gt), None, None, None, None, 0, dev(X), None, None, 0, partial, dW, S, B, M, K, T, bf16)
    assert rel_err(dW, torch.einsum("bmt,bkt->mk", Gt, X)) < tol
    gp = ga[None, :, None] * Gt + gb[None, :, None] * G2 + gc[None, :, None]
    xp = torch.clamp(X * xa[None, :, None] + xb[None, :, None], 0, 6)
    N.call("v100_pw_wgrad", dev(Gt), dev(G2), dev(ga), dev(gb), dev(gc), 2, dev(X), dev(xa), dev(xb), 1, partial, dW, S, B, M, K, T, bf16)
    assert rel_err(dW, torch.einsum("bmt,bkt->mk", gp, xp)) < tol


def test_bn_finalize_and_backward_coeffs(cuda):
    N = _native()
    g = torch.Generator().manual_seed(5)
    B, C, T = 4, 7, 333
    a = torch.randn(B, C, T, generator=g) * 2 + 1
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    bn = torch.nn.BatchNorm1d(C)
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta); bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    ag = a.clone().requires_grad_(True)
    y = bn(ag)
    dz = torch.randn(B, C, T, generator=g)
    y.backward(dz)
    dev = lambda t: t.to(cuda).contiguous()
    G = 2
    part = torch.empty(G, C, 2, device=cuda)
    N.call("v100_chan_reduce2", dev(a), None, part, G, B, C, T)
    rmd, rvd, nbt = dev(rm), dev(rv), torch.zeros((), dtype=torch.int64, device=cuda)
    sc, sh, mean, rstd = (torch.empty(C, device=cuda) for _ in range(4))
    N.call("v100_bn_finalize_train", part, G, B * T, dev(gamma), dev(beta), rmd, rvd, nbt, 0.1, 1e-5, sc, sh, mean, rstd, C)
    assert rel_err(dev(a) * sc[None, :, None] + sh[None, :, None], y) < TOL
    assert rel_err(rmd, bn.running_mean) < 1e-5 and rel_err(rvd, bn.running_var) < 1e-5 and int(nbt) == 1
    N.call("v100_chan_reduce2", dev(dz), dev(a), part, G, B, C, T)
    p, q, r, dg, db = (torch.empty(C, device=cuda) for _ in range(5))
    N.call("v100_bn_bwd_finalize", part, G, B * T, dev(gamma), mean, rstd, p, q, r, dg, db, C)
    da = torch.empty(B, C, T, device=cuda)
    N.call("v100_chan_affine2", dev(dz), dev(a), p, q, r, da, B, C, T)
    assert rel_err(da, ag.grad) < TOL
    assert rel_err(dg, bn.weight.grad) < TOL and rel_err(db, bn.bias.grad) < TOL
    N.call("v100_bn_eval_coeffs", dev(gamma), dev(beta), dev(rm), dev(rv), 1e-5, sc, sh, C)
    bn2 = torch.nn.BatchNorm1d(C).eval()
    with torch.no_grad():
        bn2.weight.copy_(gamma); bn2.bias.copy_(beta); bn2.running_mean.copy_(rm); bn2.running_var.copy_(rv)
        assert rel_err(dev(a) * sc[None, :, None] + sh[None, :, None], bn2(a)) < TOL


def test_layout_embedding_dropout(cuda):
    from voice100_amd import functional as F_
    g = torch.Generator().manual_seed(9)
    x = torch.randn(3, 101, 64, generator=g).to(cuda).requires_grad_(True)
    y = F_.transpose_last2(x)
    assert torch.equal(y.detach().cpu(), x.detach().cpu().transpose(1, 2))
    gy = torch.randn(3, 64, 101, generator=g)
    y.backward(gy.to(cuda))
    assert torch.equal(x.grad.cpu(), gy.transpose(1, 2))
    table = torch.randn(29, 48, generator=g).to(cuda).requires_grad_(True)
    idx = torch.randint(0, 29, (2, 77), generator=g)
    e = F_.embedding_bct(idx.to(cuda), table)
    ref_t = table.detach().cpu().clone().requires_grad_(True)
    ref = F.embedding(idx, ref_t).transpose(1, 2)
    assert torch.equal(e.detach().cpu(), ref.detach())
    ge = torch.randn(2, 48, 77, generator=g)
    e.backward(ge.to(cuda)); ref.backward(ge)
    assert rel_err(table.grad, ref_t.grad) < 1e-5
    keep = (torch.rand(2, 8, 50, generator=g) > 0.2).float()
    h = torch.randn(2, 8, 50, generator=g)
    out = F_.dropout(h.to(cuda), 0.2, True, keep.to(cuda))
    assert rel_err(out, h * keep / 0.8) < 1e-6


def test_errors_are_loud(cuda):
    N = _native()
    x = torch.zeros(1, 2, 8, device=cuda)
    with pytest.raises(RuntimeError):
        N.call("v100_dwconv", x, None, None, None, None, None, 0, x, None, None, None, 3, None, 1, 1, 2, 8, 8, 3, 1, 1, 0, 1, 0)
    with pytest.raises(RuntimeError):
        N.call("v100_pw_gemm", None, None, x, None, None, None, None, 0, x, None, None, None, None, 0, None, 1, 2, 2, 8, 0)
    with pytest.raises(RuntimeError):
        N.call("v100_transpose_last2", torch.zeros(2, 2), torch.zeros(2, 2), 1, 2, 2)       # CPU tensors are refused
    from voice100_amd.layers import InvertedResidual
    with pytest.raises(RuntimeError):
        InvertedResidual(4, 4, 5)(torch.zeros(1, 4, 16))                                     # no CPU fallback


@pytest.mark.parametrize("B,T,V,L", [(3, 40, 29, 7), (4, 130, 71, 30), (2, 9, 5, 6), (5, 64, 29, 1),
                                     (3, 700, 29, 300), (2, 1300, 71, 600), (2, 2500, 29, 1200),    # L > 255: 4 / 8 / 16 states per thread
                                     (2, 1100, 29, 505),                                            # 1011 states: the 16-wave pipeline
                                     (32, 512, 29, 100), (3, 700, 29, 127), (6, 300, 128, 90), (2, 777, 5, 64)])   # the bench shape; the class limit V = 128; few classes
def test_ctc_loss_fused(cuda, B, T, V, L):
    """Fused log_softmax + CTC (value and gradient) vs torch's CPU F.ctc_loss, ragged lengths, repeated labels,
    an infeasible utterance (zero_infinity) and an empty target."""
    from voice100_amd import functional as F_
    g = torch.Generator().manual_seed(B * 100 + T)
    logits = torch.randn(B, T, V, generator=g) * 2
    targets = torch.randint(1, V, (B, L), generator=g)
    if L > 2:
        targets[0, 1] = targets[0, 0]                      # repeated label needs a blank in between
    in_len = torch.randint(min(2 * L + 1, T), T + 1, (B,), generator=g).to(torch.int32)
    tgt_len = torch.randint(1, L + 1, (B,), generator=g).to(torch.int32)
    if B >= 4:
        in_len[1] = max(1, int(tgt_len[1]) - 1)            # too short: infinite loss -> zeroed
        tgt_len[2] = 0                                      # empty target
    # reference in float64: torch's own fp32 CPU lattice is itself 8e-4 (T = 700) ... 4e-3 (T = 1100) off the exact gradient -- more
    # than the kernel under test (5e-4 / 2e-3, tools/micro/ctc_acc.py) -- so two fp32 implementations can differ by the sum
    ref_in = logits.double().clone().requires_grad_(True)
    ref = F.ctc_loss(F.log_softmax(ref_in.transpose(0, 1), dim=-1), targets, in_len, tgt_len, blank=0, reduction="mean",
                     zero_infinity=True)
    ref.backward()
    x = logits.to(cuda).requires_grad_(True)
    loss = F_.ctc_loss(x, targets.to(cuda), in_len.to(cuda), tgt_len.to(cuda))
    loss.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-4 * max(1.0, abs(float(ref.detach())))
    # lattice values grow with T (|alpha + beta| ~ 1e3 at T = 700: one fp32 ulp there is 6e-5 in the log domain, and the
    # occupancy exp(alpha + beta + nll - logp) inherits it), so the long cases compare at a wider fp32 bar
    assert rel_err(x.grad, ref_in.grad.float()) < (2e-4 if T <= 200 else 5e-3)


def test_ctc_gradient_survives_a_wide_class_spread(cuda):
    """Round 6: the gradient kernel normalises exp(alpha + beta) per CLASS.  Normalised by the frame's overall maximum (rounds 2-5) a
    class more than ~87 nats below the frame's best one underflowed to an occupancy of exactly 0 although the transcript forces it:
    right loss, that label's gradient 100 % wrong.  Utterance 0: class 1 has logit -400 at every frame and occurs three times in the
    transcript; utterance 1: class 1 is 25 nats down and is every second token of a 60-token transcript; utterance 2 is ordinary."""
    from voice100_amd import functional as F_
    g = torch.Generator().manual_seed(77)
    B, T, V, L = 3, 220, 29, 60
    logits = torch.randn(B, T, V, generator=g) * 2
    logits[0, :, 1] = -400.0
    logits[1, :, 1] -= 25.0
    targets = torch.randint(2, V, (B, L), generator=g)
    targets[0, 2] = 1; targets[0, 5] = 1; targets[0, 8] = 1
    targets[1, 0::2] = 1                                  # 1, x, 1, x, ... (x != 1: no repeated neighbours)
    in_len = torch.tensor([220, 200, 215], dtype=torch.int32)
    tgt_len = torch.tensor([10, 60, 33], dtype=torch.int32)
    ref_in = logits.double().clone().requires_grad_(True)
    ref = F.ctc_loss(F.log_softmax(ref_in.transpose(0, 1), dim=-1), targets, in_len, tgt_len, blank=0, reduction="mean", zero_infinity=True)
    ref.backward()
    x = logits.to(cuda).requires_grad_(True)
    loss = F_.ctc_loss(x, targets.to(cuda), in_len.to(cuda), tgt_len.to(cuda))
    loss.backward()
    assert torch.isfinite(loss) and abs(float(loss.detach()) - float(ref.detach())) < 1e-4 * abs(float(ref.detach()))
    gref = ref_in.grad.float()
    assert torch.isfinite(x.grad).all()
    for b in range(B):
        assert rel_err(x.grad[b], gref[b]) < 5e-3, b
    # the forced label's own gradient column (softmax ~ 0 minus an occupancy of up to 1) is what used to vanish
    assert float(gref[0, :, 1].abs().max()) > 1e-3 and rel_err(x.grad[0, :, 1], gref[0, :, 1]) < 5e-3


@pytest.mark.parametrize("B,C,T,K,S", [(5, 12, 130, 19, 1), (3, 8, 77, 83, 1), (2, 6, 40, 9, 1), (4, 10, 61, 11, 2), (2, 4, 600, 51, 1)])
def test_dwconv_bwd_fused_matches_split_and_torch(cuda, B, C, T, K, S):
    """v100_dwconv_bwd: the fused kernel (stride 1, specialised K), the two-pass fallback (other K / stride) and
    autograd of conv1d(relu6(bn(a1))) agree: dxin (through the ReLU6 mask), its BN-backward sums and dW."""
    N = _native()
    g = torch.Generator().manual_seed(K * 31 + T)
    pad = (K - 1) // 2
    Tout = (T + 2 * pad - K) // S + 1
    a1 = torch.randn(B, C, T, generator=g) * 2
    w = torch.randn(C, K, generator=g) * 0.2
    xa, xb = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    dz2, a2 = torch.randn(B, C, Tout, generator=g), torch.randn(B, C, Tout, generator=g)
    ga, gb, gc = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.randn(C, generator=g) * 0.1
    # reference: g' = BN-backward affine; xin = relu6(bn(a1)); y = dwconv(xin); loss = sum(y * g')
    gp = ga[None, :, None] * dz2 + gb[None, :, None] * a2 + gc[None, :, None]
    a1r, wr = a1.clone().requires_grad_(True), w.clone().requires_grad_(True)
    pre = a1r * xa[None, :, None] + xb[None, :, None]
    y = torch.nn.functional.conv1d(torch.clamp(pre, 0, 6), wr[:, None, :], stride=S, padding=pad, groups=C)
    (y * gp).sum().backward()
    dpre = a1r.grad / xa[None, :, None]                      # gradient w.r.t. the pre-activation = what the kernel stores
    dev = lambda t: t.to(cuda).contiguous()
    G = N.helper("v100_dw_num_groups", B, C)
    outs = []
    for force_split in (0, 1):
        dxin = torch.full((B, C, T), float("nan"), device=cuda)
        st, part, dw = torch.zeros(G, C, 2, device=cuda), torch.zeros(G, C, K, device=cuda), torch.zeros(C, K, device=cuda)
        N.call("v100_dwconv_bwd", dev(dz2), dev(a2), dev(w), dev(ga), dev(gb), dev(gc), dev(a1), dev(xa), dev(xb), dxin, st, part, dw,
               G, B, C, T, Tout, K, S, pad, force_split)
        outs.append((dxin.cpu(), st.sum(0).cpu(), dw.cpu()))
        assert rel_err(dxin, dpre.detach()) < TOL
        assert rel_err(dw, wr.grad) < TOL
        assert rel_err(st.sum(0)[:, 0], dpre.detach().sum((0, 2)), floor=1e-2) < 10 * TOL
        assert rel_err(st.sum(0)[:, 1], (dpre.detach() * a1).sum((0, 2)), floor=1e-2) < 10 * TOL
    assert rel_err(outs[0][0], outs[1][0]) < 1e-5 and rel_err(outs[0][2], outs[1][2]) < 1e-5


def test_tensors_past_the_2gib_descriptor_limit(cuda):
    """Maximum sizes: activations above 2 GiB do not fit one buffer descriptor, so the depthwise and GEMM launchers
    leave their buffer-addressed kernels for the 64-bit-indexed ones.  The big call must agree with the same entry point
    run on single utterances of it (which take the specialised kernels) and, on sampled rows, with torch fp32."""
    N = _native()
    g = torch.Generator().manual_seed(99)
    # depthwise forward (BN+ReLU6 prologue, raw + statistics): 9 x 2048 x 32768 fp32 = 2.25 GiB in, the same out
    B, C, T, K = 9, 2048, 32768, 19
    pad = (K - 1) // 2
    x = torch.randn(B, C, T, device=cuda)
    w = (torch.randn(C, K, generator=g) * 0.2).to(cuda)
    s, sh = (torch.rand(C, generator=g) + 0.5).to(cuda), torch.randn(C, generator=g).to(cuda)
    G = N.helper("v100_dw_num_groups", B, C)
    y = torch.empty(B, C, T, device=cuda)
    st = torch.zeros(G, C, 2, device=cuda)
    N.call("v100_dwconv", x, None, w, s, sh, None, 1, y, None, None, None, 0, st, G, B, C, T, T, K, 1, pad, 0, 1, 0)
    for b in (0, B - 1):
        y1 = torch.empty(1, C, T, device=cuda)
        st1 = torch.zeros(1, C, 2, device=cuda)
        N.call("v100_dwconv", x[b:b + 1], None, w, s, sh, None, 1, y1, None, None, None, 0, st1, 1, 1, C, T, T, K, 1, pad, 0, 1, 0)
        assert rel_err(y[b:b + 1], y1) < 1e-6
    rows = [(0, 0), (4, 1000), (B - 1, C - 1)]
    for b, c in rows:
        h = torch.clamp(x[b, c] * s[c] + sh[c], 0, 6).cpu()
        ref = F.conv1d(h[None, None], w[c].cpu()[None, None], padding=pad)[0, 0]
        assert rel_err(y[b, c], ref) < TOL
    assert rel_err(st.sum(0)[:, 0], y.sum((0, 2)), floor=1.0) < 1e-3
    del x, y, st, y1
    torch.cuda.empty_cache()
    # pointwise GEMM, bf16 operands, statistics epilogue: output 9 x 2048 x 32768 fp32 = 2.25 GiB
    B, M, Kc, T = 9, 2048, 64, 32768
    A = (torch.randn(M, Kc, generator=g) / Kc ** 0.5).to(cuda)
    Abf = A.to(torch.bfloat16)
    X = torch.randn(B, Kc, T, device=cuda)
    parts = N.helper("v100_pw_num_parts", B, T)
    Y = torch.empty(B, M, T, device=cuda)
    stp = torch.zeros(parts, M, 2, device=cuda)
    N.call("v100_pw_gemm", A, Abf, X, None, None, None, None, 0, Y, None, None, None, None, 1, stp, B, M, Kc, T, 1)
    for b in (0, B - 1):
        Y1 = torch.empty(1, M, T, device=cuda)
        st1 = torch.zeros(N.helper("v100_pw_num_parts", 1, T), M, 2, device=cuda)
        N.call("v100_pw_gemm", A, Abf, X[b:b + 1], None, None, None, None, 0, Y1, None, None, None, None, 1, st1, 1, M, Kc, T, 1)
        assert rel_err(Y[b:b + 1], Y1) < 1e-6
    ref = torch.einsum("mk,kt->mt", Abf.float().cpu(), X[B - 1].to(torch.bfloat16).float().cpu())
    assert rel_err(Y[B - 1], ref) < 1e-4
    assert rel_err(stp.sum(0)[:, 1], (Y * Y).sum((0, 2))) < 1e-3


@pytest.mark.parametrize("B,M,cx,T,shifts,lpad", [(2, 40, 64, 77, (0, 1, 2, 3, 4), 2), (3, 256, 192, 130, (2, 0, 1), 1), (1, 300, 128, 513, (5, 0, 3, 1, 7, 2, 6, 4), 4),
                                                   (2, 64, 24, 50, (1, 0), 1), (2, 129, 64, 1, (0, 1, 2), 1)])
@pytest.mark.parametrize("bf16", [0, 1])
def test_tap_addressed_gemm_and_wgrad(cuda, B, M, cx, T, shifts, lpad, bf16):
    """v100_pad_copy / v100_pw_gemm_taps / v100_pw_wgrad_taps against the explicit sum over taps in torch fp32: arbitrary
    (unsorted) shifts, channel counts that are odd multiples of 64 (bf16) or no multiple at all (fp32), M and T off the
    tile sizes, the +R epilogue, bias, and a padded, offset G operand."""
    import ctypes
    N = _native()
    ntap = len(shifts)
    g = torch.Generator().manual_seed(M * 3 + T)
    tx = (T + max(shifts) + 3) // 4 * 4 + 4
    if bf16 and not N.helper("v100_pw_taps_supported", B, M, cx, ntap, T, tx, 1):
        # bf16 operands need cx % 64 == 0; the entry point refuses loudly (callers then take the im2col path)
        assert cx % 64 != 0
        d = torch.zeros(1 << 16, device=cuda)
        with pytest.raises(RuntimeError):
            N.call("v100_pw_gemm_taps", d, d.to(torch.bfloat16), d, d, None, None, B, M, cx, T, tx, ntap, (ctypes.c_int * ntap)(*shifts), 1)
        return
    tol = 2e-2 if bf16 else TOL
    x = torch.randn(B, cx, T + 3, generator=g)                 # source rows longer than what is copied
    xp = torch.full((B * cx * tx + 64,), float("nan"), device=cuda)[:B * cx * tx].view(B, cx, tx)
    N.call("v100_pad_copy", x.to(cuda), xp, B, cx, T + 3, 1, 1, T, tx, lpad)
    ref_xp = torch.zeros(B, cx, tx)
    ref_xp[:, :, lpad:lpad + T] = x[:, :, 1:1 + T]
    assert torch.equal(xp.cpu(), ref_xp)
    A = torch.randn(M, ntap * cx, generator=g) / (ntap * cx) ** 0.5
    bias, R = torch.randn(M, generator=g), torch.randn(B, M, T, generator=g)
    Ad = A.to(cuda)
    Abf = Ad.to(torch.bfloat16) if bf16 else None
    sh = (ctypes.c_int * ntap)(*shifts)
    xv = torch.cat([ref_xp[:, :, s:s + T] for s in shifts], dim=1)           # the virtual [B, ntap*cx, T] operand
    ref = torch.einsum("mk,bkt->bmt", A, xv)
    Y = torch.full((B, M, T), float("nan"), device=cuda)
    N.call("v100_pw_gemm_taps", Ad, Abf, xp, Y, bias.to(cuda), None, B, M, cx, T, tx, ntap, sh, bf16)
    assert rel_err(Y, ref + bias[None, :, None]) < tol
    N.call("v100_pw_gemm_taps", Ad, Abf, xp, Y, None, R.to(cuda), B, M, cx, T, tx, ntap, sh, bf16)
    assert rel_err(Y, ref + R) < tol
    # backward-weight with G inside a padded buffer (pitch tg, first column g_off)
    G = torch.randn(B, M, T, generator=g)
    tg, g_off = T + 9, 5
    Gp = torch.full((B, M, tg), 7.0)
    Gp[:, :, g_off:g_off + T] = G
    S = N.helper("v100_pw_wgrad_splits", B, M, ntap * cx)
    partial = torch.empty(S, M, ntap * cx, device=cuda)
    dW = torch.empty(M, ntap * cx, device=cuda)
    N.call("v100_pw_wgrad_taps", Gp.to(cuda), tg, g_off, xp, partial, dW, S, B, M, cx, T, tx, ntap, sh, bf16)
    assert rel_err(dW, torch.einsum("bmt,bkt->mk", G, xv)) < tol


def test_dropout_fused(cuda):
    """nn.Dropout(0.2) as one kernel each way: kept elements scaled by 1/(1-p), dropped ones zero, keep rate ~ 1-p, the byte mask
    drives backward, a seed repeats and another seed differs."""
    from voice100_amd import functional as F_
    x = torch.randn(7, 96, 333, device=cuda)        # numel not a multiple of 4: tail path
    x = torch.where(x == 0, torch.ones_like(x), x)  # (randn yields an exact 0.0 about once in 2^24 samples: a kept zero would read as dropped)
    torch.manual_seed(11)
    xg = x.clone().requires_grad_(True)
    y = F_.dropout(xg, 0.2, True)
    kept = y != 0
    assert abs(float(kept.float().mean()) - 0.8) < 5e-3
    assert torch.allclose(y[kept], x[kept] / 0.8, rtol=1e-6)
    gy = torch.randn_like(y)
    y.backward(gy)
    assert torch.equal(xg.grad != 0, kept & (gy != 0))
    assert torch.allclose(xg.grad[kept], gy[kept] / 0.8, rtol=1e-6)
    torch.manual_seed(11)
    assert torch.equal(F_.dropout(x, 0.2, True), y.detach())
    assert not torch.equal(F_.dropout(x, 0.2, True), y.detach())
    assert F_.dropout(x, 0.2, False) is x
    # no visible structure along the fastest axis: neighbours are kept independently
    k = kept.float()
    assert abs(float((k[..., 1:] * k[..., :-1]).mean()) - 0.64) < 5e-3


def test_fused_adam_matches_torch(cuda):
    """FusedAdam (csrc/adam.hip) against torch.optim.Adam on the same parameters / gradients over several steps, with
    weight decay and a StepLR schedule (asr.py:169-176); state_dict round trip continues the same trajectory."""
    from voice100_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(3)
    shapes = [(512, 64, 1), (512,), (2048, 1, 83), (29, 512, 1), (3,), (70001,)]
    pa = [torch.nn.Parameter(torch.randn(s, generator=g).to(cuda)) for s in shapes]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    oa = FusedAdam(pa, lr=1e-3, weight_decay=4e-5)
    ob = torch.optim.Adam(pb, lr=1e-3, weight_decay=4e-5)
    sa, sb = torch.optim.lr_scheduler.StepLR(oa, 1, 0.98), torch.optim.lr_scheduler.StepLR(ob, 1, 0.98)
    for step in range(6):
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, generator=g).to(cuda) * (10.0 ** (step - 3))
            a.grad, b.grad = gr.clone(), gr.clone()
        oa.step(); ob.step()
        if step % 2:
            sa.step(); sb.step()
        if step == 3:                                   # resume from a checkpoint of the optimizer
            sd = oa.state_dict()
            oa = FusedAdam(pa, lr=1e-3, weight_decay=4e-5)
            oa.load_state_dict(sd)
            sa.optimizer = oa                           # the schedule goes on with the restored optimizer
    for a, b in zip(pa, pb):
        assert rel_err(a, b) < 2e-6, (a.shape, rel_err(a, b))
    for a, b in zip(pa, pb):
        assert rel_err(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) < 1e-5
        assert rel_err(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]) < 1e-5


@pytest.mark.parametrize("B,cin,cout,T,prec", [(3, 64, 29, 52, "fp32"), (2, 512, 29, 128, "bf16"), (4, 96, 32, 260, "bf16"),
                                               (2, 64, 29, 51, "fp32"), (2, 48, 29, 64, "bf16"), (2, 128, 40, 64, "fp32")])
def test_dropout_pointwise_node_equals_the_pair(cuda, B, cin, cout, T, prec):
    """Dropout -> Conv1d(k=1) as one autograd node (LinearCharDecoder's training forward) against the two separate nodes on the same
    seed: output, data gradient (keep mask applied in the small-K GEMM's epilogue where that kernel applies: the first three shapes;
    the others take the two-kernel route), weight and bias gradients -- all bit for bit."""
    from voice100_amd import functional as F_
    g = torch.Generator().manual_seed(B * 1000 + T)
    x = torch.randn(B, cin, T, generator=g).to(cuda)
    w = (torch.randn(cout, cin, 1, generator=g) * 0.1).to(cuda)
    b = torch.randn(cout, generator=g).to(cuda)
    gy = torch.randn(B, cout, T, generator=g).to(cuda)
    res = []
    for fused in (True, False):
        xi, wi, bi = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        torch.manual_seed(77)
        if fused:
            y = F_.dropout_pointwise_conv1d(xi, wi, bi, 0.2, precision=prec)
        else:
            y = F_.pointwise_conv1d(F_.dropout(xi, 0.2, True), wi, bi, precision=prec)
        y.backward(gy)
        res.append((y.detach(), xi.grad, wi.grad, bi.grad))
    for a, c in zip(*res):
        assert torch.equal(a, c)
    assert 0.7 < float((res[0][1] != 0).float().mean()) < 0.9


def test_ctc_gradient_in_the_transposed_layout(cuda):
    """Logits that are transpose_last2() of a [B, V, T] tensor (asr.py:114): ctc_loss writes its gradient in THAT layout and the
    transpose's backward hands the buffer on without a launch; same values as the plain route, with the unit root gradient and with
    a scaled one, ragged lengths, an infeasible and an empty utterance."""
    from voice100_amd import functional as F_
    import voice100_amd._native as N
    g = torch.Generator().manual_seed(9)
    B, V, T, L = 5, 29, 70, 12
    src = (torch.randn(B, V, T, generator=g) * 2).to(cuda)
    tgt = torch.randint(1, V, (B, L), generator=g).to(cuda)
    il = torch.tensor([70, 5, 33, 70, 41], dtype=torch.int32, device=cuda)
    tl = torch.tensor([12, 9, 0, 7, 12], dtype=torch.int32, device=cuda)        # utterance 1: too short (zero_infinity); 2: empty target
    a = src.clone().requires_grad_(True)
    loss_a = F_.ctc_loss(a.transpose(1, 2).contiguous(), tgt, il, tl)            # plain route: torch's transpose, [B, T, V] gradient
    loss_a.backward()
    for scale in (None, 2.5):
        b = src.clone().requires_grad_(True)
        logits = F_.transpose_last2(b)
        assert getattr(logits, "_v100_grad_T", False)
        loss_b = F_.ctc_loss(logits, tgt, il, tl)
        n0 = N.launch_count()
        if scale is None:
            loss_b.backward(F_.unit_grad(loss_b))
            assert N.launch_count() == n0                                         # gradient computed with the loss; no transpose launch
            assert torch.equal(loss_a.detach(), loss_b.detach()) and torch.equal(a.grad, b.grad)
        else:
            loss_b.backward(torch.full((), scale, device=cuda))
            assert N.launch_count() == n0
            assert torch.allclose(b.grad, a.grad * scale, rtol=1e-6, atol=0)
        assert b.grad.is_contiguous()
    c = src.clone().requires_grad_(True)                                          # a consumer in between: the tag does not travel
    mid = F_.transpose_last2(c) * 1.0
    assert not getattr(mid, "_v100_grad_T", False)
    F_.ctc_loss(mid, tgt, il, tl).backward()
    assert torch.equal(c.grad, a.grad)
