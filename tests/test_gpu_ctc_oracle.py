"""The CTC head (K10, csrc/ctc.hip) per utterance and element by element against the float64 reference of tests/_ctc_cases.py, over
every launch regime of ctc_run: the skew pipeline with 1, 2, 4 and 16 waves, ctc_lattice_kernel<8> and <16> with every slot live, the
launch above 64 KiB of LDS, and both gradient layouts.  test_ctc_cases_cpu.py checks that the cases reach all that.

Bars.  nll_b: 1e-4 * max(1, |nll64_b|), the project's loss bar, per utterance.  Gradient (entries in [-1, 1]), per utterance:
max |G[b] - G64[b]| <= max(2e-4, 2 e32_b, sqrt(in_len_b) * max(1, |nll64_b|) * 2^-24), all three from the reference: 2e-4 is the bar of
the short cases in test_gpu_kernels.py, e32_b is the error of torch's own float32 lattice on the CPU (a log-domain recursion of the
same length), the last term a random walk of in_len roundings of values of size |nll|.  tools/micro/ctc_acc.py had measured the
kernels at 0.55 - 0.65 of torch's float32 error in relative L2 over a batch; the max-abs ratio per utterance was first measured with
these cases (tools/micro/ctc_acc.py --cases, profiles/ctc_oracle_errors.json): 0.33 - 4.1 x e32, median 1.0 x; the largest err / bar
is 0.79 for the pipeline (flat[2]), 0.50 for <8> (edge_1023[1]) and 0.56 for <16> (max_2046_v128[1])."""
import numpy as np
import pytest
import torch

import _ctc_cases as C
from voice100_amd import _native as N
from voice100_amd import functional as F_

pytestmark = pytest.mark.gpu

PAD = 64                      # sentinel elements on either side of the workspace, nll and grad
SENTINEL = -77.0
cases = pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)


def bits(t):
    return t.contiguous().view(torch.int32)


def _lengths(dev, case):
    return (torch.tensor(case.in_len, dtype=torch.int32, device=dev), torch.tensor(case.tgt_len, dtype=torch.int32, device=dev))


def run_raw(dev, case, fill):
    """One v100_ctc_loss call on views inside sentinel margins, the workspace pre-filled with `fill`: (nll [B], unscaled gradient
    [B, T, V]) on the CPU.  The margins are checked here."""
    logits, labels = C.inputs(case)
    B, T, V, L = case.B, case.T, case.V, case.Lmax
    nws = int(N.helper("v100_ctc_workspace_floats", B, T, L))
    assert nws == C.workspace_floats(case)
    bufs = {"workspace": torch.full((nws + 2 * PAD,), fill, dtype=torch.float32, device=dev),
            "nll": torch.full((B + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev),
            "grad": torch.full((B * T * V + 2 * PAD,), SENTINEL, dtype=torch.float32, device=dev)}
    bufs["workspace"][:PAD] = SENTINEL
    bufs["workspace"][PAD + nws:] = SENTINEL
    view = {k: v[PAD:v.numel() - PAD] for k, v in bufs.items()}
    il, tl = _lengths(dev, case)
    before = N.launch_count()
    N.call("v100_ctc_loss", logits.to(dev), labels.to(dev), il, tl, view["workspace"], view["nll"], view["grad"], B, T, V, L, case.blank)
    assert N.launch_count() - before == 3                 # lse, lattice, gradient
    torch.cuda.synchronize()
    for k, v in bufs.items():
        assert bool((v[:PAD] == SENTINEL).all()) and bool((v[v.numel() - PAD:] == SENTINEL).all()), k
    return view["nll"].cpu(), view["grad"].view(B, T, V).cpu()


_RAW = {}


def raw(dev, case):
    """The call of (a), workspace pre-filled with NaN; shared by the tests of one case."""
    if case.name not in _RAW:
        _RAW[case.name] = run_raw(dev, case, float("nan"))
    return _RAW[case.name]


def product(dev, case, transposed):
    """functional.ctc_loss (reduction 'mean') and the gradient it leaves on its input, as [B, T, V] on the CPU."""
    logits, labels = C.inputs(case)
    il, tl = _lengths(dev, case)
    if transposed:
        src = logits.transpose(1, 2).contiguous().to(dev).requires_grad_(True)      # [B, V, T], as the encoder hands it over
        x = F_.transpose_last2(src)
        assert getattr(x, "_v100_grad_T", False)
    else:
        src = x = logits.to(dev).requires_grad_(True)
    loss = F_.ctc_loss(x, labels.to(dev), il, tl, blank=case.blank)
    loss.backward()
    grad = src.grad
    if transposed:
        assert grad.shape == (case.B, case.V, case.T) and grad.is_contiguous()
        grad = grad.transpose(1, 2)
    return loss.detach().cpu(), grad.cpu().contiguous()


_PRODUCT = {}


def plain_product(dev, case):
    if case.name not in _PRODUCT:
        _PRODUCT[case.name] = product(dev, case, False)
    return _PRODUCT[case.name]


@cases
def test_per_utterance_against_float64(cuda, case):
    ref = C.reference(case)
    nll, G = raw(cuda, case)
    nll, G = nll.double(), G.double()
    bar = C.grad_bar(case, ref)
    assert bool(torch.isfinite(G).all())
    for b in range(case.B):
        want = float(ref.nll64[b])
        err = float((G[b] - ref.G64[b]).abs().max())
        print(f"{case.name}[{b}] nll {float(nll[b]):.6g} (ref {want:.6g})  grad err {err:.3e}  e32 {float(ref.e32[b]):.3e}  "
              f"bar {float(bar[b]):.3e}  ratio {err / float(bar[b]):.3f}")
    for b in range(case.B):
        want = float(ref.nll64[b])
        if want == float("inf"):
            assert float(nll[b]) == float("inf"), b
            assert not bool(bits(G[b].float()).any()), b                  # exactly +0
            continue
        assert abs(float(nll[b]) - want) <= 1e-4 * max(1.0, abs(want)), (b, float(nll[b]), want)
        assert float((G[b] - ref.G64[b]).abs().max()) <= float(bar[b]), b
        assert not bool(G[b, case.in_len[b]:].any()), b                   # padded frames


@cases
def test_product_entry_point(cuda, case):
    """functional.ctc_loss: the 'mean' loss against float64, and its gradient against the unscaled one of v100_ctc_loss -- only the
    factor 1 / (B * max(tgt_len, 1)), applied in float32 inside the gradient kernel, separates the two: 2 ulps."""
    ref = C.reference(case)
    _, G = raw(cuda, case)
    loss, grad = plain_product(cuda, case)
    assert abs(float(loss) - ref.mean64) <= 1e-4 * max(1.0, abs(ref.mean64)), (float(loss), ref.mean64)
    denom = torch.tensor([case.B * max(n, 1) for n in case.tgt_len], dtype=torch.float64).view(-1, 1, 1)
    want = (G.double() / denom).numpy()
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    excess = np.abs(grad.double().numpy() - want) / ulp
    print(f"{case.name}: loss {float(loss):.6g} (ref {ref.mean64:.6g}), largest distance {excess.max():.2f} ulp")
    assert excess.max() <= 2.0


@cases
def test_transposed_layout_is_the_same_bits(cuda, case):
    """The logits as transpose_last2() of a [B, V, T] tensor: the gradient is written as [B, V, T] by ctc_grad_kernel<16, true>."""
    loss, grad = plain_product(cuda, case)
    loss_t, grad_t = product(cuda, case, True)
    assert torch.equal(bits(loss.view(1)), bits(loss_t.view(1)))
    assert torch.equal(bits(grad), bits(grad_t))


@cases
def test_workspace_is_written_before_it_is_read(cuda, case):
    """Whatever the workspace held before the call (NaN, zeros) changes no bit of the outputs; nothing is written beside it."""
    nll, G = raw(cuda, case)
    nll0, G0 = run_raw(cuda, case, 0.0)
    assert torch.equal(bits(nll), bits(nll0)) and torch.equal(bits(G), bits(G0))


@cases
def test_same_bits_twice(cuda, case):
    """The skew kernel takes its speculative fetch or its spin by timing: both must give the same bits."""
    nll, G = raw(cuda, case)
    nll2, G2 = run_raw(cuda, case, float("nan"))
    assert torch.equal(bits(nll), bits(nll2)) and torch.equal(bits(G), bits(G2))


def test_limits_are_loud(cuda):
    """Past the kernels' limits the call raises and launches nothing."""
    def refuses(B, T, V, L, blank=0, match=None):
        x = torch.zeros(B, T, V, device=cuda)
        labels = torch.ones(B, L, dtype=torch.int64, device=cuda)
        il = torch.full((B,), T, dtype=torch.int32, device=cuda)
        tl = torch.ones(B, dtype=torch.int32, device=cuda)
        before = N.launch_count()
        with pytest.raises(RuntimeError, match=match):
            F_.ctc_loss(x, labels, il, tl, blank=blank)
        small = torch.zeros(64, device=cuda)
        with pytest.raises(RuntimeError, match="status 1"):
            N.call("v100_ctc_loss", x, labels, il, tl, small, small, small, B, T, V, L, blank)      # refused before anything is touched
        assert N.launch_count() == before

    refuses(1, 4, 29, 2048, match="2047")
    refuses(1, 4, 129, 2)
    refuses(1, 4, 29, 2, blank=29)
    refuses(1, 4, 29, 2, blank=-1)
    # a workspace of 2^31 floats or more: B * T * (2 * 2 * 2047 + 2 + 1) + B floats, i.e. B * 8191 * T + B at Lmax 2047
    B, T, Lmax = 32, 8193, 2047
    assert B * T * 8191 + B >= 2 ** 31 > B * (T - 1) * 8191 + B
    assert N.helper("v100_ctc_workspace_floats", B, T, Lmax) == -1
    assert N.helper("v100_ctc_workspace_floats", B, T - 1, Lmax) == B * (T - 1) * 8191 + B          # the largest that is granted
    x = torch.zeros(B, T, 2, device=cuda)
    before = N.launch_count()
    with pytest.raises(RuntimeError, match="workspace"):
        F_.ctc_loss(x, torch.ones(B, Lmax, dtype=torch.int64, device=cuda), torch.full((B,), T, dtype=torch.int32, device=cuda),
                    torch.ones(B, dtype=torch.int32, device=cuda))
    assert N.launch_count() == before
