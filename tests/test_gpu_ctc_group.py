"""The two hand-over forms of the CTC wave pipeline (csrc/ctc.hip: edge states handed between neighbouring waves once per frame, or
once per group of frames) BIT FOR BIT against each other, forced with the hook v100_ctc_lattice_form, through v100_ctc_loss_mean_t in
both gradient layouts: the whole workspace (alpha, beta, lse, stall flags; NaN-filled first, so a cell one form leaves unwritten
shows), nll, the loss and the gradient.  The per-frame form is the one tests/test_gpu_ctc_oracle.py pins against float64 wherever the
host rule picks it; here both forms also meet the float64 loss of tests/_ctc_cases.py per utterance at that file's bar, 1e-4 * max(1,
|nll|).  Cases: tests/_ctc_group_cases.py (what they reach: test_ctc_group_cpu.py)."""
import pytest
import torch

import _ctc_cases as C
import _ctc_group_cases as G
from voice100_amd import _native as N

pytestmark = pytest.mark.gpu

PER_FRAME, GROUPED, RULE = 0, 1, -1


def bits(t):
    return t.contiguous().view(torch.int32)


def run(dev, case, form, bvt):
    """One v100_ctc_loss_mean_t call with the hand-over forced to `form`: workspace, nll, loss, grad as CPU tensors."""
    logits, labels = C.inputs(case)
    B, T, V, L = case.B, case.T, case.V, case.Lmax
    ws = torch.full((int(N.helper("v100_ctc_workspace_floats", B, T, L)),), float("nan"), dtype=torch.float32, device=dev)
    nll = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float32, device=dev)
    grad = torch.full((B * T * V,), float("nan"), dtype=torch.float32, device=dev)
    il = torch.tensor(case.in_len, dtype=torch.int32, device=dev)
    tl = torch.tensor(case.tgt_len, dtype=torch.int32, device=dev)
    N.call("v100_ctc_lattice_form", form)
    try:
        before = N.launch_count()
        N.call("v100_ctc_loss_mean_t", logits.to(dev), labels.to(dev), il, tl, ws, nll, loss, grad, bvt, B, T, V, L, case.blank)
        assert N.launch_count() - before == 3                 # lse, lattice, gradient
        torch.cuda.synchronize()
    finally:
        N.call("v100_ctc_lattice_form", RULE)
    return ws.cpu(), nll.cpu(), loss.cpu(), grad.cpu()


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c.name)
def test_forms_agree_bit_for_bit(cuda, case):
    ref = C.reference(case)
    for bvt in (0, 1):
        ws0, nll0, loss0, grad0 = run(cuda, case, PER_FRAME, bvt)
        ws1, nll1, loss1, grad1 = run(cuda, case, GROUPED, bvt)
        n = case.B * case.T * (2 * case.Lmax + 1)
        for name, lo, hi in (("alpha", 0, n), ("beta", n, 2 * n), ("lse", 2 * n, 2 * n + case.B * case.T)):
            assert torch.equal(bits(ws0[lo:hi]), bits(ws1[lo:hi])), (name, bvt)
        stall = bits(ws0[2 * n + case.B * case.T:])
        assert stall.numel() == case.B and not bool(stall.any()) and not bool(bits(ws1[2 * n + case.B * case.T:]).any())
        assert torch.equal(bits(nll0), bits(nll1)), bvt
        assert torch.equal(bits(loss0), bits(loss1)), bvt
        assert torch.equal(bits(grad0), bits(grad1)), bvt
        assert bool(torch.isfinite(grad1).all()) and bool(torch.isfinite(loss1).all())
        # and they are the right bits: every utterance's loss against float64
        for b in range(case.B):
            want = float(ref.nll64[b])
            if want == float("inf"):
                assert float(nll1[b]) == float("inf"), b
            else:
                assert abs(float(nll1[b]) - want) <= 1e-4 * max(1.0, abs(want)), (b, float(nll1[b]), want)
        assert abs(float(loss1) - ref.mean64) <= 1e-4 * max(1.0, abs(ref.mean64))


def test_the_rule_runs_the_form_it_names(cuda):
    """Unforced, ctc_run gives the same bits again (either form does), and the hook refuses what it does not know."""
    case = G.RING_WRAP
    want = run(cuda, case, GROUPED, 1)
    got = run(cuda, case, RULE, 1)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(want, got))
    with pytest.raises(RuntimeError, match="status 1"):
        N.call("v100_ctc_lattice_form", 2)
