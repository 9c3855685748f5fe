"""Gradient clipping on the GPU (csrc/adam.hip): the stand-alone clip_grad_norm_ / clip_grad_value_ and the clip fused into the Adam
launch, against torch.nn.utils and torch.optim.Adam; NaN / inf behaviour, run-to-run determinism, no host synchronisation, the product
TrainStep and the world-2 step with clipping."""
import math
import os
import random

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(512, 64, 1), (512,), (2048, 1, 83), (29, 512, 1), (3,), (29,), (70001,)]


def _params(cuda, seed, misaligned=True):
    """Parameters of the odd shapes of test_fused_adam_matches_torch, gradients scaled to ~1; the last gradient is a view at a 4-byte offset
    into a larger buffer (off the 16-byte accesses)."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(cuda)) for s in SHAPES]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).to(cuda)
    if misaligned:
        n = ps[-1].numel()
        big = torch.randn(n + 5, generator=g).to(cuda)
        ps[-1].grad = big[1:1 + n].view(ps[-1].shape)
        assert ps[-1].grad.data_ptr() % 16 == 4
    return ps


def _total_fp64(grads, norm_type):
    flat = torch.cat([g.detach().reshape(-1).double().cpu() for g in grads])
    return float(flat.abs().max()) if math.isinf(norm_type) else float(flat.norm())


@pytest.mark.parametrize("norm_type", [2.0, math.inf])
@pytest.mark.parametrize("ratio", [0.5, 2.0])
def test_clip_grad_norm_matches_torch(cuda, norm_type, ratio):
    from voice100_amd.optim import clip_grad_norm_
    pa, pb = _params(cuda, 1), _params(cuda, 1)
    orig = [p.grad.detach().cpu().clone() for p in pa]
    want = _total_fp64([p.grad for p in pa], norm_type)
    max_norm = ratio * want                                  # 0.5: the clip engages; 2.0: coefficient 1
    got = clip_grad_norm_(pa, max_norm, norm_type)
    ref = torch.nn.utils.clip_grad_norm_(pb, max_norm, norm_type)
    assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float32
    assert abs(float(got) - want) <= 1e-6 * want
    # every workgroup scaled by the same coefficient: torch's formula on the returned total, evaluated on the CPU in IEEE fp32
    coef = torch.clamp(max_norm / (got.cpu() + 1e-6), max=1.0)
    for a, b, o in zip(pa, pb, orig):
        assert torch.equal(a.grad.cpu(), o * coef)
        assert rel_err(a.grad, b.grad) < 1e-6
        if ratio > 1:
            assert torch.equal(a.grad.cpu(), o)


def test_clip_grad_value_matches_torch(cuda):
    from voice100_amd.optim import clip_grad_value_
    pa, pb = _params(cuda, 2), _params(cuda, 2)
    assert clip_grad_value_(pa, 0.7) is None
    torch.nn.utils.clip_grad_value_(pb, 0.7)
    for a, b in zip(pa, pb):
        assert torch.equal(a.grad, b.grad)
    assert float(max(p.grad.abs().max() for p in pa)) == pytest.approx(0.7)


def _adam_pair(cuda, seed, **clip):
    """FusedAdam stepping with the clip fused in, and torch's clip + torch.optim.Adam, over 6 steps with gradient scales 1e-3 .. 1e2, weight
    decay, StepLR and two param groups (the norm spans both).  Returns both parameter lists, both optimizers and the norms of each step."""
    from voice100_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(seed)
    pa = [torch.nn.Parameter(torch.randn(s, generator=g).to(cuda)) for s in SHAPES]
    pb = [torch.nn.Parameter(p.detach().clone()) for p in pa]
    groups = lambda ps: [{"params": ps[:3]}, {"params": ps[3:], "lr": 3e-3}]
    oa = FusedAdam(groups(pa), lr=1e-3, weight_decay=4e-5)
    ob = torch.optim.Adam(groups(pb), lr=1e-3, weight_decay=4e-5)
    sa, sb = torch.optim.lr_scheduler.StepLR(oa, 1, 0.98), torch.optim.lr_scheduler.StepLR(ob, 1, 0.98)
    norms, grads = [], []
    for step in range(6):
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, generator=g).to(cuda) * (10.0 ** (step - 3))
            a.grad, b.grad = gr.clone(), gr.clone()
        if "max_grad_norm" in clip:
            ref = torch.nn.utils.clip_grad_norm_(pb, clip["max_grad_norm"])
        else:
            ref = torch.nn.utils.clip_grad_value_(pb, clip["grad_clip_value"])
        oa.step(**clip)
        ob.step()
        norms.append((oa.last_grad_norm, ref))
        grads.append([rel_err(a.grad, b.grad) for a, b in zip(pa, pb)])
        if step % 2:
            sa.step(); sb.step()
    return pa, pb, oa, ob, norms, grads


@pytest.mark.parametrize("clip", [{"max_grad_norm": 10.0}, {"grad_clip_value": 0.05}])
def test_fused_adam_clip_matches_torch(cuda, clip):
    pa, pb, oa, ob, norms, grads = _adam_pair(cuda, 3, **clip)
    for a, b in zip(pa, pb):
        assert rel_err(a, b) < 2e-6, (a.shape, rel_err(a, b))
        assert rel_err(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"]) < 1e-5
        assert rel_err(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"]) < 1e-5
    assert max(max(e) for e in grads) < 1e-6                # p.grad after each step is torch's clipped gradient
    if "max_grad_norm" in clip:
        engaged = [float(ref) > clip["max_grad_norm"] for _, ref in norms]
        assert any(engaged) and not all(engaged)
        for got, ref in norms:
            assert got.is_cuda and abs(float(got) - float(ref)) <= 1e-5 * float(ref)
    else:
        assert all(got is None for got, _ in norms)


def test_fused_clip_and_standalone_clip_agree_bitwise(cuda):
    """The coefficient is formed inside each consuming launch: the clipped Adam step and the stand-alone clip must scale identically."""
    from voice100_amd.optim import FusedAdam, clip_grad_norm_
    pa, pb = _params(cuda, 4, misaligned=False), _params(cuda, 4, misaligned=False)
    oa = FusedAdam(pa, lr=1e-3)
    oa.step(max_grad_norm=1.0)
    nb = clip_grad_norm_(pb, 1.0)
    assert torch.equal(oa.last_grad_norm, nb)
    for a, b in zip(pa, pb):
        assert torch.equal(a.grad, b.grad)


def test_coefficient_one_is_a_noop(cuda):
    from voice100_amd.optim import FusedAdam
    pa, pb = _params(cuda, 5, misaligned=False), _params(cuda, 5, misaligned=False)
    orig = [p.grad.clone() for p in pa]
    oa, ob = FusedAdam(pa, lr=1e-3, weight_decay=1e-4), FusedAdam(pb, lr=1e-3, weight_decay=1e-4)
    for _ in range(3):
        oa.step(max_grad_norm=1e30)
        ob.step()
    for a, b, o in zip(pa, pb, orig):
        assert torch.equal(a, b) and torch.equal(a.grad, o)
        assert torch.equal(oa.state[a]["exp_avg"], ob.state[b]["exp_avg"])
        assert torch.equal(oa.state[a]["exp_avg_sq"], ob.state[b]["exp_avg_sq"])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
@pytest.mark.parametrize("clip", [{"max_grad_norm": 1.0}, {"max_grad_norm": 1.0, "norm_type": math.inf}, {"grad_clip_value": 0.1}])
def test_nonfinite_gradients_follow_torch(cuda, bad, clip):
    from voice100_amd.optim import FusedAdam
    pa, pb = _params(cuda, 6, misaligned=False), _params(cuda, 6, misaligned=False)
    for ps in (pa, pb):
        ps[2].grad.view(-1)[12345] = bad
    oa, ob = FusedAdam(pa, lr=1e-3, weight_decay=1e-4), torch.optim.Adam(pb, lr=1e-3, weight_decay=1e-4)
    oa.step(**clip)
    if "max_grad_norm" in clip:
        torch.nn.utils.clip_grad_norm_(pb, clip["max_grad_norm"], clip.get("norm_type", 2.0))
    else:
        torch.nn.utils.clip_grad_value_(pb, clip["grad_clip_value"])
    ob.step()
    for a, b in zip(pa, pb):
        for f in (torch.isnan, torch.isinf, lambda x: x == 0):
            assert torch.equal(f(a), f(b))
            assert torch.equal(f(a.grad), f(b.grad))


def test_clip_is_deterministic(cuda):
    from voice100_amd.optim import FusedAdam, clip_grad_norm_

    def run():
        g = torch.Generator().manual_seed(8)
        ps = [torch.nn.Parameter(torch.randn(n, generator=g).to(cuda)) for n in (3_000_000, 2_000_001, 29, 512 * 512)]
        opt = FusedAdam(ps, lr=1e-3)
        norms = []
        for i in range(3):
            for p in ps:
                p.grad = torch.randn(p.shape, generator=g).to(cuda) * 10
            opt.step(max_grad_norm=100.0)
            norms.append(opt.last_grad_norm.clone())
            for p in ps:
                p.grad = torch.randn(p.shape, generator=g).to(cuda)
            norms.append(clip_grad_norm_(ps, 100.0))
        return [p.detach().clone() for p in ps], norms

    (pa, na), (pb, nb) = run(), run()
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
    assert all(torch.equal(a, b) for a, b in zip(na, nb))


def test_clipped_paths_do_not_synchronise(cuda):
    from voice100_amd.optim import FusedAdam, clip_grad_norm_, clip_grad_value_
    pa, pb = _params(cuda, 9, misaligned=False), _params(cuda, 9)
    opt = FusedAdam(pa, lr=1e-3)
    src = [p.grad.clone() for p in pa]
    opt.step(max_grad_norm=1.0); opt.step(grad_clip_value=0.1)      # warm-up: tables built, gradient pointers uploaded
    clip_grad_norm_(pb, 1.0); clip_grad_value_(pb, 0.5)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(2):
            for p, s in zip(pa, src):
                p.grad.copy_(s)                                    # same gradient tensors: nothing to re-upload
            opt.step(max_grad_norm=1.0)
            opt.step(grad_clip_value=0.1)
            clip_grad_norm_(pb, 1.0)
            clip_grad_value_(pb, 0.5)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


@pytest.mark.parametrize("clip", [1.0, 0.01])
def test_product_trainstep_with_clipping_matches_torch_clip(cuda, clip):
    """AudioToTextCTC at a small width, fp32: TrainStep(gradient_clip_val) against the same model driven as backward ->
    torch.nn.utils.clip_grad_norm_ -> optimizer.step() under the same seeds (dropout, augmentation)."""
    from voice100_amd import functional as F_
    from voice100_amd.asr import AudioToTextCTC
    from voice100_amd.trainer import TrainStep
    dims = (64, 32, 29, 32)
    torch.manual_seed(11)
    ma = AudioToTextCTC(*dims).to(cuda)
    mb = AudioToTextCTC(*dims).to(cuda)
    mb.load_state_dict(ma.state_dict())
    g = torch.Generator().manual_seed(12)
    B, T, L = 4, 96, 10
    audio = (torch.randn(B, T, 64, generator=g) * 2 - 4).to(cuda)
    alen = torch.randint(T // 2, T + 1, (B,), generator=g).to(torch.int32).to(cuda)
    text = torch.randint(1, 29, (B, L), generator=g).to(cuda)
    tlen = torch.randint(L // 2, L + 1, (B,), generator=g).to(torch.int32).to(cuda)
    batch = ((audio, alen), (text, tlen))
    try:
        step = TrainStep(ma, precision=32, gradient_clip_val=clip)
        opt_b = mb.configure_optimizers()["optimizer"]
        mb.train()
        got, ref = [], []
        for i in range(3):
            random.seed(7 + i); torch.manual_seed(7 + i)
            step(batch)
            got.append(float(step.last_grad_norm))
            random.seed(7 + i); torch.manual_seed(7 + i)
            for p in mb.parameters():
                p.grad = None
            mb.training_step(batch, i).backward()
            ref.append(float(torch.nn.utils.clip_grad_norm_(list(mb.parameters()), clip)))
            opt_b.step()
    finally:
        F_.set_matmul_precision("fp32")
    for a, b in zip(ma.parameters(), mb.parameters()):
        assert rel_err(a, b) < 1e-5
    for a, b in zip(got, ref):
        assert abs(a - b) <= 1e-5 * b
    if clip < 1:
        assert all(r > clip for r in ref)                  # engaged on every step


def test_clipped_product_step_world2_on_one_gpu(cuda, tmp_path):
    """Two ranks on the one GPU (as tests/test_gpu_dist2.py): with gradient_clip_val=1.0 the replicas stay bit-identical, both report the
    same norm, and that norm is the norm of the gradient MEAN."""
    from voice100_amd.trainer import launch_ranks
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gradclip_gpu_worker.py")
    assert launch_ranks(worker, [str(tmp_path)], 2, timeout=600) == 0
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    assert torch.equal(r0["weights"], r1["weights"])
    assert r0["norms"] == r1["norms"]
    for got, want, local in zip(r0["norms"], r0["want"], r0["local"]):
        assert abs(got - want) <= 1e-5 * want
        assert abs(local - want) > 1e-3 * want              # the mean's norm, not the rank's own gradient's
