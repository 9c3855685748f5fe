"""Gradient clipping in TrainStep on the CPU (Lightning's trainer.gradient_clip_val / gradient_clip_algorithm, which every training recipe
of the reference sets): the step must be backward -> torch.nn.utils.clip_grad_norm_ (or clip_grad_value_) over all the optimizer's
parameters -> optimizer.step(), bit for bit, and with two ranks the clip must see the gradient MEAN (Lightning clips after DDP's
all-reduce), so that the replicas stay identical."""
import os

import pytest
import torch

from _dist_worker import Toy
from voice100_amd.trainer import TrainStep


def _batch():
    g = torch.Generator().manual_seed(7)
    return torch.randn(6, 4, 20, generator=g) * 10, torch.randn(6, 2, 20, generator=g)


def _hand_loop(clip, algorithm, steps=3):
    torch.manual_seed(5)
    model = Toy(hidden=8, learning_rate=1e-2)
    cfg = model.configure_optimizers()
    opt = cfg["optimizer"]
    batch, norms = _batch(), []
    for i in range(steps):
        for p in model.parameters():
            p.grad = None
        model.training_step(batch, i).backward()
        if algorithm == "norm":
            norms.append(torch.nn.utils.clip_grad_norm_([p for g in opt.param_groups for p in g["params"]], clip))
        else:
            torch.nn.utils.clip_grad_value_([p for g in opt.param_groups for p in g["params"]], clip)
        opt.step()
    return model, norms


def _trainstep(clip, algorithm, steps=3):
    torch.manual_seed(5)
    model = Toy(hidden=8, learning_rate=1e-2)
    step = TrainStep(model, gradient_clip_val=clip, gradient_clip_algorithm=algorithm)
    batch, norms = _batch(), []
    for _ in range(steps):
        step(batch)
        norms.append(step.last_grad_norm)
    return model, norms


@pytest.mark.parametrize("clip,algorithm,engages", [(0.05, "norm", True), (1e6, "norm", False), (0.01, "value", True)])
def test_clipped_trainstep_matches_the_hand_written_loop(clip, algorithm, engages):
    got, got_norms = _trainstep(clip, algorithm)
    ref, ref_norms = _hand_loop(clip, algorithm)
    for a, b in zip(got.parameters(), ref.parameters()):
        assert torch.equal(a, b)
        assert torch.equal(a.grad, b.grad)                 # p.grad holds the clipped gradient afterwards
    if algorithm == "norm":
        assert all(torch.equal(a, b) for a, b in zip(got_norms, ref_norms))
        assert (float(ref_norms[0]) > clip) == engages
    else:
        assert got_norms == [None] * 3
        assert float(max(p.grad.abs().max() for p in got.parameters())) == pytest.approx(0.01)
    unclipped, _ = _trainstep(None, "norm")                 # and the clip really changed the trajectory (or really did not)
    same = all(torch.equal(a, b) for a, b in zip(got.parameters(), unclipped.parameters()))
    assert same != engages


def test_clip_disabled_by_none_and_zero():
    a, na = _trainstep(None, "norm")
    b, nb = _trainstep(0, "value")
    for x, y in zip(a.parameters(), b.parameters()):
        assert torch.equal(x, y)
    assert na == nb == [None] * 3


@pytest.mark.parametrize("kwargs", [dict(gradient_clip_val=1.0, gradient_clip_algorithm="l2"),
                                    dict(gradient_clip_val=-0.5), dict(gradient_clip_val=float("nan"))])
def test_invalid_clip_arguments_raise(kwargs):
    with pytest.raises(ValueError):
        TrainStep(Toy(hidden=8, learning_rate=1e-2), **kwargs)


def test_clipped_trainstep_gloo_world2(tmp_path):
    """Two gloo ranks through launch_ranks, clipping by norm at a value that engages: the norm TrainStep reports is the norm of the gradient
    mean (not of a rank's own gradient), the ranks agree on it exactly and hold identical weights."""
    from voice100_amd.trainer import launch_ranks
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_gradclip_worker.py")
    assert launch_ranks(worker, [str(tmp_path), "0.05"], 2, timeout=300) == 0
    r0, r1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(2))
    assert r0["norms"] == r1["norms"]
    for a, b in zip(r0["final"], r1["final"]):
        assert torch.equal(a, b)
    for got, want in zip(r0["norms"], r0["want"]):
        assert got == pytest.approx(want, rel=1e-5)
        assert want > 0.05                                  # the clip engaged on every step
