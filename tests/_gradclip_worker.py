"""Worker of tests/test_gradclip_cpu.py::test_clipped_trainstep_gloo_world2, started by voice100_amd.trainer.launch_ranks: the world-2
TrainStep of tests/_dist_worker.py with gradient clipping by norm.  Each rank writes its weights, the norm TrainStep reported at every step
and the norm of the mean gradient it saw (recomputed independently: the gradient mean gathered over the ranks) to <outdir>/rank<r>.pt."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for d in (ROOT, HERE):
    if d not in sys.path:
        sys.path.insert(0, d)

import torch
import torch.distributed as dist

from _dist_worker import Toy
from voice100_amd.dist import shard_batch
from voice100_amd.trainer import TrainStep, init_distributed


def main():
    outdir, clip = sys.argv[1], float(sys.argv[2])
    if torch.cuda.is_available():
        dist.init_process_group("gloo")                  # gloo on the CPU, as tests/_dist_worker.py
    rank, _, world = init_distributed()
    assert dist.is_initialized() and dist.get_world_size() == world == 2
    torch.manual_seed(100 + rank)
    model = Toy(hidden=8, learning_rate=1e-2)
    step = TrainStep(model, bucket_bytes=64, gradient_clip_val=clip)
    g = torch.Generator().manual_seed(7)
    x_all, y_all = torch.randn(6, 4, 20, generator=g) * 10, torch.randn(6, 2, 20, generator=g)
    lo, hi = shard_batch(6, rank, world)
    norms, want = [], []
    finish = step.buckets.finish_step

    def finish_and_measure():                            # the mean gradient, between the exchange and the clip: its norm, in fp64
        finish()
        want.append(float(torch.cat([p.grad.reshape(-1) for p in model.parameters()]).double().norm()))

    step.buckets.finish_step = finish_and_measure
    for _ in range(3):
        step((x_all[lo:hi], y_all[lo:hi]))
        norms.append(float(step.last_grad_norm))
    torch.save({"final": [p.detach().clone() for p in model.parameters()], "norms": norms, "want": want},
               os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
