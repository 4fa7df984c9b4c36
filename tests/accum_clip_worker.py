"""Rank program of tests/test_accum_clip_multirank_gpu.py (not a test module): the small U-Net on
two ranks with Trainer(accumulate_grad_batches=2, gradient_clip_val=c) semantics through StepRunner
+ GradSync (bucketed all-reduce from backward hooks, sent only by the last micro-batch of a window),
then a toy module whose parameter ``a`` has a gradient in the first micro-batch of a window only.
Parameters are saved per rank."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def micro_batches(device, rank=None, windows=2, world=2):
    """Seeded inputs: micro-batch k of window w is item (rank) of a 2-item batch; rank=None gives
    the concatenation over ranks (the single-process equivalent)."""
    g = torch.Generator().manual_seed(1234)
    out = []
    for _ in range(2 * windows):
        x = torch.rand((world, 2, 32, 32, 32), generator=g)
        y = (torch.rand((world, 1, 32, 32, 32), generator=g) > 0.8).float()
        sl = slice(None) if rank is None else slice(rank, rank + 1)
        out.append({"image": x[sl].to(device), "mask": y[sl].to(device)})
    return out


def run(net, batches, clip, sync_kwargs=None):
    from adell_mri_amd.parallel import GradSync
    from adell_mri_amd.trainer import StepRunner

    opt = net.configure_optimizers()["optimizer"]
    sync = GradSync(opt, **(sync_kwargs or {}))
    runner = StepRunner(net, opt, sync, gradient_clip_val=clip, accumulate_grad_batches=2)
    for b in batches:
        runner.train_step(b)
    torch.cuda.synchronize()
    return runner, {k: p.detach().cpu().clone() for k, p in net.named_parameters()}


class Toy(torch.nn.Module):
    def __init__(self, device):
        super().__init__()
        self.a = torch.nn.Parameter(torch.full((8,), 2.0, device=device))
        self.b = torch.nn.Parameter(torch.full((8,), 3.0, device=device))

    def training_step(self, batch, idx):
        if idx % 2 == 0:
            return (self.a * batch["x"]).sum() + (self.b * batch["x"]).sum()
        return (self.b * batch["x"]).sum()


def main():
    import ddp_worker

    from adell_mri_amd.optim import FusedSGD
    from adell_mri_amd.parallel import GradSync, init_distributed
    from adell_mri_amd.trainer import StepRunner

    out, clip = sys.argv[1], float(sys.argv[2])
    rank, world, _ = init_distributed()
    device = torch.device("cuda", 0)    # both ranks share the one card (gloo)
    torch.cuda.set_device(device)
    net = ddp_worker.build(device)
    runner, params = run(net, micro_batches(device, rank), clip,
                         dict(n_buckets=3, min_bucket_elems=1))
    assert runner.sync.overlap and len(runner.sync.buckets) == 3
    assert runner.optimizer_steps == 2 and runner.step_idx == 4
    toy = Toy(device)
    opt = FusedSGD(toy.parameters(), lr=0.5)
    tr = StepRunner(toy, opt, GradSync(opt), accumulate_grad_batches=2)
    assert tr.sync.overlap
    x = torch.arange(8, dtype=torch.float32, device=device) * (rank + 1)
    tr.train_step({"x": x})
    tr.train_step({"x": torch.ones(8, device=device)})
    torch.cuda.synchronize()
    torch.save({"params": params, "norm": float(runner.last_grad_norm),
                "toy": {"a": toy.a.detach().cpu(), "b": toy.b.detach().cpu()}},
               os.path.join(out, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
