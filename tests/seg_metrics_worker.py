"""Rank program of tests/test_seg_metrics_multirank_gpu.py (not a test module): every rank updates
binary and multi-class metrics with its shard of seeded predictions, then ``compute()`` sums the
counts over the ranks. Values and local counts are saved per rank."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shards(device, world=2, steps=3):
    """[(binary pred, binary target, 3-class pred, 3-class target)] per step and rank."""
    g = torch.Generator().manual_seed(77)
    out = []
    for _ in range(steps):
        row = []
        for _ in range(world):
            pb = torch.rand((1, 1, 12, 10, 9), generator=g)
            yb = (torch.rand((1, 1, 12, 10, 9), generator=g) < 0.3).float()
            pm = torch.randn((2, 3, 6, 7, 8), generator=g)
            ym = torch.randint(0, 3, (2, 6, 7, 8), generator=g)
            row.append(tuple(t.to(device) for t in (pb, yb, pm, ym)))
        out.append(row)
    return out


def build(device):
    from adell_mri_amd import metrics as M

    return {"IoU": M.BinaryJaccardIndex().to(device), "F1": M.BinaryFBetaScore(1.0).to(device),
            "mIoU": M.MulticlassJaccardIndex(3).to(device), "mDice": M.MulticlassDice(3).to(device)}


def update(ms, pb, yb, pm, ym):
    from adell_mri_amd import metrics as M

    M.update_many([ms["IoU"], ms["F1"]], pb, yb)
    M.update_many([ms["mIoU"], ms["mDice"]], pm, ym)


def main():
    from adell_mri_amd.parallel import init_distributed

    out = sys.argv[1]
    rank, world, _ = init_distributed()
    device = torch.device("cuda", 0)    # both ranks share the one card (gloo)
    torch.cuda.set_device(device)
    ms = build(device)
    for row in shards(device, world):
        update(ms, *row[rank])
    local = {k: m.state.cpu().clone() for k, m in ms.items()}
    values = {k: float(m.compute()) for k, m in ms.items()}
    after = {k: m.state.cpu().clone() for k, m in ms.items()}
    torch.save({"values": values, "local": local, "after": after},
               os.path.join(out, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
