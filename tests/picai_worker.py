"""Rank program of tests/test_picai_eval_multirank_gpu.py (not a test module): every rank feeds its
shard of the fixture cases to a PicaiEval, then ``compute()`` averages AP / score / AUROC over the
ranks (Lightning's sync_dist). Values and the local values are saved per rank."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "picai_eval.npz")


def shard(rank, world=2):
    """(probabilities, targets) of this rank's cases: every other fixture case."""
    f = np.load(GOLDEN)
    idx = list(range(rank, len(f["names"]), world))
    p = f["pred_levels"][idx].astype(np.float32) / np.float32(255)
    return torch.from_numpy(p), torch.from_numpy(f["target"][idx])


def main():
    from adell_mri_amd.modules.segmentation.picai_eval import PicaiEval
    from adell_mri_amd.parallel import init_distributed

    out = sys.argv[1]
    rank, world, _ = init_distributed()
    device = torch.device("cuda", 0)    # both ranks share the one card (gloo)
    torch.cuda.set_device(device)
    p, t = shard(rank, world)
    acc = PicaiEval()
    acc.update(p[:3].to(device).unsqueeze(1), t[:3].to(device).unsqueeze(1))
    acc.update(p[3:].to(device), t[3:].to(device))
    m = acc.metrics()
    with np.errstate(invalid="ignore", divide="ignore"):
        local = [m.AP, m.score, m.auroc]
    values = acc.compute()
    torch.save({"values": values, "local": local}, os.path.join(out, f"rank{rank}.pt"))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
