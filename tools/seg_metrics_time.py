"""Timing of the segmentation metrics (csrc/seg_metrics.hip).

  loop: N x update_metrics of a 4-metric dict on a (2, 1, 128^3) fp32 prediction with an fp32
        target (33.5 MB read per update); run it under ``rocprofv3 --kernel-trace --stats`` for the
        per-kernel times, the script prints the wall time per update;
  step: config-2 training steps (bench.build_module, 2 x 128^3) with compute_train_metrics off and
        on, interleaved, timed with events; prints ms per step of each side."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def loop(n):
    from adell_mri_amd.modules.segmentation.pl import get_metric_dict, update_metrics

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    p = torch.rand((2, 1, 128, 128, 128), generator=g).to(dev)
    y = (torch.rand((2, 1, 128, 128, 128), generator=g) > 0.9).float().to(dev)
    md = get_metric_dict(2, False, None, "T_", dev=dev)
    for _ in range(10):
        update_metrics(None, md, p, y, None, None)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        update_metrics(None, md, p, y, None, None)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / n
    print(json.dumps({"updates": n, "us_per_update_wall": round(us, 2),
                      "bytes_per_update": p.numel() * 8,
                      "T_Dice": float(md["T_Dice"].compute())}))


def step(steps, rounds):
    import bench
    from adell_mri_amd.trainer import StepRunner

    dev = torch.device("cuda:0")
    net, _ = bench.build_module(dev)
    net.train()
    runner = StepRunner(net)
    batch = bench.synthetic_batch(2, 128, dev, 0)
    for _ in range(3):
        runner.train_step(batch)
    torch.cuda.synchronize()
    res = {False: [], True: []}
    for _ in range(rounds):
        for on in (False, True):
            net.compute_train_metrics = on
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                runner.train_step(batch)
            e1.record()
            torch.cuda.synchronize()
            res[on].append(e0.elapsed_time(e1) / steps)
    off, on = sorted(res[False]), sorted(res[True])
    print(json.dumps({"ms_per_step_off": off, "ms_per_step_on": on,
                      "median_delta_ms": round(on[len(on) // 2] - off[len(off) // 2], 4),
                      "train_IoU": float(net.train_metrics["IoU"].compute())}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["loop", "step"])
    ap.add_argument("--n", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    loop(a.n) if a.mode == "loop" else step(a.steps, a.rounds)
