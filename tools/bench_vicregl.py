#!/usr/bin/env python3
"""Forward + backward time of the local VICReg loss alone (VICRegLocalLoss, csrc/vicregl.hip)
against the plain-torch restatement of the reference's arithmetic (tests/vicregl_ref.py with
rank="cdist": torch.cdist + torch.topk, which materialise the T x T matrices) on the same GPU.

    python tools/bench_vicregl.py [--iters 10] [--warmup 3]

One JSON line per shape: device-event times over ``iters`` alternating rounds (median, min, max,
in ms), the four terms of both, and the per-kernel arithmetic the ranking needs (3 T^2 C flops per
item: subtract, multiply, add) over the time of the HIP loss -- an end-to-end rate of the whole
loss, not a kernel's share of peak."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import vicregl_ref as R  # noqa: E402

from adell_mri_amd.modules.self_supervised.losses import VICRegLocalLoss  # noqa: E402

SHAPES = [((32, 512, 4, 4, 4), 10), ((32, 128, 64, 64), 10)]


def timed(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    for shape, gamma in SHAPES:
        g = torch.Generator().manual_seed(0)
        B, ndim = shape[0], len(shape) - 2
        fmt = torch.channels_last_3d if ndim == 3 else torch.channels_last
        x1 = torch.randn(shape, generator=g).to(dev).contiguous(memory_format=fmt).requires_grad_(True)
        x2 = (0.5 * x1.detach().cpu() + torch.randn(shape, generator=g)).to(dev).contiguous(
            memory_format=fmt).requires_grad_(True)
        lo1, lo2 = 20.0 * torch.rand((B, ndim), generator=g), 20.0 * torch.rand((B, ndim), generator=g)
        b1 = torch.cat([lo1, lo1 + 16.0 + 32.0 * torch.rand((B, ndim), generator=g)], 1).to(dev)
        b2 = torch.cat([lo2, lo2 + 16.0 + 32.0 * torch.rand((B, ndim), generator=g)], 1).to(dev)
        loss = VICRegLocalLoss(gamma=gamma)

        def hip():
            x1.grad = x2.grad = None
            terms = loss(x1, x2, b1, b2)
            sum(terms).backward()
            return [float(t.detach()) for t in terms]

        def torch_ref():
            x1.grad = x2.grad = None
            terms, _, _ = R.vicregl_loss(x1, x2, b1, b2, gamma=gamma, rank="cdist")
            sum(terms).backward()
            return [float(t.detach()) for t in terms]

        for _ in range(args.warmup):
            hip()
            torch_ref()
        t_hip, t_ref = [], []
        for _ in range(args.iters):           # alternating: the machine is shared
            ms, terms_hip = timed(hip)
            t_hip.append(ms)
            ms, terms_ref = timed(torch_ref)
            t_ref.append(ms)
        T = 1
        for s in shape[2:]:
            T *= s
        flops = 3.0 * B * T * T * (shape[1] + ndim)
        med = statistics.median(t_hip)
        print(json.dumps({
            "shape": list(shape), "gamma": gamma, "tokens": T,
            "hip_ms": {"median": round(med, 3), "min": round(min(t_hip), 3), "max": round(max(t_hip), 3)},
            "torch_ms": {"median": round(statistics.median(t_ref), 3), "min": round(min(t_ref), 3),
                         "max": round(max(t_ref), 3)},
            "speedup_median": round(statistics.median(t_ref) / med, 2),
            "ranking_gflops_over_hip_loss_time": round(flops / med / 1e6, 1),
            "terms_hip": terms_hip, "terms_torch": terms_ref}), flush=True)


if __name__ == "__main__":
    main()
