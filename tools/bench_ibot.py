#!/usr/bin/env python3
"""Time of iBOT's token-level losses on the fused kernels (functional.ibot_view, ops.ibot_token_sums;
csrc/ibot.hip) against the plain-torch restatement of the reference's arithmetic (tests/ibot_ref.py)
on the same GPU.

    python tools/bench_ibot.py [--iters 30] [--warmup 3] [--inner 10]

Per case (B, Tt, K, M) two JSON lines:
  * ``view_fwd_bwd``: forward plus backward of one view -- the "mean" reduction of the student's
    logits and the masked-row loss, gradients of both into ds;
  * ``teacher_pass``: the teacher's side of one step for two views -- the "mean" reduction of each
    view and the centre sum over all patch tokens of both (the restatement concatenates them).
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds), and the bytes the algorithm needs (view: one read of s,
one write of ds, the masked rows of s and y twice more = 4 (2 B Tt K + 4 B M K); teacher: one read
of each teacher tensor = 4 (2 B Tt K)) over the HIP time -- an end-to-end rate of the whole call,
launches and autograd included, not a kernel's share of peak."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dino_ref as R  # noqa: E402
import ibot_ref as IR  # noqa: E402

from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd import ops  # noqa: E402

CASES = [(8, 216, 8192, 54), (2, 216, 8192, 54)]
T1, T2 = 0.1, 0.04


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, out


def compare(name, hip, ref, nbytes, args, extra):
    for _ in range(args.warmup):
        hip()
        ref()
    t_hip, t_ref = [], []
    for _ in range(args.iters):               # alternating: the machine is shared
        us, out_hip = timed(hip, args.inner)
        t_hip.append(us)
        us, out_ref = timed(ref, args.inner)
        t_ref.append(us)
    med, med_ref = statistics.median(t_hip), statistics.median(t_ref)
    print(json.dumps({
        "case": name, **extra,
        "hip_us": {"median": round(med, 2), "min": round(min(t_hip), 2), "max": round(max(t_hip), 2)},
        "torch_us": {"median": round(med_ref, 2), "min": round(min(t_ref), 2),
                     "max": round(max(t_ref), 2)},
        "torch_over_hip": round(med_ref / med, 2),
        "hip_max_below_torch_min": bool(max(t_hip) < min(t_ref)),
        "algorithm_bytes": nbytes, "hip_gb_per_s": round(nbytes / med / 1e3, 1),
        "result_hip": float(out_hip), "result_torch": float(out_ref)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for B, Tt, K, M in CASES:
        s = (torch.rand((B, Tt, K), generator=g) * 2 - 1).to(dev).requires_grad_(True)
        y = (torch.rand((B, Tt, K), generator=g) * 2 - 1).to(dev)
        y2 = (torch.rand((B, Tt, K), generator=g) * 2 - 1).to(dev)
        centers = (0.2 * (torch.rand((K,), generator=g) * 2 - 1)).to(dev)
        w = (torch.rand((B, K), generator=g) * 2 - 1).to(dev)
        m = np.unique(np.linspace(0, Tt - 1, M).astype(np.int64))
        assert len(m) == M
        rows = HF.patch_rows(m, Tt, 0, dev)      # a fixed mask: one upload, as the table cache keeps it
        shape = {"B": B, "Tt": Tt, "K": K, "M": M}

        def hip_view():
            s.grad = None
            s_red, loss = HF.ibot_view(s, y, rows, centers, T1, T2, False, "mean")
            (loss + (s_red * w).sum()).backward()
            return loss.detach()

        def ref_view():
            s.grad = None
            s_red, loss = IR.view(s, y, m, centers, T1, T2, False, "mean")
            (loss + (s_red * w).sum()).backward()
            return loss.detach()

        compare("view_fwd_bwd", hip_view, ref_view, 4 * (2 * B * Tt * K + 4 * B * M * K), args, shape)

        def hip_teacher():
            sums = torch.empty((2 * B, K), device=dev, dtype=torch.float64)
            mean1, _ = ops.ibot_token_sums(y, 0, 1.0 / Tt, raw_out=sums[:B])
            mean2, _ = ops.ibot_token_sums(y2, 0, 1.0 / Tt, raw_out=sums[B:])
            return ops.ibot_center_sum(sums)[0, 0] + mean1[0, 0] + mean2[0, 0]

        def ref_teacher():
            mean1, _ = IR.reduce(y, False, "mean")
            mean2, _ = IR.reduce(y2, False, "mean")
            total, _ = R.center_sum(torch.cat([y, y2]))
            return total[0, 0] + mean1[0, 0] + mean2[0, 0]

        compare("teacher_pass", hip_teacher, ref_teacher, 4 * 2 * B * Tt * K, args, shape)


if __name__ == "__main__":
    main()
