#!/usr/bin/env python3
"""Forward + backward time of the fused DINO loss (DinoLoss, csrc/dino.hip) and of the DINO head
(L2 normalisation + weight-normalised Linear) against the plain-torch restatement of the
reference's arithmetic (tests/dino_ref.py) on the same GPU.

    python tools/bench_dino.py [--iters 50] [--warmup 5] [--inner 20]

One JSON line per case: device-event times of ``inner`` back-to-back calls, divided by ``inner``,
over ``iters`` alternating rounds (median, min, max, in microseconds); the bytes the algorithm needs
(loss: read a and b in the forward, read both and write da in the backward = 5 R K floats; head: the
[out, in] direction read by the forward and both backward GEMMs and its gradient written once, plus
the [R, out] activations) over the HIP time -- an end-to-end rate of the whole call, launches and
autograd included, not a kernel's share of peak; and the results of both sides."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dino_ref as R  # noqa: E402

from adell_mri_amd import functional as HF  # noqa: E402

LOSS_SHAPES = [(64, 65536), (8, 4096)]
HEAD = (64, 256, 65536)          # rows, in, out
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
        "algorithm_bytes": nbytes, "hip_gb_per_s": round(nbytes / med / 1e3, 1),
        "result_hip": float(out_hip), "result_torch": float(out_ref)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for rows, K in LOSS_SHAPES:
        a = (torch.rand((rows, K), generator=g) * 2 - 1).to(dev).requires_grad_(True)
        b = (torch.rand((rows, K), generator=g) * 2 - 1).to(dev)
        centers = (0.2 * (torch.rand((K,), generator=g) * 2 - 1)).to(dev)

        def hip():
            a.grad = None
            loss = HF.dino_loss(a, b, centers, T1, T2)
            loss.backward()
            return loss.detach()

        def ref():
            a.grad = None
            loss = R.dino_loss(a, b, centers, T1, T2)
            loss.backward()
            return loss.detach()

        compare("loss_fwd_bwd", hip, ref, 5 * rows * K * 4, args, {"shape": [rows, K]})

    rows, inp, out = HEAD
    x = torch.randn((rows, inp), generator=g).to(dev).requires_grad_(True)
    v = torch.randn((out, inp), generator=g).to(dev).requires_grad_(True)
    gm = torch.ones((out, 1), device=dev)
    r = torch.randn((rows, out), generator=g).to(dev)

    def hip_head():
        x.grad = v.grad = None
        y = HF.weight_norm_linear(HF.l2_normalize(x), gm, v)
        y.backward(r)
        return y.detach()[0, 0]

    def ref_head():
        x.grad = v.grad = None
        y = R.weight_norm_linear(R.l2_normalize(x), gm, v)
        y.backward(r)
        return y.detach()[0, 0]

    nbytes = 4 * (4 * out * inp + 6 * rows * out)
    compare("head_fwd_bwd", hip_head, ref_head, nbytes, args, {"rows": rows, "in": inp, "out": out})


if __name__ == "__main__":
    main()
