#!/usr/bin/env python3
"""Time of the classification kernels (csrc/classify.hip) against their plain-torch composites, in
fp32 on the same GPU.

    python tools/bench_classification.py [--iters 30] [--warmup 3] [--inner 20]

  * ``mixup``: ``functional.mixup_rows`` against ``x * f + x[perm] * (1.0 - f)`` at
    [16, 3, 128, 128, 32] and [4, 1, 64, 64, 16]. The algorithm reads two rows and writes one per
    item: 3 B V floats.
  * ``bce`` / ``ce`` / ``ordinal`` / ``roc``: forward plus backward of each loss at B = 32 and
    B = 256 (K = 5 classes for ``ce`` and ``ordinal``) against
    ``binary_cross_entropy_with_logits`` / ``cross_entropy`` / the reference's ordinal composite /
    its relative order consistency, written out in torch.
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds). For mixup also the bytes the algorithm needs over the HIP
time: an end-to-end rate of the whole call, launch and allocation included, not a kernel's share of
peak. The losses are launch-bound: their times are launch and autograd overhead, not arithmetic."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from adell_mri_amd import functional as HF  # noqa: E402

MIXUP_SHAPES = [(16, 3, 128, 128, 32), (4, 1, 64, 64, 16)]
LOSS_BATCHES = [32, 256]
K = 5


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, out


def compare(name, hip, ref, args, extra, nbytes=None):
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
    line = {
        "case": name, **extra,
        "hip_us": {"median": round(med, 2), "min": round(min(t_hip), 2), "max": round(max(t_hip), 2)},
        "torch_us": {"median": round(med_ref, 2), "min": round(min(t_ref), 2),
                     "max": round(max(t_ref), 2)},
        "torch_over_hip": round(med_ref / med, 2),
        "hip_max_below_torch_min": bool(max(t_hip) < min(t_ref)),
        "torch_max_below_hip_min": bool(max(t_ref) < min(t_hip)),
        "max_abs_difference": float((out_hip.double() - out_ref.double()).abs().max())}
    if nbytes is not None:
        line.update({"algorithm_bytes": nbytes, "hip_gb_per_s": round(nbytes / med / 1e3, 1),
                     "torch_gb_per_s": round(nbytes / med_ref / 1e3, 1)})
    print(json.dumps(line), flush=True)


def torch_ordinal(pred, target, n_classes):
    t = (target[:, None] >= torch.arange(1, n_classes, device=pred.device)[None, :]).to(pred.dtype)
    ls = F.logsigmoid(pred)
    return -(ls * t + (ls - pred) * (1 - t)).sum(1)


def torch_roc(pred, target):
    pred = pred.squeeze(1)
    d = pred[:, None] - pred[None, :]
    td = target[:, None] - target[None, :]
    keep = td != 0
    return F.binary_cross_entropy_with_logits(d[keep], torch.clamp(td, 0, 1).to(pred.dtype)[keep])


def fwd_bwd(loss_fn, x):
    """Forward plus backward of ``loss_fn`` on a fresh leaf; returns the gradient."""
    def run():
        leaf = x.detach().requires_grad_(True)
        loss_fn(leaf).backward()
        return leaf.grad
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classification.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(0)
    for shape in MIXUP_SHAPES:
        B = shape[0]
        x = torch.rand(shape, generator=g).to(dev)
        factor = torch.as_tensor(rng.beta(0.4, 0.4, B), dtype=torch.float32, device=dev)
        perm = (np.arange(B) + 1 + rng.integers(0, B - 1, 1)[0]) % B          # no fixed point
        perm_dev = torch.as_tensor(perm, device=dev)
        fx = factor.reshape([-1] + [1] * (len(shape) - 1))
        compare("mixup", lambda: HF.mixup_rows(x, factor, perm),
                lambda: x * fx + x[perm_dev] * (1.0 - fx), args, {"shape": list(shape)},
                nbytes=3 * x.numel() * 4)
    for B in LOSS_BATCHES:
        x1 = (torch.rand((B,), generator=g) * 8 - 4).to(dev)
        xk = (torch.rand((B, K), generator=g) * 8 - 4).to(dev)
        xo = (torch.rand((B, K - 1), generator=g) * 8 - 4).to(dev)
        pre = (torch.rand((B, 1), generator=g) * 8 - 4).to(dev)
        soft = torch.rand((B,), generator=g).to(dev)
        y = torch.randint(0, K, (B,), generator=g).to(dev)
        w = (torch.rand((K,), generator=g) + 0.5).to(dev)
        extra = {"B": B, "K": K}
        compare("bce", fwd_bwd(lambda t: HF.bce_with_logits(t, soft), x1),
                fwd_bwd(lambda t: F.binary_cross_entropy_with_logits(t, soft), x1), args, extra)
        compare("ce", fwd_bwd(lambda t: HF.cross_entropy(t, y, w), xk),
                fwd_bwd(lambda t: F.cross_entropy(t, y, w), xk), args, extra)
        compare("ordinal", fwd_bwd(lambda t: HF.ordinal_sigmoidal_loss(t, y, K).mean(), xo),
                fwd_bwd(lambda t: torch_ordinal(t, y, K).mean(), xo), args, extra)
        compare("roc", fwd_bwd(lambda t: HF.relative_order_consistency(t, y), pre),
                fwd_bwd(lambda t: torch_roc(t, y), pre), args, extra)


if __name__ == "__main__":
    main()
