#!/usr/bin/env python3
"""Time and peak memory of the semi-supervised losses of csrc/semisl.hip, forward plus backward,
each against the same rule in plain torch ops (the reference's expressions, the "composed" route) in
fp32 on the same GPU.

    python tools/bench_semisl_losses.py [--iters 10] [--warmup 2] [--inner 5]

Features are channels-last, as the networks produce them. Two sizes per loss:
  * ``anchor``: ``functional.loco_anchor_loss`` at [2, 32, 16^3] and [2, 32, 64^3], anchors detached
    (the wrapper's case).
  * ``nn``: ``functional.nn_queue_loss`` at (B, C, K, V, Q) = (2, 32, 2, 16^3, 64) and
    (2, 32, 2, 32^3, 128). The composite's ``F.cosine_similarity`` multiplies the broadcast normalised
    operands, a [B, V, Q, C] product, on top of its [B, V, Q] tensors; the large size is chosen IN
    ADVANCE, not by running out of memory: its [B, V, Q] tensors are 32 MiB each (about ten of them
    live at once) and the product is 1 GiB (B V Q C * 4 bytes, printed as ``composite_product_mib``);
    with the product's gradient and the normalised temporaries the composite was expected to peak
    near 4 GiB and measures 5.1 GiB. The next size up (Q or V doubled) would double that.
  * ``pseudo_label``: ``functional.pseudo_label_ce`` at [2, 3, 16^3] and [2, 3, 128^3] with a weight and
    label smoothing, against ``F.cross_entropy`` on the thresholded targets.
  * ``put``: ``NearestNeighbourLoss.put`` at [2, 32, 32^3] and [2, 32, 96^3] with two classes, against the
    reference's ``torch.where`` / index / choice on the device.
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds): end-to-end times of the whole call, launch, autograd and
allocation included. ``peak_mib``: ``torch.cuda.max_memory_allocated`` over one call of each route,
less what was allocated before it. One JSON line per case."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd.modules.semi_supervised_segmentation import NearestNeighbourLoss  # noqa: E402


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, out


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 2 ** 20, 1)


def compare(name, fns, args, extra):
    """``fns``: {label: callable}, "fused" first. Alternating rounds: the machine is shared."""
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    times, outs = {k: [] for k in fns}, {}
    for _ in range(args.iters):
        for k, fn in fns.items():
            us, outs[k] = timed(fn, args.inner)
            times[k].append(us)
    line = {"case": name, **extra}
    for k, t in times.items():
        line[k + "_us"] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1),
                           "max": round(max(t), 1)}
        line[k + "_peak_mib"] = peak_mib(fns[k])
    f, c = times["fused"], times["composed"]
    line["composed_over_fused"] = round(statistics.median(c) / statistics.median(f), 2)
    line["verdict"] = ("faster" if max(f) < min(c) else "SLOWER" if max(c) < min(f)
                       else "not distinguishable")
    if outs["fused"] is not None:
        line["max_abs_difference"] = float((outs["fused"].double() - outs["composed"].double()).abs().max())
    print(json.dumps(line), flush=True)


def features(shape, g, dev):
    return torch.randn(shape, generator=g).to(dev).contiguous(memory_format=torch.channels_last_3d)


def bench_anchor(args, dev, g):
    for side in (16, 64):
        shape = (2, 32, side, side, side)
        x = features(shape, g, dev).requires_grad_(True)
        a1, a2 = features(shape, g, dev), features(shape, g, dev)

        def run(fn):
            x.grad = None
            fn(x, a1, a2, 0.1).sum().backward()
            return x.grad
        compare("anchor", {"fused": lambda: run(HF.loco_anchor_loss),
                           "composed": lambda: run(HF.loco_anchor_loss_composite)}, args,
                {"shape": list(shape)})


def bench_nn(args, dev, g):
    for side, Q in ((16, 64), (32, 128)):
        B, C, K = 2, 32, 2
        shape = (B, C, side, side, side)
        x = features(shape, g, dev).requires_grad_(True)
        y = (torch.rand((B, K, side, side, side), generator=g) > 0.5).float().to(dev)
        past = torch.randn(Q, C, generator=g).to(dev)
        cls = torch.arange(Q, dtype=torch.int32, device=dev) * K // Q
        labels = F.one_hot(cls.long(), K)

        def fused():
            x.grad = None
            HF.nn_queue_loss(x, y, past, cls, 0.1).backward()
            return x.grad

        def composed():
            x.grad = None
            HF.nn_queue_loss_composite(x, y, past, labels, 0.1).backward()
            return x.grad
        compare("nn", {"fused": fused, "composed": composed}, args,
                {"shape": list(shape), "K": K, "Q": Q,
                 "composite_product_mib": B * side ** 3 * Q * C * 4 / 2 ** 20})


def bench_pl(args, dev, g):
    for side in (16, 128):
        shape = (2, 3, side, side, side)
        pred = torch.randn(shape, generator=g).to(dev).requires_grad_(True)
        proba = torch.rand(shape, generator=g).to(dev)
        w = torch.tensor([0.2, 1.0, 3.0], device=dev)

        def fused():
            pred.grad = None
            HF.pseudo_label_ce(pred, proba, 0.7, w, 0.1, "mean").backward()
            return pred.grad

        def composed():
            pred.grad = None
            F.cross_entropy(pred, (proba > 0.7).float(), w, label_smoothing=0.1).backward()
            return pred.grad
        compare("pseudo_label", {"fused": fused, "composed": composed}, args, {"shape": list(shape)})


def reference_put(mod, X, y):
    X = X.flatten(start_dim=2)
    y = y.flatten(start_dim=2)
    b, c, v = torch.where(y > 0)
    for cl in range(mod.n_classes):
        idx = c == cl
        elements = X[b[idx], :, v[idx]]
        n_elements = elements.shape[0]
        if n_elements > mod.max_elements_per_batch:
            elements = elements[mod.rng.choice(n_elements, mod.max_elements_per_batch)]
        if n_elements > 0:
            mod.q[cl].put(elements.detach())


def bench_put(args, dev, g):
    for side in (32, 96):
        shape = (2, 32, side, side, side)
        x = features(shape, g, dev)
        y = (torch.rand((2, 2, side, side, side), generator=g) > 0.5).float().to(dev)

        def run(put):
            mod = NearestNeighbourLoss(maxsize=0, n_classes=2, max_elements_per_batch=256,
                                       n_samples_per_class=4)
            put(mod, x, y)
            return torch.cat([mod.q[cl].queue[0] for cl in range(2)])
        compare("put", {"fused": lambda: run(lambda m, a, b: m.put(a, b)),
                        "composed": lambda: run(reference_put)}, args, {"shape": list(shape)})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    device = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    for name, fn in (("anchor", bench_anchor), ("nn", bench_nn), ("pseudo_label", bench_pl),
                     ("put", bench_put)):
        if not a.only or name in a.only.split(","):
            fn(a, device, gen)
