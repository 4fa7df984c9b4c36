#!/usr/bin/env python3
"""Time of the batch-ensemble kernels (csrc/batch_ensemble.hip), of the eval mean of one residual
stage on its two routes, and of one training and one validation step of a ``CatNet(batch_ensemble=4)``,
each against the same arithmetic in plain torch ops (the reference's stack / broadcast / mean code) in
fp32 on the same GPU.

    python tools/bench_batch_ensemble.py [--iters 20] [--warmup 3] [--inner 10]

Two sizes each: the fixture's and a workload-like one (a stage activation [16, 64, 64, 64, 16] of a
classifier on [16, 3, 128, 128, 32] volumes for the scale; a 64-wide stage on [16, 64, 32, 32, 8] for
the mean; a two-stage network on [8, 1, 64, 64, 16] for the steps).
  * ``be_scale``: forward plus backward against ``x * table[idx][:, :, None, None, None]`` and
    autograd (the broadcast multiply, and for the table an index-add of the per-item sums).
  * ``stage_mean``: ``BatchEnsembleWrapper`` in eval mode around two residual blocks, n = 4: the
    "batched" route, the "loop" route and the reference's loop (2 n multiplies, a stack and a mean).
  * ``training_step`` / ``validation_step``: ``ClassNetPL`` around the network with the layers as
    built, against the same module with ``functional.be_scale`` and the eval mean replaced by the
    torch expressions (convolutions, norms and head are the same HIP kernels on both sides).
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds): end-to-end times of the whole call, launch, autograd and
allocation included. One JSON line per case."""
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

from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd.modules.layers import batch_ensemble as BE  # noqa: E402
from adell_mri_amd.modules.layers.adn_fn import get_adn_fn  # noqa: E402
from adell_mri_amd.modules.layers.res_blocks import ResidualBlock3d  # noqa: E402

N = 4
SCALE_SHAPES = [(4, 8, 8, 8, 4), (16, 64, 64, 64, 16)]
STAGES = [((4, 8, 8, 8, 4), 8), ((16, 64, 32, 32, 8), 64)]           # (input, inner width)
NETWORKS = [((4, 1, 16, 16, 8), [(8, 8, 3, 2), (16, 16, 3, 2)]),
            ((8, 1, 64, 64, 16), [(32, 32, 3, 2), (64, 64, 3, 2)])]


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, out


def compare(name, fns, args, extra, inner=None):
    """``fns``: {label: callable}; the first is what the others are compared with. Alternating
    rounds: the machine is shared."""
    inner = inner or args.inner
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    times, outs = {k: [] for k in fns}, {}
    for _ in range(args.iters):
        for k, fn in fns.items():
            us, outs[k] = timed(fn, inner)
            times[k].append(us)
    first = next(iter(fns))
    line = {"case": name, **extra}
    for k, t in times.items():
        line[k + "_us"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2),
                           "max": round(max(t), 2)}
        if k != first:
            line[f"{k}_over_{first}"] = round(statistics.median(t) / statistics.median(times[first]), 2)
            line[f"{first}_max_below_{k}_min"] = bool(max(times[first]) < min(t))
            line[f"{k}_max_below_{first}_min"] = bool(max(t) < min(times[first]))
            line[f"max_abs_difference_{k}"] = float(
                (outs[k].double() - outs[first].double()).abs().max())
    print(json.dumps(line), flush=True)


def channels_last(t):
    return t.contiguous(memory_format=torch.channels_last_3d) if t.dim() == 5 else t


def rows_of(table, x):
    return table.reshape(table.shape + (1,) * (x.dim() - 2))


def torch_scale(x, table, idx=None):
    return x * rows_of(table[idx.long()] if idx is not None else table[:1], x)


def torch_members_mean(X, pre, post, n, mod, route=None):
    """The reference's eval loop (batch_ensemble.py:244-254)."""
    outs = []
    for m in range(n):
        o = mod(X * rows_of(pre[m][None], X))
        outs.append(o * rows_of(post[m][None], o))
    return torch.stack(outs).mean(0)


def bench_scale(args, dev):
    g = torch.Generator().manual_seed(0)
    for shape in SCALE_SHAPES:
        x = channels_last(torch.randn(shape, generator=g).to(dev))
        dy = channels_last(torch.randn(shape, generator=g).to(dev))
        table = (1 + 0.1 * torch.randn((N, shape[1]), generator=g)).to(dev)
        idx = HF.be_indices(np.random.default_rng(0).integers(0, N, shape[0]), N, shape[0], dev)

        def fwd_bwd(fn):
            def run():
                xd, td = x.detach().requires_grad_(True), table.detach().requires_grad_(True)
                fn(xd, td, idx).backward(dy)
                return torch.cat([xd.grad.flatten()[:4096], td.grad.flatten()])
            return run

        compare("be_scale", {"hip": fwd_bwd(HF.be_scale), "torch": fwd_bwd(torch_scale)}, args,
                {"shape": list(shape), "n": N, "bytes_per_tensor": x.numel() * 4})


def bench_stage_mean(args, dev):
    adn = get_adn_fn(3, "batch", "swish", 0.0)
    g = torch.Generator().manual_seed(1)
    for shape, inner_width in STAGES:
        width = shape[1]
        torch.manual_seed(0)
        np.random.seed(0)
        stage = torch.nn.Sequential(
            ResidualBlock3d(width, 3, inner_width, width, adn),
            ResidualBlock3d(width, 3, inner_width, width, adn, skip_activation=True))
        layer = BE.BatchEnsembleWrapper(None, N, width, width, adn)
        stage, layer = stage.to(dev).eval(), layer.to(dev).eval()
        x = channels_last(torch.randn(shape, generator=g).to(dev))
        pre, post = layer.all_weights["pre"], layer.all_weights["post"]

        def reference():
            with torch.no_grad():
                return layer.adn_op(torch_members_mean(x, pre, post, N, stage))

        compare("stage_mean", {"batched": lambda: layer(x, mod=stage, route="batched"),
                               "loop": lambda: layer(x, mod=stage, route="loop"),
                               "torch": reference}, args,
                {"shape": list(shape), "n": N, "member_batch_bytes": x.numel() * 4,
                 "chunk": HF.be_chunk(N, shape[0], x[0].numel() * 4),
                 "default_route": HF.be_route(N, shape[0], x[0].numel() * 4, stage)})


def bench_steps(args, dev):
    from adell_mri_amd.modules.classification.pl import ClassNetPL

    for shape, structure in NETWORKS:
        torch.manual_seed(0)
        np.random.seed(0)
        net = ClassNetPL(adn_fn=get_adn_fn(3, "batch", "swish", 0.0), spatial_dimensions=3,
                         in_channels=shape[1], n_classes=2, resnet_structure=structure,
                         maxpool_structure=[(2, 2, 2)] * len(structure), batch_ensemble=N).to(dev)
        g = torch.Generator().manual_seed(2)
        batch = {"image": torch.rand(shape, generator=g).to(dev),
                 "label": (torch.rand((shape[0],), generator=g) > 0.5).float().to(dev)}
        built = (HF.be_scale, BE.members_mean)

        def step(fused, train):
            def run():
                HF.be_scale, BE.members_mean = built if fused else (torch_scale, torch_members_mean)
                try:
                    np.random.seed(3)                       # the same members on both sides
                    if train:
                        net.train()
                        net.zero_grad()
                        loss = net.training_step(batch, 0)
                        loss.backward()
                    else:
                        net.eval()
                        with torch.no_grad():
                            loss = net.validation_step(batch, 0)
                            loss = loss[0] if isinstance(loss, tuple) else loss
                finally:
                    HF.be_scale, BE.members_mean = built
                return loss.detach()
            return run

        extra = {"input": list(shape), "structure": [list(s) for s in structure], "n": N}
        compare("training_step", {"hip": step(True, True), "torch": step(False, True)}, args, extra,
                inner=max(1, args.inner // 2))
        compare("validation_step", {"hip": step(True, False), "torch": step(False, False)}, args,
                extra, inner=max(1, args.inner // 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_ensemble.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    bench_scale(args, dev)
    bench_stage_mean(args, dev)
    bench_steps(args, dev)


if __name__ == "__main__":
    main()
