#!/usr/bin/env python3
"""Timings of spectral normalisation on the device (README "Spectral normalisation", docs/LABBOOK.md):

    python tools/bench_spectral_norm.py [--reps 7] [--iters 50]

* per access, forward + backward, of the fused parametrization against torch's own ``_SpectralNorm`` on
  the same device tensors, at five weight shapes;
* one training step of the small U-Net of the tests (depths 4 / 16 / 32, 2 x 2 x 16^3) and of a wider
  one (depths 16 / 32 / 64 / 128, 2 x 2 x 64^3: the shape of ``smoke()``'s network at training size)
  with the fused parametrization, with torch's own ``spectral_norm`` on the same network (it runs through the
  same single-evaluation and pack fixes: its value has a ``grad_fn``, so its packs live on the tensor)
  and without spectral norm.
Medians over ``--reps`` repetitions of ``--iters`` timed iterations each, with the range; one JSON line
per measurement. Wall time between two device synchronisations, so launch and host cost are included:
that is what a training step pays."""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch.nn.utils.parametrizations import _SpectralNorm as TorchSN  # noqa: E402
from torch.nn.utils.parametrizations import spectral_norm as torch_spectral_norm  # noqa: E402

from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd.modules.layers.spectral_norm import _SpectralNorm  # noqa: E402

ACCESS = [((8, 8, 3, 3, 3), 0), ((64, 64, 3, 3, 3), 0), ((256, 256, 3, 3, 3), 0),
          ((128, 64, 2, 2, 2), 1), ((4096, 512), 0)]


def timed(fn, reps, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / iters * 1e6)
    out.sort()
    return {"median_us": round(out[len(out) // 2], 2), "min_us": round(out[0], 2),
            "max_us": round(out[-1], 2)}


def access(shape, dim, cls, reps, iters, dev):
    w = torch.randn(shape, device=dev, requires_grad=True)
    sn = cls(w.detach(), 1, dim, 1e-12).to(dev).train()
    g = torch.randn(shape, device=dev)

    def once():
        w.grad = None
        sn(w).backward(g)
    return timed(once, reps, iters)


def unet(kind, variant, dev):
    from adell_mri_amd.modules.activations import activation_factory
    from adell_mri_amd.modules.segmentation.losses import (CompoundLoss, binary_focal_loss,
                                                           binary_generalized_dice_loss)
    from adell_mri_amd.modules.segmentation.pl import UNetPL
    from adell_mri_amd.trainer import StepRunner

    if kind == "small":
        kw = dict(depth=[4, 16, 32], kernel_sizes=[3] * 3, strides=[2] * 3)
        shape = (2, 2, 16, 16, 16)
    else:
        kw = dict(depth=[16, 32, 64, 128], kernel_sizes=[3] * 4, strides=[2] * 4)
        shape = (2, 2, 64, 64, 64)
    loss_fn = CompoundLoss([(binary_generalized_dice_loss, {"smooth": 1e-5, "eps": 1e-6}),
                            (binary_focal_loss, {"gamma": 1.0, "eps": 1e-6})])
    net = UNetPL(image_key="image", label_key="mask", learning_rate=5e-4, weight_decay=5e-3,
                 loss_fn=loss_fn, activation_fn=activation_factory["swish"], spatial_dimensions=3,
                 conv_type="regular", link_type="residual", upscale_type="transpose",
                 norm_type="instance", padding=1, dropout_param=0.0, in_channels=2, n_classes=2,
                 **copy.deepcopy(kw)).to(dev).train()
    if variant == "torch":
        for m in list(net.modules()):
            for name, p in list(m.named_parameters(recurse=False)):
                if "weight" in name and p.ndim >= 2 and "Norm" not in type(m).__name__:
                    torch_spectral_norm(m, name)
    runner = StepRunner(net, spectral_norm=1 if variant == "fused" else None)
    g = torch.Generator().manual_seed(0)
    batch = {"image": torch.rand(shape, generator=g).to(dev),
             "mask": (torch.rand((shape[0], 1) + shape[2:], generator=g) > 0.9).float().to(dev)}
    return lambda: runner.train_step(batch)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shape, dim in ACCESS:
        outer = 1
        for s in shape[:dim]:
            outer *= s
        w = 1
        for s in shape[dim + 1:]:
            w *= s
        row = {"what": "access fwd+bwd", "shape": list(shape), "dim": dim,
               "route": HF.spectral_norm_route(shape[dim], outer * w)}
        row["fused"] = access(shape, dim, _SpectralNorm, args.reps, args.iters, dev)
        row["torch"] = access(shape, dim, TorchSN, args.reps, args.iters, dev)
        print(json.dumps(row), flush=True)
    if args.skip_steps:
        return
    for kind in ("small", "wide"):
        row = {"what": "training step", "unet": kind}
        for variant in ("fused", "torch", "none"):
            row[variant] = timed(unet(kind, variant, dev), args.reps, max(5, args.iters // 5))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
