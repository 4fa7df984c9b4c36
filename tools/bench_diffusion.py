#!/usr/bin/env python3
"""Time of the diffusion kernels (csrc/diffusion.hip) against the same arithmetic in plain torch ops
on the same GPU, by the method of tools/bench_mil.py.

    python tools/bench_diffusion.py [--iters 20] [--warmup 3] [--inner 10]

Two sizes: a workload size [2, 32, 128, 128, 32] and a launch-bound size [2, 8, 16, 16, 8].
  * ``eca_apply``: gate apply forward + backward against ``x * sigmoid(z)[..., None, None, None]`` in
    torch ops and against the existing ``functional.scale_per_item_channel(x, sigmoid(z))``.
  * ``eca_gates``: the logits of a seven-site network (depth [32, 64, 128], t_dim 256, and depth
    [8, 16, 32], t_dim 32) forward + backward against the seven blocks in torch modules.
  * ``reverse_step_<kind>``: one reverse step with guidance against the reference's chain of
    elementwise torch ops (coefficients from device tables, as it writes them).
  * ``sample_step``: one whole step of ``Diffusion.sample`` with guidance on the small 3-D network
    (two network calls and the step) against the same two calls followed by the torch chain.
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds). SLOWER where torch is faster; "not distinguishable" where
the two ranges overlap."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd.modules.activations import activation_factory  # noqa: E402
from adell_mri_amd.modules.diffusion import Diffusion, DiffusionUNet  # noqa: E402
from adell_mri_amd.modules.layers.class_attention import (  # noqa: E402
    EfficientConditioningAttentionBlock)

SHAPES = [(2, 32, 128, 128, 32), (2, 8, 16, 16, 8)]
GATE_NETS = [([32, 64, 128], 256), ([8, 16, 32], 32)]
KINDS = ("ddpm", "ddim", "alpha_deblending")


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, out


def compare(name, hip, ref, args, extra, ref_name="torch"):
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
    if max(t_hip) < min(t_ref):
        verdict = "faster"
    elif max(t_ref) < min(t_hip):
        verdict = "SLOWER"
    else:
        verdict = "not distinguishable"
    print(json.dumps({
        "case": name, "against": ref_name, **extra,
        "hip_us": {"median": round(med, 2), "min": round(min(t_hip), 2), "max": round(max(t_hip), 2)},
        "ref_us": {"median": round(med_ref, 2), "min": round(min(t_ref), 2), "max": round(max(t_ref), 2)},
        "ref_over_hip": round(med_ref / med, 2), "verdict": verdict,
        "max_abs_difference": float((out_hip.double() - out_ref.double()).abs().max())}), flush=True)


def channels_last(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


def torch_step(kind, d, x, eps, eps_u, scale, noise, t, eta=1.0):
    """The reference's step text on device tables (``d``: beta, alpha, alpha_bar on the device)."""
    e = eps_u + scale * (eps - eps_u)
    sh = (-1, 1, 1, 1, 1)
    ab = d["alpha_bar"][t].reshape(sh)
    abp = d["alpha_bar"][t - 1].reshape(sh)
    if kind == "ddpm":
        bb = 1.0 - ab
        x0 = torch.clamp((x - torch.sqrt(bb) * e) / torch.sqrt(ab), -1, 1)
        out = torch.sqrt(abp) * d["beta"][t] / bb * x0 + torch.sqrt(d["alpha"][t]) * (1.0 - abp) / bb * x
        return out + noise * torch.sqrt((1 - abp) / (1 - ab) * d["beta"][t]) * eta
    if kind == "ddim":
        var = torch.multiply(torch.sqrt((1 - abp) / (1 - ab)), torch.sqrt(1 - ab / abp)) * eta
        x0 = torch.divide(x - torch.sqrt(1 - ab) * e, torch.sqrt(ab))
        direction = torch.sqrt(torch.clamp(1 - abp - var ** 2, min=0)) * e
        return torch.add(torch.sqrt(abp) * x0, direction + noise * var)
    return x + (ab - abp) * e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_diffusion.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)

    for shape in SHAPES:
        N, Cc = shape[:2]
        x = channels_last(torch.randn(shape, generator=g).to(dev))
        dy = channels_last(torch.randn(shape, generator=g).to(dev))
        z = torch.randn((N, Cc), generator=g).to(dev)

        def fwd_bwd(fn):
            def run():
                xl, zl = x.detach().requires_grad_(True), z.detach().requires_grad_(True)
                fn(xl, zl).backward(dy)
                return xl.grad
            return run

        extra = {"shape": list(shape)}
        compare("eca_apply", fwd_bwd(HF.eca_apply),
                fwd_bwd(lambda a, b: a * torch.sigmoid(b)[:, :, None, None, None]), args, extra)
        compare("eca_apply", fwd_bwd(HF.eca_apply),
                fwd_bwd(lambda a, b: HF.scale_per_item_channel(a, torch.sigmoid(b))), args, extra,
                ref_name="scale_per_item_channel")

        eps, eps_u, noise = (channels_last(torch.randn(shape, generator=g).to(dev)) for _ in range(3))
        d = Diffusion(noise_steps=1000, img_size=tuple(shape[2:]))
        dt = {k: getattr(d, k).to(dev) for k in ("beta", "alpha", "alpha_bar")}
        for kind in KINDS:
            compare(f"reverse_step_{kind}",
                    lambda k=kind: HF.diffusion_reverse_step(k, x, eps, 500, d.tables, noise=noise,
                                                             eps_uncond=eps_u, scale=3.0),
                    lambda k=kind: torch_step(k, dt, x, eps, eps_u, 3.0, noise, 500), args, extra)

    for depth, t_dim in GATE_NETS:
        widths = depth + depth[:-1][::-1] + depth[:-1][::-1]
        torch.manual_seed(0)
        blocks = [EfficientConditioningAttentionBlock(t_dim, w, op_type="linear").to(dev) for w in widths]
        t = torch.tensor([0.3, 0.7], device=dev)
        gz = [torch.randn((2, w), generator=g).to(dev) for w in widths]

        def hip():
            for b in blocks:
                b.zero_grad()
            torch.autograd.backward(HF.eca_gates(t, blocks), gz)
            return blocks[0].class_to_channels.weight.grad

        def ref():
            for b in blocks:
                b.zero_grad()
            emb = HF.timestep_embedding(t, t_dim)
            torch.autograd.backward([b.op(b.class_to_channels(emb)) for b in blocks], gz)
            return blocks[0].class_to_channels.weight.grad

        compare("eca_gates_7_sites", hip, ref, args, {"depth": depth, "t_dim": t_dim})

    kw = dict(t_dim=32, classifier_free_guidance=True, classifier_classes=3, spatial_dimensions=3,
              in_channels=1, depth=[8, 16, 32], strides=[[2, 2, 2], [2, 2, 1], [2, 2, 1]],
              kernel_sizes=[3, 3, 3], conv_type="resnet", link_type="conv", upscale_type="transpose",
              norm_type="instance", padding=1, dropout_param=0.0,
              activation_fn=activation_factory["swish"])
    torch.manual_seed(0)
    net = DiffusionUNet(**kw).to(dev).eval()
    d = Diffusion(noise_steps=1000, img_size=(16, 16, 8))
    dt = {k: getattr(d, k).to(dev) for k in ("beta", "alpha", "alpha_bar")}
    x = torch.randn((2, 1, 16, 16, 8), generator=g).to(dev)
    noise = torch.randn((2, 1, 16, 16, 8), generator=g).to(dev)
    d.randn_like = lambda v: noise
    cls = torch.tensor([0, 2], device=dev)
    tt = torch.full((1,), 0.5, device=dev)

    def hip_step():
        with torch.no_grad():
            return d.step(x, net(x, tt, cls), 500, epsilon_uncond=net(x, tt), scale=3.0)

    def ref_step():
        with torch.no_grad():
            return torch_step("ddpm", dt, x, net(x, tt, cls), net(x, tt), 3.0, noise, 500)

    compare("sample_step_ddpm", hip_step, ref_step, args, {"shape": [2, 1, 16, 16, 8]})


if __name__ == "__main__":
    main()
