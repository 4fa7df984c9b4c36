#!/usr/bin/env python3
"""Time of the ensemble and Gaussian-process kernels (csrc/ensemble.hip) and of one ensemble training
step against the same arithmetic composed from torch ops, in fp32 on the same GPU.

    python tools/bench_ensemble.py [--iters 30] [--warmup 3] [--inner 20]

Two shapes each: the smallest test shape and a workload-like one (three members of 512 features,
r = 1024 random features, N = 32 rows).
  * ``gp_phi``: ``functional.gp_phi`` forward plus backward (one launch, then at most two) against
    ``layer_norm`` / ``matmul`` / ``cos`` / ``matmul`` and autograd.
  * ``gp_precision_update``: one launch in place against ``einsum("n,ni,nj->ij")`` and ``add_``.
  * ``gp_variance``: against ``(phi @ cov * phi).sum(-1)``.
  * ``gp_sample``: samples, their mean and unbiased std in one launch against the three torch calls.
  * ``ensemble_pool``: forward plus backward against ``flatten(2).max(-1).values`` per member and
    ``concat``.
  * ``ensemble_average``: forward plus backward against ``sum / K`` and sigmoid / softmax.
  * ``training_step``: ``GenericEnsemblePL.training_step`` plus backward of the fixture network
    ``gen2d_gp32`` (tests/ensemble_cases.py) and of a workload-like ensemble (three 2-D U-Net
    encoders of 512 features, r = 1024, 32 items) with the fused pooling and head, against the same module
    with ``functional.ensemble_pool`` and the head's ``forward_with_phi`` replaced by the torch
    expressions (the encoders are the same HIP kernels on both sides).
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds): end-to-end times of the whole call, launch, autograd and
allocation included. These kernels are small and launch-bound: what they remove is launches,
intermediates and host reads."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd import ops  # noqa: E402

GP_SHAPES = [(5, 24, 130, 3), (32, 512, 1024, 2)]          # (N, i, r, o)
POOLS = [[(2, 5, 3, 7), (2, 130, 2, 3, 5), (2, 33)], [(32, 512, 4, 4, 2)] * 3]
AVERAGES = [(3, 5, 1), (3, 32, 3)]                          # (K, B, C)


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, out


def compare(name, hip, ref, args, extra):
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
        "torch_max_below_hip_min": bool(max(t_ref) < min(t_hip)),
        "max_abs_difference": float((out_hip.double() - out_ref.double()).abs().max())}), flush=True)


def fwd_bwd(fn, leaves, weight):
    """Forward plus backward of ``fn`` on fresh leaves; returns the first leaf's gradient."""
    def run():
        ls = [t.detach().requires_grad_(True) for t in leaves]
        out = fn(*ls)
        out = out if isinstance(out, tuple) else (out,)
        sum((o * w).sum() for o, w in zip(out, weight)).backward()
        return ls[0].grad
    return run


def torch_gp(W, b, scale):
    def fn(x, gamma, beta, weights):
        phi = scale * torch.cos(b - F.layer_norm(x, x.shape[-1:], gamma, beta, 1e-5) @ W[0].T)
        return phi @ weights.T, phi
    return fn


def torch_pool(*members):
    return torch.concat([m.flatten(start_dim=2).max(-1).values if m.dim() > 2 else m
                         for m in members], 1)


def torch_average(*logits):
    mean = sum(logits) / len(logits)
    return torch.sigmoid(mean) if mean.shape[1] == 1 else torch.softmax(mean, 1)


def channels_last(t):
    if t.dim() == 4:
        return t.contiguous(memory_format=torch.channels_last)
    return t.contiguous(memory_format=torch.channels_last_3d) if t.dim() == 5 else t


def bench_kernels(args, dev):
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(s, generator=g).to(dev)  # noqa: E731
    for N, i, r, o in GP_SHAPES:
        extra = {"shape": [N, i, r, o]}
        x, gamma, beta, weights = rn(N, i), 1 + 0.3 * rn(i), 0.2 * rn(i), rn(o, r) / r ** 0.5
        W, b = rn(1, r, i) * (2.0 / i) ** 0.5, torch.rand((1, r), generator=g).to(dev) * 6.28
        scale = (2.0 / r) ** 0.5
        wl, wp = rn(N, o), rn(N, r)
        compare("gp_phi", fwd_bwd(lambda x_, g_, b_, w_: HF.gp_phi(x_, g_, b_, W, b, w_, scale),
                                  [x, gamma, beta, weights], [wl, wp]),
                fwd_bwd(torch_gp(W, b, scale), [x, gamma, beta, weights], [wl, wp]), args, extra)
        with torch.no_grad():
            phi = HF.gp_phi(x, gamma, beta, W, b, weights, scale)[1]
        prob = torch.softmax(rn(N, 3), 1)
        P_hip, P_ref = (torch.eye(r, device=dev)[None].contiguous() for _ in range(2))

        def update_ref():
            c = (prob * (1 - prob)).sum(-1)
            P_ref.add_(torch.einsum("n,ni,nj->ij", c, phi, phi)[None])
            return P_ref

        compare("gp_precision_update", lambda: ops.gp_precision_update(P_hip, phi, prob), update_ref,
                args, extra)
        cov = torch.linalg.inv(P_ref[0].double()).float()[None].contiguous()
        compare("gp_variance", lambda: ops.gp_variance(phi, cov),
                lambda: ((phi @ cov[0]) * phi).sum(-1), args, extra)
        mean, var = rn(N, o), ops.gp_variance(phi, cov)
        for S in (7, 100):
            eps = rn(S, N, o)

            def sample_ref():
                s = mean[None] + var.clamp_min(0).sqrt()[None, :, None] * eps
                return torch.stack([s.mean(0), s.std(0)])

            compare("gp_sample", lambda: torch.stack(ops.gp_sample(mean, var, eps)[1:]), sample_ref,
                    args, dict(extra, samples=S))
    for shapes in POOLS:
        members = [channels_last(rn(*s)) for s in shapes]
        w = rn(shapes[0][0], sum(s[1] for s in shapes))
        compare("ensemble_pool", fwd_bwd(lambda *m: HF.ensemble_pool(list(m)), members, [w]),
                fwd_bwd(torch_pool, members, [w]), args, {"shapes": [list(s) for s in shapes]})
    for K, B, C in AVERAGES:
        logits, w = [rn(B, C) for _ in range(K)], rn(B, C)
        compare("ensemble_average", fwd_bwd(lambda *t: HF.ensemble_average(list(t)), logits, [w]),
                fwd_bwd(torch_average, logits, [w]), args, {"shape": [K, B, C]})


def small_step_network(dev):
    """The fixture network ``gen2d_gp32`` and a batch [4, 1, 16, 16]."""
    import ensemble_cases as C
    from test_ensemble import build_pl

    name = "gen2d_gp32"
    net, _ = build_pl(name)
    net.load_state_dict(C.fill(net.state_dict(), 2.0))
    g = torch.Generator().manual_seed(1)
    batch = {"image": torch.rand(C.input_shape(name), generator=g).to(dev),
             "label": torch.tensor(C.CONFIGS[name][5]).to(dev)}
    return name, net.to(dev).train(), batch


def workload_step_network(dev):
    """Three 2-D ``UNet(depth=[32, 128, 512], encoder_only=True)`` members of 512 features each, a
    head of 1536 -> 512 and a Gaussian-process layer of r = 1024 on N = 32 items [32, 1, 32, 32]."""
    from adell_mri_amd.modules.activations import activation_factory
    from adell_mri_amd.modules.classification.pl import GenericEnsemblePL
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.segmentation.unet import UNet

    torch.manual_seed(0)
    members = [UNet(spatial_dimensions=2, in_channels=1, depth=[32, 128, 512], kernel_sizes=[3, 3, 3],
                    strides=[2, 2, 2], dropout_param=0.0, activation_fn=activation_factory["swish"],
                    encoder_only=True) for _ in range(3)]
    net = GenericEnsemblePL(image_keys=["image"], spatial_dimensions=2, networks=members,
                            n_features=[512, 512, 512], head_structure=[512], n_classes=2,
                            head_adn_fn=get_adn_fn(1, "batch", "swish", 0.0), gaussian_process=True,
                            gp_n_rff=1024)
    g = torch.Generator().manual_seed(1)
    batch = {"image": torch.rand((32, 1, 32, 32), generator=g).to(dev),
             "label": (torch.rand((32,), generator=g) > 0.5).float().to(dev)}
    return "3 x 512 features, r = 1024, N = 32", net.to(dev).train(), batch


def bench_step(args, dev, build):
    """One training step (forward, loss, backward), fused against composed."""
    name, net, batch = build(dev)
    head = net.gaussian_process_head
    fused = (HF.ensemble_pool, head.forward_with_phi)

    def composed_head(X):
        return torch_gp(head.W, head.b, head._scale)(X, head.input_norm.weight, head.input_norm.bias,
                                                     head.weights)

    def step(fused_path):
        def run():
            HF.ensemble_pool, head.forward_with_phi = fused if fused_path else (
                lambda members: torch_pool(*members), composed_head)
            try:
                net.zero_grad()
                loss = net.training_step(batch, 0)
                loss.backward()
            finally:
                HF.ensemble_pool, head.forward_with_phi = fused
            return loss.detach()
        return run

    compare("training_step", step(True), step(False), args, {"network": name})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    bench_kernels(args, dev)
    bench_step(args, dev, small_step_network)
    bench_step(args, dev, workload_step_network)


if __name__ == "__main__":
    main()
