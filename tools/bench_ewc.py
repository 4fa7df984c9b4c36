#!/usr/bin/env python3
"""Cost of the elastic-weight-consolidation penalty over the REAL parameter lists of BASELINE config 2
(the 3-D U-Net, 8.26 M parameters) and config 3 (UNETR, 36.1 M), p = 2:

  * autograd route: ``ewc(model)`` forward + backward (3 launches);
  * fused route: ``ewc.add_to_optimizer`` into the flat gradient slots of a FusedSGD (2 + groups);
  * the same arithmetic with plain torch operators on the same GPU, per parameter, as the reference
    writes it (``out = out.add(torch.norm(param - anchor, p=p))``), forward + backward, once with
    ``.grad`` unset (set_to_none) and once accumulating into existing gradients.

Each figure is wall time per call: the median over ``--runs`` windows (>= 20) of ``--inner`` calls each,
a window ended by one device synchronise, after ``--warmup`` calls; the variants alternate window by
window. It is host enqueue time plus device time -- dominated by the host's enqueue for the torch loop
-- which is what a launch-bound term costs a training step; it is not kernel time. Device launches
are counted with torch's profiler in a run of its own. Needs a GPU; prints one JSON line.

    python tools/bench_ewc.py [--runs 30] [--inner 10] [--warmup 5] [--configs 2,3]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parameter_shapes(config):
    """name -> shape of the config's network, built on the CPU through the entry point's factory."""
    import torch

    import bench

    if config == 2:
        net, _ = bench.build_module("cpu")
    else:
        from adell_mri_amd.modules.config_parsing import parse_config_unet
        from adell_mri_amd.utils.network_factories import get_segmentation_network

        cfg, _ = parse_config_unet(os.path.join(bench.CONFIGS_DIR, "unetr.yaml"), 1, 2)
        cfg["patch_size"] = [16, 16, 16]
        torch.manual_seed(0)
        net = get_segmentation_network("unetr", cfg, False, [], [], None, None, None, 100, [None], False,
                                       None, None, None, False, 2, ["image"],
                                       random_crop_size=[96, 96, 96])
    return {k.replace(".", "_"): tuple(p.shape) for k, p in net.named_parameters()}


def timed(variants, runs, inner, warmup):
    """``variants``: name -> (prepare or None, fn). Windows of ``inner`` calls of one variant, the
    variants in turn, ``runs`` rounds; ``prepare`` runs untimed before each window."""
    import torch

    out = {name: [] for name in variants}
    for r in range(-1, runs):                      # round -1: the warm-up
        for name, (prepare, fn) in variants.items():
            if prepare is not None:
                prepare()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(warmup if r < 0 else inner):
                fn()
            torch.cuda.synchronize()
            if r >= 0:
                out[name].append(1e3 * (time.perf_counter() - t0) / inner)
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": runs,
                   "calls_per_window": inner} for name, v in out.items()}


def device_launches(fn):
    """Kernels one call of ``fn`` launches (torch's profiler; None if it records no device activity)."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e.device_type, "name", "") == "CUDA"
                and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return n or None
    except Exception as exc:       # the profiler is an aid: the timings do not depend on it
        print(f"profiler unavailable: {exc!r}", file=sys.stderr)
        return None


def bench_config(config, runs, inner, warmup, device):
    import torch

    from adell_mri_amd.modules.continuous_learning import ElasticWeightConsolidation
    from adell_mri_amd.optim import FusedSGD

    shapes = parameter_shapes(config)
    torch.manual_seed(config)
    model = torch.nn.Module()
    for k, s in shapes.items():
        model.register_parameter(k, torch.nn.Parameter(torch.randn(s, device=device)))
    params = dict(model.named_parameters())
    ewc = ElasticWeightConsolidation(model, p=2)
    opt = FusedSGD(model.parameters(), lr=1e-3)        # re-homes p.data, as every real run does
    with torch.no_grad():
        for q in params.values():
            q.add_(0.01 * torch.randn_like(q))
    anchors = {k: a.detach().clone() for k, a in ewc.anchor_parameters.items()}

    def ours():
        for q in params.values():
            q.grad = None
        ewc(model).backward()

    def fused():
        ewc.add_to_optimizer(model, opt, 1.0)

    def torch_route(set_to_none):
        def fn():
            if set_to_none:
                for q in params.values():
                    q.grad = None
            out = torch.zeros([1], device=device)
            for k, q in params.items():
                out = out.add(torch.norm(q - anchors[k], p=2))
            out.backward()
        return fn

    # the two routes compute the same thing (checked at the size that is timed)
    ours()
    mine = {k: q.grad.detach().clone() for k, q in params.items() if q.numel()}
    torch_route(True)()
    worst = max(float((g - params[k].grad).abs().max() / params[k].grad.abs().max())
                for k, g in mine.items())
    rec = {"tensors": len(shapes), "parameters": int(sum(q.numel() for q in params.values())),
           "max_grad_deviation_from_torch": worst}
    def slots():                                       # p.grad = the flat slots: torch accumulates
        opt.zero_grad(set_to_none=False)

    rec.update(timed({"hip_autograd": (None, ours), "hip_fused_add": (slots, fused),
                      "torch_set_to_none": (None, torch_route(True)),
                      "torch_accumulate": (slots, torch_route(False))}, runs, inner, warmup))
    print(f"config {config}: {json.dumps(rec)}", file=sys.stderr, flush=True)
    for name, fn in (("hip_autograd", ours), ("hip_fused_add", fused),
                     ("torch_set_to_none", torch_route(True))):
        rec[name]["device_launches"] = device_launches(fn)
    return rec


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="2,3")
    args = ap.parse_args()
    if args.runs < 20:
        ap.error("--runs must be at least 20")
    if not torch.cuda.is_available():
        sys.exit("bench_ewc: needs a GPU (no CPU timing stands in for it)")
    device = torch.device("cuda:0")
    out = {f"config{c}": bench_config(int(c), args.runs, args.inner, args.warmup, device)
           for c in args.configs.split(",")}
    print(json.dumps({"bench": "ewc", "p": 2, **out}))


if __name__ == "__main__":
    main()
