#!/usr/bin/env python3
"""Time of the multiple-instance kernels (csrc/mil.hip) against the plain-torch expressions they
replace, forward plus backward, in fp32 on the same GPU.

    python tools/bench_mil.py [--iters 30] [--warmup 3] [--inner 20]

  * ``volume_to_slices``: ``functional.volume_to_slices`` against
    ``x.permute(0, 4, 1, 2, 3).contiguous().view(B * S, C, H, W)`` at [8, 1, 256, 256, 24] and
    [4, 1, 16, 16, 8]; each direction reads and writes the batch once: 4 numel floats in all.
  * ``gated_pool`` (the three modes, with the gate) and ``plain_pool`` ("mean" without it):
    ``functional.mil_gated_pool`` against ``softmax(W(tanh(hv) * sigmoid(hu)), -2)`` and the
    reference's pooling expression at (B, S, N = F) = (8, 24, 512) and (4, 8, 16).
  * ``slice_tokens``: ``functional.slice_tokens`` against ``cat([class_token.expand, x + pos], 1)`` at
    [8, 24, 512] and [4, 8, 16].
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds). For the transpose also the bytes the algorithm needs over
the time: an end-to-end rate of the whole call, launch, autograd and allocation included, not a
kernel's share of peak. The pooling and token cases are launch-bound at these sizes: their times are
launch and autograd overhead, not arithmetic."""
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

VOLUMES = [(8, 1, 256, 256, 24), (4, 1, 16, 16, 8)]
ROWS = [(8, 24, 512), (4, 8, 16)]


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


def fwd_bwd(fn, leaves, weight):
    """Forward plus backward of ``fn`` on fresh leaves; the outputs are weighted by ``weight`` so that
    every incoming gradient differs from 1. Returns the first leaf's gradient."""
    def run():
        ls = [t.detach().requires_grad_(True) for t in leaves]
        out = fn(*ls)
        out = out if isinstance(out, tuple) else (out,)
        sum((o * w).sum() for o, w in zip(out, weight)).backward()
        return ls[0].grad
    return run


def torch_pool(mode):
    def fn(feat, hv, hu, w, b):
        A = F.softmax(F.linear(torch.tanh(hv) * torch.sigmoid(hu), w[None], b), -2)
        if mode == "mean":
            return torch.sum(feat * A, -2), A
        if mode == "max":
            return torch.max(feat * A, -2).values, A
        return (F.softmax(feat, dim=-1) * A).sum(-2), A
    return fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mil.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for shape in VOLUMES:
        B, C, H, W, S = shape
        x = torch.rand(shape, generator=g).to(dev)
        wy = torch.rand((B * S, C, H, W), generator=g).to(dev)
        compare("volume_to_slices", fwd_bwd(HF.volume_to_slices, [x], [wy]),
                fwd_bwd(lambda t: t.permute(0, 4, 1, 2, 3).contiguous().view(B * S, C, H, W), [x],
                        [wy]), args, {"shape": list(shape)}, nbytes=4 * x.numel() * 4)
    for B, S, E in ROWS:
        feat, hv, hu = (torch.randn((B, S, E), generator=g).to(dev) for _ in range(3))
        w, b = torch.randn((E,), generator=g).to(dev), torch.randn((1,), generator=g).to(dev)
        wp, wA = torch.rand((B, E), generator=g).to(dev), torch.rand((B, S, 1), generator=g).to(dev)
        extra = {"shape": [B, S, E]}
        for mode in ("mean", "max", "vocabulary"):
            compare(f"gated_pool_{mode}",
                    fwd_bwd(lambda *t, m=mode: HF.mil_gated_pool(*t, mode=m), [feat, hv, hu, w, b],
                            [wp, wA]),
                    fwd_bwd(torch_pool(mode), [feat, hv, hu, w, b], [wp, wA]), args, extra)
        compare("plain_pool_mean",
                fwd_bwd(lambda t: HF.mil_gated_pool(t, mode="mean")[0], [feat], [wp]),
                fwd_bwd(lambda t: torch.sum(t * (torch.ones([B, S, 1], device=dev) / S), -2), [feat],
                        [wp]), args, extra)
        pos = torch.randn((1, S, 1), generator=g).to(dev)
        ct = torch.randn((1, 1, E), generator=g).to(dev)
        wt = torch.rand((B, S + 1, E), generator=g).to(dev)
        compare("slice_tokens", fwd_bwd(HF.slice_tokens, [feat, pos, ct], [wt]),
                fwd_bwd(lambda x, p, c: torch.cat([c.expand(B, 1, E), x + p], 1), [feat, pos, ct],
                        [wt]), args, extra)


if __name__ == "__main__":
    main()
