"""Timing of windowed attention beyond the small-window kernel (csrc/tokens.hip): forward, backward
(dQ + dK/dV) and the bias-gradient kernel with a per-head relative-position bias and region labels,
event-timed means over ``--iters`` calls after a warm-up, at
  (W = 64 windows, H = 2, T = 216, 32 / 32) and (W = 64, H = 1, T = 512, 32 / 32),
and for the first shape the same three calls on the dense-mask route (rel[None] + mask[:, None] as a
[W * H, T, T] bias, nbias = W * H, plus the sum of that gradient over the windows).
Prints one JSON line per shape."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1e3 / iters, 1)


def shape(W, H, T, A, iters, dense):
    from adell_mri_amd import ops

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    q, k, v, do = (torch.randn(W * H, T, A, generator=g).to(dev) for _ in range(4))
    rel = torch.randn(H, T, T, generator=g).to(dev)
    lab = torch.randint(0, 4, (W, T), generator=g, dtype=torch.int32).to(dev)
    scale = A ** -0.5
    out, lse = ops.attention_fwd(q, k, v, rel, scale, labels=lab, heads=H)
    res = {"W": W, "H": H, "T": T, "A": A, "Dv": A, "iters": iters,
           "plan": [ops.attention_plan(T, A, A, w).path for w in ("fwd", "dq", "dkv")],
           "labels_us": {
               "fwd": timed(lambda: ops.attention_fwd(q, k, v, rel, scale, labels=lab, heads=H), iters),
               "bwd": timed(lambda: ops.attention_bwd(q, k, v, rel, out, do, lse, scale, labels=lab,
                                                      heads=H), iters),
               "bias_grad": timed(lambda: ops.attention_bias_grad(q, k, v, rel, out, do, lse, scale, H,
                                                                  labels=lab, heads=H), iters)}}
    if dense:
        mask = torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0)
        bias = (rel[None] + mask[:, None]).reshape(W * H, T, T).contiguous()
        od, ld = ops.attention_fwd(q, k, v, bias, scale)

        def bias_grad():
            ds = ops.attention_bias_grad(q, k, v, bias, od, do, ld, scale, W * H)
            return ops.sum_bcast(ds, (H, T, T))

        res["dense_mask_us"] = {
            "bias_bytes": bias.numel() * 4,
            "fwd": timed(lambda: ops.attention_fwd(q, k, v, bias, scale), iters),
            "bwd": timed(lambda: ops.attention_bwd(q, k, v, bias, od, do, ld, scale), iters),
            "bias_grad": timed(bias_grad, iters)}
    print(json.dumps(res))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("window_attention_time.py needs a GPU")
    shape(64, 2, 216, 32, a.iters, dense=True)
    shape(64, 1, 512, 32, a.iters, dense=False)
