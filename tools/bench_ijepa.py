#!/usr/bin/env python3
"""Time of I-JEPA's token plumbing and loss on the fused kernels (functional.predictor_tokens,
functional.ijepa_block_loss; csrc/ijepa.hip) against the plain-torch composition of the reference's
arithmetic (tests/ijepa_ref.py, in fp32 on the same GPU).

    python tools/bench_ijepa.py [--iters 30] [--warmup 3] [--inner 10]

The UNETR shape of configs/unetr.yaml: 6^3 = 216 tokens of 512 features, batch 8 and batch 2, 54
context tokens and four target blocks of 27 tokens each. Per case two JSON lines:
  * ``predictor_input``: forward plus backward of the predictor's input for the four blocks (the
    gradients of the embedded context, the positional embedding and the mask token);
  * ``block_losses``: forward plus backward of the loss of the four blocks from the teacher's raw
    output [B, 216, 512] (the composition normalises all of it once, then gathers four times).
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds), and the bytes the algorithm needs over the HIP time -- an
end-to-end rate of the whole call, launches and autograd included, not a kernel's share of peak.
predictor_input: per block 4 B (nc + nt) P floats (out written, dout read, e read, de written, less
the target rows of e / de) plus pos rows and the whole dpos; block_losses: per block pred read twice,
dpred written, the target rows of h read twice."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd import ops  # noqa: E402

# (B, T, E, nc, nt, blocks)
CASES = [(8, 216, 512, 54, 27, 4), (2, 216, 512, 54, 27, 4)]


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
        "hip_max_below_torch_min": bool(max(t_hip) < min(t_ref)),
        "torch_max_below_hip_min": bool(max(t_ref) < min(t_hip)),
        "algorithm_bytes": nbytes, "hip_gb_per_s": round(nbytes / med / 1e3, 1),
        "result_hip": float(out_hip), "result_torch": float(out_ref)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    for B, T, E, nc, nt, blocks in CASES:
        rng = np.random.default_rng(0)
        order = rng.permutation(T)
        ctx = np.sort(order[:nc])
        tgts = [np.sort(order[nc + i * nt:nc + (i + 1) * nt]) for i in range(blocks)]
        # fixed index sets: one upload each, as the table cache keeps them
        ctx_rows = ops.token_rows(ctx, T, dev)
        tgt_rows = [ops.token_rows(t, T, dev) for t in tgts]
        ctx_t = torch.from_numpy(ctx).to(dev)
        tgt_t = [torch.from_numpy(t).to(dev) for t in tgts]
        e = (torch.rand((B, nc, E), generator=g) * 2 - 1).to(dev).requires_grad_(True)
        pos = torch.rand((1, T, E), generator=g).to(dev).requires_grad_(True)
        mask = torch.rand((1, 1, E), generator=g).to(dev).requires_grad_(True)
        w = [(torch.rand((B, nc + nt, E), generator=g) * 2 - 1).to(dev) for _ in range(blocks)]
        h = ((torch.rand((B, T, E), generator=g) * 2 - 1) *
             (0.5 + 3.5 * torch.rand((B, T, 1), generator=g))).to(dev)
        preds = [(torch.rand((B, nt, E), generator=g) * 4 - 2).to(dev).requires_grad_(True)
                 for _ in range(blocks)]
        shape = {"B": B, "T": T, "E": E, "nc": nc, "nt": nt, "blocks": blocks}

        def clear():
            for t in (e, pos, mask, *preds):
                t.grad = None

        def hip_input():
            clear()
            total = sum((HF.predictor_tokens(e, pos, mask, ctx_rows, r) * wi).sum()
                        for r, wi in zip(tgt_rows, w))
            total.backward()
            return mask.grad.sum().detach()

        def ref_input():
            clear()
            total = 0
            for t, wi in zip(tgt_t, w):
                x = e + pos[:, ctx_t, :]
                m = (mask + pos[:, t, :]).expand(B, -1, -1)
                total = total + (torch.cat([x, m], dim=1) * wi).sum()
            total.backward()
            return mask.grad.sum().detach()

        nbytes = 4 * blocks * (2 * B * (nc + nt) * E + 2 * B * nc * E + (nc + nt) * E + T * E)
        compare("predictor_input", hip_input, ref_input, nbytes, args, shape)

        def hip_loss():
            clear()
            loss = torch.stack([HF.ijepa_block_loss(p, h, r) for p, r in zip(preds, tgt_rows)]).mean()
            loss.backward()
            return loss.detach()

        def ref_loss():
            clear()
            hn = torch.nn.functional.layer_norm(h, (E,))
            crit = torch.nn.SmoothL1Loss()
            loss = torch.stack([crit(p, hn[:, t]) for p, t in zip(preds, tgt_t)]).mean()
            loss.backward()
            return loss.detach()

        compare("block_losses", hip_loss, ref_loss, 4 * blocks * 5 * B * nt * E, args, shape)


if __name__ == "__main__":
    main()
