#!/usr/bin/env python3
"""Time of the masked autoencoder's token plumbing and loss on the fused kernels
(functional.mae_keep_tokens + functional.mae_restore_tokens, functional.mae_reconstruction_loss;
csrc/mae.hip) against the plain-torch composition of the reference's arithmetic (tests/mae_ref.py, in
fp32 on the same GPU).

    python tools/bench_mae.py [--iters 30] [--warmup 3] [--inner 10]

A ViT-B/16-like shape: 14 x 14 = 196 tokens of 256 features (16 x 16 patches of one channel), 49 kept
(mask_fraction 0.75), batch 8 and batch 2. Per case three JSON lines:
  * ``keep_restore``: forward plus backward of keep followed by restore (the encoder between them
    left out: the kept rows go straight back), with the gradients of the tokens, the mask token, its
    scale and the positional embedding; torch: ``gather`` / ``repeat`` / ``cat`` / ``gather`` / add;
  * ``loss_c1`` / ``loss_c2``: forward plus backward of the reconstruction loss for one channel
    (pred [B, 196, 256] against [B, 1, 224, 224]) and two (pred [B, 196, 512] against [B, 2, 224,
    224]); torch: ``view`` / ``permute`` / ``contiguous`` / ``view`` / ``mse_loss``.
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds), and the bytes the algorithm needs over the HIP time -- an
end-to-end rate of the whole call, launches and autograd included, not a kernel's share of peak.
keep_restore: x rows read and dx written (B L E each, the kept quarter of x), the kept rows written
and read again as enc, out written, dout read twice (denc / dpos, masked sums), denc written, pos
and dpos; loss: pred read twice, x read twice, dpred written."""
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

# (B, L, E, K)
CASES = [(8, 196, 256, 49), (2, 196, 256, 49)]
IMAGE = (224, 224)


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
    for B, L, E, K in CASES:
        rng = np.random.default_rng(0)
        ids = np.argsort(rng.uniform(size=[B, L]), axis=1, kind="stable")
        # a fixed shuffle: one upload (a training step uploads one per forward)
        shuffle = ops.MaeShuffle(ids, K, dev)
        ids_t = torch.from_numpy(ids).to(dev)
        ids_keep = ids_t[:, :K].unsqueeze(-1).repeat(1, 1, E)
        ids_restore = torch.argsort(ids_t, dim=1, stable=True).unsqueeze(-1).expand(-1, -1, E)
        x = (torch.rand((B, L, E), generator=g) * 2 - 1).to(dev).requires_grad_(True)
        pos = torch.rand((1, L, E), generator=g).to(dev).requires_grad_(True)
        token = (torch.rand((1, 1, E), generator=g) - 0.5).to(dev).requires_grad_(True)
        scale = torch.tensor([0.75], device=dev, requires_grad=True)
        w = (torch.rand((B, L, E), generator=g) * 2 - 1).to(dev)
        shape = {"B": B, "L": L, "E": E, "K": K}
        leaves = (x, pos, token, scale)

        def clear(ts):
            for t in ts:
                t.grad = None

        def hip_tokens():
            clear(leaves)
            kept = HF.mae_keep_tokens(x, shuffle)
            out = HF.mae_restore_tokens(kept, token, scale, pos, shuffle)
            (out * w).sum().backward()
            return (token.grad.sum() + scale.grad.sum()).detach()

        def ref_tokens():
            clear(leaves)
            kept = torch.gather(x, 1, ids_keep)
            full = torch.cat([kept, scale * token.repeat(B, L - K, 1)], dim=1)
            out = torch.gather(full, 1, ids_restore) + pos
            (out * w).sum().backward()
            return (token.grad.sum() + scale.grad.sum()).detach()

        nbytes = 4 * E * (2 * B * K + 2 * B * K + B * L + 2 * B * L + B * K + B * L + 2 * L)
        compare("keep_restore", hip_tokens, ref_tokens, nbytes, args, shape)

        for C in (1, 2):
            P = E
            pred = (torch.rand((B, L, P * C), generator=g) * 2 - 1).to(dev).requires_grad_(True)
            image = (torch.rand((B, C, *IMAGE), generator=g) * 2 - 1).to(dev)
            assert L * P == IMAGE[0] * IMAGE[1]

            def hip_loss():
                pred.grad = None
                loss = HF.mae_reconstruction_loss(pred, image, P)
                loss.backward()
                return loss.detach()

            def ref_loss():
                pred.grad = None
                recon = pred.view(B, L, 16, 16, C).permute(0, 4, 1, 2, 3).contiguous().view(
                    B, C, *IMAGE)
                loss = torch.nn.functional.mse_loss(recon, image)
                loss.backward()
                return loss.detach()

            compare(f"loss_c{C}", hip_loss, ref_loss, 4 * 5 * B * L * P * C, args,
                    {"B": B, "C": C, "L": L, "P": P})


if __name__ == "__main__":
    main()
