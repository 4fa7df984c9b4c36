"""Timing of the PI-CAI evaluation (csrc/components.hip, modules/segmentation/picai_eval.py).

  loop:     N x PicaiEval.update + one compute on 2 x 128^3 cases with realistic lesion masks (a few
            spherical GT lesions; a smooth prediction with matching blobs, a miss and false
            positives); run it under ``rocprofv3 --kernel-trace --stats`` for the per-kernel times,
            the script prints the wall time per update and the labelling time alone;
            It also times the labelling of 4 x 128^3 volumes that are one component each (all
            ones, and one box over half of the volume), the worst case of the cross-tile merge;
  validate: validate_steps of a config-2 module (bench.build_module) on 2 x 128^3 batches with
            picai_eval off and on, interleaved; prints ms per case of each side."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cases(dev, B=2, S=128, seed=0):
    g = torch.Generator().manual_seed(seed)
    ax = torch.arange(S, dtype=torch.float32)
    zz, yy, xx = torch.meshgrid(ax, ax, ax, indexing="ij")
    pred = torch.zeros((B, S, S, S))
    target = torch.zeros((B, S, S, S))
    for b in range(B):
        for k in range(6):
            c = torch.randint(12, S - 12, (3,), generator=g).float()
            r = 4 + 6 * torch.rand(1, generator=g).item()
            d2 = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2
            if k < 4:
                target[b][d2 <= r * r] = 1.0
            if k != 0:                     # lesion 0 missed; 4 and 5 false positives
                pred[b] = torch.maximum(pred[b], torch.exp(-d2 / (0.5 * r * r)))
        pred[b] += 0.12 * torch.rand((S, S, S), generator=g) ** 200    # a few hundred specks
    return pred.clamp(0, 1).to(dev), target.to(dev)


def loop(n):
    from adell_mri_amd import ops
    from adell_mri_amd.modules.segmentation.picai_eval import PicaiEval

    dev = torch.device("cuda:0")
    p, y = cases(dev)
    acc = PicaiEval()
    for _ in range(5):
        acc.update(p, y)
    acc.compute()
    acc.reset()
    both = torch.cat([p, y])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        ops.label_components(both, 0.1)
    e1.record()
    torch.cuda.synchronize()
    us_label = e0.elapsed_time(e1) * 1e3 / n
    big = {}
    for name in ("all_ones", "half_box"):
        v = torch.zeros((4, 128, 128, 128), device=dev)
        if name == "all_ones":
            v.fill_(1.0)
        else:
            v[:, :64, :, :] = 1.0
            v[:, 64:, 10:118, 10:118] = (torch.rand((4, 64, 108, 108), device=dev) > 0.999).float()
        ops.label_components(v)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(n):
            ops.label_components(v)
        e1.record()
        torch.cuda.synchronize()
        big[f"us_label_4_volumes_{name}"] = round(e0.elapsed_time(e1) * 1e3 / n, 2)
    t0 = time.perf_counter()
    for _ in range(n):
        acc.update(p, y)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    vals = acc.compute()
    t2 = time.perf_counter()
    m = acc.metrics()
    print(json.dumps({"updates": n, "us_per_update_wall": round((t1 - t0) * 1e6 / n, 2),
                      "us_label_4_volumes": round(us_label, 2),
                      "ms_compute_all": round((t2 - t1) * 1e3, 3),
                      "cases": len(acc), "y_list_case0": len(m.lesion_results[0]),
                      "bytes_read_per_update": p.numel() * 8, **big, **vals}))


def validate(batches, rounds):
    import bench
    from adell_mri_amd import trainer

    dev = torch.device("cuda:0")
    net, _ = bench.build_module(dev)
    data = [bench.synthetic_batch(2, 128, dev, s) for s in range(batches)]
    for on in (False, True):
        net.picai_eval = on
        trainer.validate_steps(net, data[:1])
    torch.cuda.synchronize()
    res = {False: [], True: []}
    out = {}
    for _ in range(rounds):
        for on in (False, True):
            net.picai_eval = on
            t0 = time.perf_counter()
            out = trainer.validate_steps(net, data)
            res[on].append((time.perf_counter() - t0) * 1e3 / (2 * batches))
    off, on = sorted(res[False]), sorted(res[True])
    print(json.dumps({"ms_per_case_off": off, "ms_per_case_on": on,
                      "median_delta_ms": round(on[len(on) // 2] - off[len(off) // 2], 3),
                      "V_AP": out.get("V_AP"), "V_AUC": out.get("V_AUC")}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["loop", "validate"])
    ap.add_argument("--n", type=int, default=50)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    loop(a.n) if a.mode == "loop" else validate(a.batches, a.rounds)
