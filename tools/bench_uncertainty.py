#!/usr/bin/env python3
"""Time of the bootstrap AUC interval and of the adaptive-prediction-set kernel on the GPU.

    python tools/bench_uncertainty.py [--iters 5] [--warmup 1] [--big-iters 3]

  * ``bootstrap``: ``utils.bootstrap_metrics.bootstrap_metric`` on a ``BinaryAUROC`` /
    ``MulticlassAUROC(3)`` holding n = 2000 scores on the device, R = 100 and R = 10 000 resamples of
    half the set (the two settings of the reference's classification test entrypoint). ``fast``: the
    one-launch-per-class path. ``loop``: the reference's loop over the same metric -- reset, update and
    compute once per resample, through a thin object that lends the metric the ``preds`` / ``target``
    names -- which is what the package could do before the fast path. Both sides make the same draw
    (R ``torch.randperm`` calls on the host), timed alone as ``draw``; ``fast_given_rows`` is the fast
    path on index rows drawn beforehand. Wall-clock times of the whole call with a device
    synchronisation at the end, in milliseconds (median, min, max over the rounds).
  * ``aps``: ``functional.aps_cumulative`` with labels on ``[4096, 5]`` and ``[4096, 64]``
    probabilities, the kernel against the torch composite of the same rule on the same device.
    Device-event times of 10 back-to-back calls, divided by 10, in microseconds.
One JSON line per case. The machine is shared: the sides alternate within every round."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from adell_mri_amd import classification_metrics as CM  # noqa: E402
from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd.utils import bootstrap_metrics as B  # noqa: E402

N, SEED = 2000, 42


class AsReferenceMetric:
    """Lends an AUROC metric the names the reference's loop reads."""

    def __init__(self, metric):
        self.metric = metric
        self.preds, self.target = metric.scores, metric.labels

    def reset(self):
        self.metric.reset()

    def update(self, preds, target):
        self.metric.update(preds, target)

    def compute(self):
        return self.metric.compute()


def make_metric(classes, dev):
    g = torch.Generator().manual_seed(classes)
    y = torch.randint(0, classes, (N,), generator=g)
    if classes == 2:
        s = torch.sigmoid(torch.randn(N, generator=g) + (2.0 * y - 1.0))
        metric = CM.BinaryAUROC()
    else:
        s = torch.softmax(torch.randn((N, classes), generator=g)
                          + 1.5 * torch.nn.functional.one_hot(y, classes), -1)
        metric = CM.MulticlassAUROC(classes)
    metric.update(s.to(dev), y.to(dev))
    return metric


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def summary(ts, digits=3):
    return {"median": round(statistics.median(ts), digits), "min": round(min(ts), digits),
            "max": round(max(ts), digits)}


def bench_bootstrap(args, dev):
    for classes in (2, 3):
        for R in (100, 10000):
            iters = args.iters if R <= 100 else args.big_iters
            rows = B.draw_sample_idxs(N, R, N // 2, torch.Generator().manual_seed(SEED))
            sides = {
                "fast": lambda: B.bootstrap_metric(make_metric(classes, dev), samples=R, seed=SEED),
                "loop": lambda: B.bootstrap_metric(AsReferenceMetric(make_metric(classes, dev)),
                                                   samples=R, seed=SEED),
                "fast_given_rows": lambda: B.bootstrap_metric(make_metric(classes, dev),
                                                              sample_idxs=rows),
                "draw": lambda: B.draw_sample_idxs(N, R, N // 2,
                                                   torch.Generator().manual_seed(SEED)),
            }
            for _ in range(args.warmup):
                for k, fn in sides.items():
                    if R <= 100 or k != "loop":
                        fn()
            times, outs = {k: [] for k in sides}, {}
            for _ in range(iters):
                for k, fn in sides.items():
                    ms, outs[k] = wall(fn)
                    times[k].append(ms)
            line = {"case": "bootstrap", "classes": classes, "n": N, "R": R, "m": N // 2, "rounds": iters}
            for k, t in times.items():
                line[k + "_ms"] = summary(t)
            line["loop_over_fast"] = round(statistics.median(times["loop"])
                                           / statistics.median(times["fast"]), 2)
            line["fast_max_below_loop_min"] = bool(max(times["fast"]) < min(times["loop"]))
            line["loop_max_below_fast_min"] = bool(max(times["loop"]) < min(times["fast"]))
            line["max_abs_difference"] = max(
                float((outs["fast"][i].double() - outs["loop"][i].double()).abs().max())
                for i in range(2))
            print(json.dumps(line), flush=True)


def events(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, out


def composite(p, y):
    cum = HF._aps_cumulative_composite(p)
    return cum, torch.take_along_dim(cum, y[:, None], 1)[:, 0]


def bench_aps(args, dev):
    g = torch.Generator().manual_seed(1)
    for n, C in ((4096, 5), (4096, 64)):
        p = torch.softmax(torch.randn((n, C), generator=g) * 2, -1).to(dev)
        y = torch.randint(0, C, (n,), generator=g).to(dev)
        sides = {"kernel": lambda: HF.aps_cumulative(p, y), "composite": lambda: composite(p, y)}
        for _ in range(max(args.warmup, 2)):
            for fn in sides.values():
                fn()
        times, outs = {k: [] for k in sides}, {}
        for _ in range(max(args.iters, 10)):
            for k, fn in sides.items():
                us, outs[k] = events(fn, 10)
                times[k].append(us)
        line = {"case": "aps", "shape": [n, C], "rounds": max(args.iters, 10)}
        for k, t in times.items():
            line[k + "_us"] = summary(t, 2)
        line["composite_over_kernel"] = round(statistics.median(times["composite"])
                                              / statistics.median(times["kernel"]), 2)
        line["kernel_max_below_composite_min"] = bool(max(times["kernel"]) < min(times["composite"]))
        line["composite_max_below_kernel_min"] = bool(max(times["composite"]) < min(times["kernel"]))
        line["mismatches"] = int((outs["kernel"][0] != outs["composite"][0]).sum()
                                 + (outs["kernel"][1] != outs["composite"][1]).sum())
        print(json.dumps(line), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--big-iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    bench_aps(args, dev)
    bench_bootstrap(args, dev)


if __name__ == "__main__":
    main()
