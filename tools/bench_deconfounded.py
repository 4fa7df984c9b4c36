#!/usr/bin/env python3
"""Time of the deconfounded-classification kernels (csrc/deconfound.hip), forward plus backward, and
of one training step of fixture network (a), each against the same arithmetic in plain torch ops (the
reference's expressions) in fp32 on the same GPU.

    python tools/bench_deconfounded.py [--iters 20] [--warmup 3] [--inner 10]

Two sizes: ``(B, F, n_conf)`` = ``(4, 64, 8)`` (the default batch, a small extractor) and
``(32, 2048, 64)`` (a wide extractor); heads of 3 and 2 classes plus 2 regression outputs.
  * ``correlation_loss``: ``functional.deconf_correlation_loss`` against the wrapper's broadcast
    expression (pl.py:2396-2407), which materialises ``[B, n_conf, F - n_conf]``.
  * ``heads_loss``: ``functional.deconf_heads_loss`` against slices, ``F.linear``,
    ``F.cross_entropy`` and ``F.mse_loss``.
  * ``split_columns``: against two slice copies and autograd's slice backward.
  * ``training_step``: ``DeconfoundedNetPL`` on the fused route against the same module with the three
    functions replaced by the torch expressions (the extractor and the classification head are the
    same HIP kernels on both sides). The torch side skips no constant feature column: its gradient
    is NaN there when one occurs; the inputs here have none.
Device-event times of ``inner`` back-to-back calls, divided by ``inner``, over ``iters`` alternating
rounds (median, min, max, in microseconds): end-to-end times of the whole call, launch, autograd and
allocation included. One JSON line per case."""
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

SIZES = [(4, 64, 8), (32, 2048, 64)]
CLASSES, N_CONT = (3, 2), 2


def timed(fn, inner):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(inner):
        out = fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) * 1e3 / inner, out


def compare(name, fns, args, extra, inner=None):
    """``fns``: {label: callable}; the first is what the others are compared with. Alternating
    rounds: the machine is shared."""
    inner = inner or args.inner
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    times, outs = {k: [] for k in fns}, {}
    for _ in range(args.iters):
        for k, fn in fns.items():
            us, outs[k] = timed(fn, inner)
            times[k].append(us)
    first = next(iter(fns))
    line = {"case": name, **extra}
    for k, t in times.items():
        line[k + "_us"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2),
                           "max": round(max(t), 2)}
        if k != first:
            line[f"{k}_over_{first}"] = round(statistics.median(t) / statistics.median(times[first]), 2)
            line[f"{first}_max_below_{k}_min"] = bool(max(times[first]) < min(t))
            line[f"{k}_max_below_{first}_min"] = bool(max(t) < min(times[first]))
            line[f"max_abs_difference_{k}"] = float(
                (outs[k].double() - outs[first].double()).abs().max())
    print(json.dumps(line), flush=True)


def torch_correlation_loss(features, n):
    conf_f = features[:, :n, None]
    deconf_f = features[:, None, n:]
    conf_f_norm = conf_f - conf_f.mean(0, keepdim=True)
    deconf_f_norm = deconf_f - deconf_f.mean(0, keepdim=True)
    num = (conf_f_norm * deconf_f_norm).sum(0)
    d = torch.multiply(conf_f_norm.square().sum(0).sqrt(),
                       deconf_f_norm.square().sum(0).sqrt()).clamp(min=1e-8)
    return torch.clamp(num / d, -1.0, 1.0).square().mean()


def torch_heads_loss(features, n, cat_heads, table, cont_head, cont_target, conf_mult=1.0):
    conf = features[:, :n]
    cat = cont = None
    if cat_heads:
        cat = sum(F.cross_entropy(F.linear(conf, W, b), table[h]) / len(cat_heads)
                  for h, (W, b) in enumerate(cat_heads)) * conf_mult
    if cont_head is not None:
        cont = F.mse_loss(F.linear(conf, *cont_head), cont_target) * conf_mult
    return cat, cont


def torch_split_columns(features, n):
    return features[:, :n].contiguous(), features[:, n:].contiguous()


def bench_kernels(args, dev):
    g = torch.Generator().manual_seed(0)
    for B, Fe, n in SIZES:
        x = (torch.rand((B, Fe), generator=g) * 2 - 1).to(dev)
        heads = [((torch.rand((K, n), generator=g) - 0.5).to(dev), torch.zeros(K, device=dev))
                 for K in CLASSES]
        chead = ((torch.rand((N_CONT, n), generator=g) - 0.5).to(dev), torch.zeros(N_CONT, device=dev))
        table = torch.stack([torch.randint(0, K, (B,), generator=g) for K in CLASSES]).to(dev)
        target = torch.rand((B, N_CONT), generator=g).to(dev)
        da, db = torch.rand((B, n), generator=g).to(dev), torch.rand((B, Fe - n), generator=g).to(dev)
        extra = {"B": B, "F": Fe, "n_conf": n}

        def corr(fn):
            def run():
                t = x.detach().requires_grad_(True)
                fn(t, n).backward()
                return t.grad
            return run

        def head(fn):
            def run():
                t = x.detach().requires_grad_(True)
                hs = [(W.detach().requires_grad_(True), b.detach().requires_grad_(True))
                      for W, b in heads]
                ch = tuple(v.detach().requires_grad_(True) for v in chead)
                cat, cont = fn(t, n, hs, table, ch, target)
                (cat + cont).backward()
                return torch.cat([t.grad.flatten(), hs[0][0].grad.flatten(), ch[0].grad.flatten()])
            return run

        def split(fn):
            def run():
                t = x.detach().requires_grad_(True)
                a, b = fn(t, n)
                torch.autograd.backward([a, b], [da, db])
                return t.grad
            return run

        compare("correlation_loss", {"hip": corr(HF.deconf_correlation_loss),
                                     "torch": corr(torch_correlation_loss)}, args, extra)
        compare("heads_loss", {"hip": head(HF.deconf_heads_loss), "torch": head(torch_heads_loss)},
                args, dict(extra, classes=list(CLASSES), n_cont=N_CONT))
        compare("split_columns", {"hip": split(HF.split_columns), "torch": split(torch_split_columns)},
                args, extra)


def bench_step(args, dev):
    import deconfounded_cases as C
    from adell_mri_amd.modules.classification import deconfounded_classification as D
    from adell_mri_amd.modules.classification.pl import DeconfoundedNetPL
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn

    torch.manual_seed(0)
    kw = C.net_kwargs("a")
    net = DeconfoundedNetPL(embedder=D.CategoricalConversion(C.CAT_VARS["a"]), cat_confounder_key="cat",
                            cont_confounder_key="cont", adn_fn=get_adn_fn(3, "batch", "swish", 0.0),
                            **kw).to(dev).train()
    batch = {"image": torch.from_numpy(C.step_input("a", 7)).to(dev),
             "label": torch.tensor(C.NETS["a"][2]).to(dev),
             "cat": torch.from_numpy(C.cat_table("a")).to(dev),
             "cont": torch.tensor(C.NETS["a"][4]).to(dev)}
    built = (HF.deconf_correlation_loss, HF.deconf_heads_loss, HF.split_columns)

    def step(fused):
        def run():
            (HF.deconf_correlation_loss, HF.deconf_heads_loss, HF.split_columns) = built if fused else (
                torch_correlation_loss, torch_heads_loss, torch_split_columns)
            try:
                net.zero_grad()
                loss = net.training_step(batch, 0)
                loss.backward()
            finally:
                HF.deconf_correlation_loss, HF.deconf_heads_loss, HF.split_columns = built
            return loss.detach()
        return run

    compare("training_step", {"hip": step(True), "torch": step(False)}, args,
            {"input": list(C.NETS["a"][1]), "network": "a"}, inner=max(1, args.inner // 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_deconfounded.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    bench_kernels(args, dev)
    bench_step(args, dev)


if __name__ == "__main__":
    main()
