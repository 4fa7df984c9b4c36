#!/usr/bin/env python3
"""Fixtures of the semi-supervised losses from the REAL reference (needs a checkout of the reference,
ADELL_REFERENCE; no test reads it, the tests read the fixtures):

    python tools/make_semisl_losses_golden.py -> tests/golden/semisl_losses_surface.json,
                                                 tests/golden/semisl_losses_anchor.npz,
                                                 tests/golden/semisl_losses_nn.npz,
                                                 tests/golden/semisl_losses_pl.npz,
                                                 tests/golden/semisl_losses_bounds.json

The reference's ``modules/__init__`` imports MONAI, which is not installed; the packages ``adell_mri``,
``adell_mri.modules`` and ``adell_mri.modules.semi_supervised_segmentation`` are stubbed with their
``__path__`` set (the recipe of tools/make_deconfounded_golden.py), after which
``...semi_supervised_segmentation.losses`` is the real module.

* surface: names, kinds and defaults of the constructors' and methods' parameters, and
  ``derangement(n, seed=0)`` for n = 2 .. 9.
* anchor (tests/semisl_losses_cases.py ANCHOR_CASES): value and gradients in fp64 of the fp32 inputs,
  which are a function of the case's name and are not stored; the gradients of the two large shapes
  are stored as every 13th element (the tests compare the whole tensors against
  tests/semisl_losses_ref.py, which tests/test_semisl_losses.py holds against these fixtures). The two
  derangement cases record the permutations drawn.
* nn: NN_PUTS ``put`` calls and one ``forward`` with its gradient; after every call the queue row for
  row (fp32, to be reproduced bit for bit) and ``len()``; a ``forward`` on an empty queue.
* pl (PL_CASES): values and gradients in fp64.
* bounds: the reference's own fp32 run against its fp64 run for every quantity; where that error uses
  more than a quarter of the project's tolerance, four times the error is recorded as "tol".
"""
import inspect
import json
import os
import sys
import types

import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADELL_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)
for name, path in [
    ("adell_mri", "adell_mri"), ("adell_mri.modules", "adell_mri/modules"),
    ("adell_mri.modules.semi_supervised_segmentation",
     "adell_mri/modules/semi_supervised_segmentation"),
]:
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(REF, path)]
    sys.modules[name] = m
import torch  # noqa: E402

from adell_mri.modules.semi_supervised_segmentation import losses as RL  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import semisl_losses_cases as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
BOUNDS = {}


def bound_value(key, v32, v64):
    v32, v64 = np.asarray(v32, dtype=np.float64), np.asarray(v64, dtype=np.float64)
    err = float(np.abs(v32 - v64).max())
    tol = float((C.VALUE_ATOL + C.VALUE_RTOL * np.abs(v64)).min())
    BOUNDS[key] = {"err": err, "share": err / tol}
    if err > tol / 4:
        BOUNDS[key]["tol"] = 4 * err


def bound_grad(key, g32, g64):
    g32, g64 = np.asarray(g32, dtype=np.float64), np.asarray(g64, dtype=np.float64)
    err = float(np.abs(g32 - g64).max())
    tol = C.GRAD_REL * float(np.abs(g64).max())
    BOUNDS[key] = {"err": err, "share": err / tol}
    if err > tol / 4:
        BOUNDS[key]["tol"] = 4 * err


def params(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


def surface():
    out = {"functions": {n: params(getattr(RL, n))
                         for n in ("swap", "derangement", "anchors_from_derangement")},
           "classes": {}}
    for cls in ("LocalContrastiveLoss", "LocalContrastiveLossWithAnchors", "AnatomicalContrastiveLoss",
                "NearestNeighbourLoss", "PseudoLabelCrossEntropy"):
        k = getattr(RL, cls)
        out["classes"][cls] = {n: params(f) for n, f in vars(k).items()
                               if inspect.isfunction(f) and (n == "__init__" or n == "__len__"
                                                             or not n.startswith("_"))}
    out["derangement_seed0"] = {str(n): [int(v) for v in RL.derangement(n, seed=0)] for n in range(2, 10)}
    with open(os.path.join(OUT, "semisl_losses_surface.json"), "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


def anchor_run(tag, dtype, out=None):
    case = C.ANCHOR_CASES[tag]
    x, a1, a2, r = (torch.from_numpy(v).to(dtype) for v in C.anchor_inputs(tag))
    x.requires_grad_(True)
    mod = RL.LocalContrastiveLossWithAnchors(case["temperature"], seed=case.get("seed", 42))
    perms = []
    if case["anchors"] == "given":
        a1.requires_grad_(True)
        a2.requires_grad_(True)
        loss = mod(x, a1, a2)
    else:
        # the permutations the module is about to draw, from a generator in the same state
        probe = np.random.default_rng(case["seed"])
        n_draws = 2 if case["anchors"] == "drawn" else 1
        perms = [RL.derangement(x.shape[0], rng=probe) for _ in range(n_draws)]
        if case["anchors"] == "drawn":
            loss = mod(x)
        else:
            a1.requires_grad_(True)
            loss = mod(x, a1)
    (loss * r).sum().backward()
    grads = {"x": x.grad}
    if a1.grad is not None:
        grads["a1"] = a1.grad
    if a2.grad is not None:
        grads["a2"] = a2.grad
    if out is not None:
        out[f"{tag}:value"] = loss.detach().numpy()
        for k, g in grads.items():
            out[f"{tag}:grad_{k}"] = C.grad_sample(g.numpy())
        if perms:
            out[f"{tag}:perms"] = np.asarray(perms, dtype=np.int64)
    return loss.detach().numpy(), {k: g.numpy() for k, g in grads.items()}


def anchor():
    out = {}
    for tag in C.ANCHOR_CASES:
        v64, g64 = anchor_run(tag, torch.float64, out)
        v32, g32 = anchor_run(tag, torch.float32)
        bound_value(f"anchor:{tag}:value", v32, v64)
        for k in g64:
            bound_grad(f"anchor:{tag}:grad_{k}", g32[k], g64[k])
        print("anchor", tag, v64, {k: float(np.abs(g).max()) for k, g in g64.items()})
    np.savez_compressed(os.path.join(OUT, "semisl_losses_anchor.npz"), **out)


def queue_state(mod, out, key):
    out[f"{key}:len"] = np.asarray(len(mod), dtype=np.int64)
    for cl, q in enumerate(mod.q):
        entries = list(q.queue)
        out[f"{key}:q{cl}:n"] = np.asarray(len(entries), dtype=np.int64)
        for k, e in enumerate(entries):
            out[f"{key}:q{cl}:{k}"] = e.numpy()


def nn_run(dtype, out=None):
    mod = RL.NearestNeighbourLoss(**C.NN_ARGS)
    for i in range(C.NN_PUTS):
        X, y = (torch.from_numpy(v) for v in C.nn_put_inputs(i))
        mod.put(X.to(dtype), y)
        if out is not None:
            queue_state(mod, out, f"put{i}")
    X, y = (torch.from_numpy(v) for v in C.nn_forward_inputs())
    X = X.to(dtype).requires_grad_(True)
    loss = mod(X, y.to(dtype))
    loss.backward()
    if out is not None:
        queue_state(mod, out, "fwd")
    return loss.detach().numpy(), X.grad.numpy()


def nn():
    out = {}
    v32, g32 = nn_run(torch.float32, out)
    v64, g64 = nn_run(torch.float64)
    out["fwd:value"], out["fwd:grad"] = v64, g64
    bound_value("nn:value", v32, v64)
    bound_grad("nn:grad", g32, g64)
    empty = RL.NearestNeighbourLoss(**C.NN_ARGS)
    X, y = (torch.from_numpy(v) for v in C.nn_forward_inputs())
    out["empty:value"] = empty(X, y).numpy()
    print("nn", v64, float(np.abs(g64).max()), "empty", out["empty:value"], "len", int(out["fwd:len"]))
    np.savez_compressed(os.path.join(OUT, "semisl_losses_nn.npz"), **out)


def pl_run(name, dtype):
    kw = dict(C.PL_CASES[name])
    if "weight" in kw:
        kw["weight"] = torch.tensor(kw["weight"], dtype=dtype)
    pred, proba = (torch.from_numpy(v) for v in C.pl_inputs())
    pred = pred.to(dtype).requires_grad_(True)
    mod = RL.PseudoLabelCrossEntropy(C.PL_THRESHOLD, **kw)
    if dtype == torch.float64:
        # the module casts the pseudo-labels to fp32; the fp64 run takes its expression with fp64 targets
        loss = mod.ce(pred, (proba > mod.threshold).to(dtype))
    else:
        loss = mod(pred, proba)
    loss.backward()
    return loss.detach().numpy(), pred.grad.numpy()


def pl():
    pred, proba = C.pl_inputs()
    out = {"pred": pred, "proba": proba}
    assert int((proba == np.float32(C.PL_THRESHOLD)).sum()) > 10
    for name in C.PL_CASES:
        v64, g64 = pl_run(name, torch.float64)
        v32, g32 = pl_run(name, torch.float32)
        out[f"{name}:value"], out[f"{name}:grad"] = v64, g64
        bound_value(f"pl:{name}:value", v32, v64)
        bound_grad(f"pl:{name}:grad", g32, g64)
        print("pl", name, v64, float(np.abs(g64).max()))
    np.savez_compressed(os.path.join(OUT, "semisl_losses_pl.npz"), **out)


if __name__ == "__main__":
    torch.manual_seed(0)
    surface()
    anchor()
    nn()
    pl()
    with open(os.path.join(OUT, "semisl_losses_bounds.json"), "w") as fh:
        json.dump(BOUNDS, fh, indent=1, sort_keys=True)
        fh.write("\n")
    worst = max(BOUNDS.items(), key=lambda kv: kv[1]["share"])
    print("largest share of a tolerance used by the reference's own fp32 error:", worst)
