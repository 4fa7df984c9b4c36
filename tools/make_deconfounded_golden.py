#!/usr/bin/env python3
"""Fixtures of the deconfounded classifier from the REAL reference (needs a checkout of the
reference, ADELL_REFERENCE; no test reads it, the tests read the fixtures):

    python tools/make_deconfounded_golden.py -> tests/golden/deconfounded_surface.json,
                                                tests/golden/deconfounded_kernels.npz,
                                                tests/golden/deconfounded_step_<net>.npz,
                                                tests/golden/deconfounded_bounds.json

The reference is imported through the stub recipe of tools/make_batch_ensemble_golden.py:
``DeconfoundedNetGeneric``, ``CategoricalConversion`` and ``CatNet`` are the real ones. Lightning is
not installed, so the arithmetic of ``DeconfoundedNetPL`` (classification/pl.py:2376-2564) is
restated here, and the signatures of the wrapper and of the factory are read from their source text.

* surface: signatures, ``state_dict`` keys and shapes of the two fixture networks.
* kernels, in fp64: the reference's ``correlation_loss`` expression (loss for every case; gradient
  where it is finite, that is without a constant column) and the heads' losses by
  ``F.cross_entropy`` / ``F.mse_loss`` with their gradients.
* steps (tests/deconfounded_cases.py NETS): one training step -- the four loss terms, the logits,
  every gradient, ``torch.optim.Adam`` over the confounder / classifier groups with a NON-ZERO weight
  decay -- and one validation step in ``eval()`` mode. The reference probes the feature width with a
  forward in ``train()`` mode, which moves the batch-norm running statistics; they are put back to
  their initial values before the weights are filled (this package reads ``output_features``).

Bounds: the reference's own fp32 run against its fp64 run, ASSERTED to stay within a quarter of the
step tolerances (the fill gain and the input seed are walked until that holds); the kernel
quantities are measured against ``SUM_BOUND`` and four times the error is recorded where one uses
more than a quarter of it (deconfounded_bounds.json).
"""
import ast
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
    ("adell_mri.modules.layers", "adell_mri/modules/layers"),
    ("adell_mri.utils", "adell_mri/utils"),
    ("adell_mri.modules.segmentation", "adell_mri/modules/segmentation"),
    ("adell_mri.modules.classification", "adell_mri/modules/classification"),
    ("adell_mri.modules.classification.classification",
     "adell_mri/modules/classification/classification"),
]:
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(REF, path)]
    sys.modules[name] = m
import einops.layers.torch  # noqa: E402,F401  (the reference uses it via bare `import einops`)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adell_mri.modules.classification.classification import classification as RC  # noqa: E402

# (the package's __init__, stubbed out above, is where the reference's module finds these two)
sys.modules["adell_mri.modules.classification.classification"].VGG = RC.VGG
sys.modules["adell_mri.modules.classification.classification"].CatNet = RC.CatNet
from adell_mri.modules.classification.classification.deconfounded_classification import (  # noqa: E402
    CategoricalConversion, DeconfoundedNetGeneric)
from adell_mri.modules.layers.adn_fn import get_adn_fn  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import deconfounded_cases as C  # noqa: E402
import deconfounded_ref as R  # noqa: E402
from cases import grad_rel_err  # noqa: E402
from classification_cases import zero_dropout  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def rel(a, r):
    return R.rel(a, r)


def bound_entry(err):
    return {"fp32_vs_fp64": err, "ratio_to_SUM_BOUND": err / C.SUM_BOUND,
            "bound": C.SUM_BOUND if err <= 0.25 * C.SUM_BOUND else 4.0 * err}


# ---- the wrapper's arithmetic (pl.py:2376-2454), restated ----------------------------------------------
def correlation_loss(features, n):
    conf_f = features[:, :n, None]
    deconf_f = features[:, None, n:]
    conf_f_norm = conf_f - conf_f.mean(0, keepdim=True)
    deconf_f_norm = deconf_f - deconf_f.mean(0, keepdim=True)
    num = (conf_f_norm * deconf_f_norm).sum(0)
    d = torch.multiply(conf_f_norm.square().sum(0).sqrt(),
                       deconf_f_norm.square().sum(0).sqrt()).clamp(min=1e-8)
    return torch.clamp(num / d, -1.0, 1.0).square().mean()


def step_losses(name, net, x, y, cat, cont, conf_mult=1.0):
    """(classification loss, cat loss | None, cont loss | None, feature loss, logits)."""
    classification, cat_pred, cont_pred, features = net(x)
    cat_loss = cont_loss = None
    if cat is not None:
        cat_loss = sum(F.cross_entropy(p, y_) / len(cat_pred) for p, y_ in zip(cat_pred, cat)) \
            * conf_mult
    if cont is not None:
        cont_loss = F.mse_loss(cont_pred, cont.to(cont_pred)) * conf_mult
    feat = correlation_loss(features, net.n_features_deconfounder)
    logits = classification.squeeze(1)
    if net.n_classes > 2:
        cls = F.cross_entropy(logits, y.to(torch.int64)).mean()
    else:
        cls = F.binary_cross_entropy_with_logits(logits, y.to(logits.dtype)).mean()
    return cls, cat_loss, cont_loss, feat, logits


def build(name):
    kw = C.net_kwargs(name)
    net = DeconfoundedNetGeneric(adn_fn=get_adn_fn(kw["n_dim"], "batch", "swish", 0.0), **kw)
    for m in net.modules():                 # the constructor's probe ran in train() mode
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.reset_running_stats()
    return net


def groups_of(net):
    conf = [n for n, _ in net.named_parameters() if "confound" in n]
    rest = [n for n, _ in net.named_parameters() if "confound" not in n]
    return [(conf, 0.0), (rest, C.STEP_WD)]


def run_step(name, gain, x, dt):
    net = build(name)
    rates = zero_dropout(net)
    keys = list(net.state_dict().keys())
    names = [k for k, _ in net.named_parameters()]
    net.load_state_dict(C.fill(net.state_dict(), gain))
    net = net.to(dt).train()
    x = torch.from_numpy(x).to(dt)
    y = torch.tensor(C.NETS[name][2])
    embedder = CategoricalConversion(C.CAT_VARS[name])
    cat = embedder([list(item) for item in C.NETS[name][3]])
    assert np.array_equal(torch.stack(cat).numpy(), C.cat_table(name))
    cont = None if C.NETS[name][4] is None else torch.tensor(C.NETS[name][4], dtype=dt)
    parts = step_losses(name, net, x, y, cat, cont)
    total = sum(v for v in parts[:4] if v is not None)
    total.backward()
    out = {"total": total.detach(), "logits": parts[4].detach()}
    for k, v in zip(("loss", "cat_loss", "cont_loss", "feat_loss"), parts[:4]):
        if v is not None:
            out[k] = v.detach()
    for k, p in net.named_parameters():
        if p.grad is not None:              # the extractor's own head takes no part
            out["grad:" + k] = p.grad.clone()
    groups = groups_of(net)
    by_name = dict(net.named_parameters())
    torch.optim.Adam([{"params": [by_name[n] for n in members], "weight_decay": wd}
                      for members, wd in groups], lr=C.STEP_LR, eps=C.STEP_EPS).step()
    net.eval()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if ".feature_extraction." not in k:     # CatNet: the same tensors as ``res_net.*``
                out["step1:" + k] = v.detach().clone()
        vparts = step_losses(name, net, x, y, cat, cont)
        out["val_total"] = sum(v for v in vparts[:4] if v is not None).detach()
        out["val_logits"] = vparts[4].detach()
        for k, v in zip(("loss", "cat_loss", "cont_loss", "feat_loss"), vparts[:4]):
            if v is not None:
                out["val_" + k] = v.detach()
        out["features"] = net(x, return_features=True).detach()
    return out, names, keys, rates, groups


class _Grads(dict):
    @property
    def files(self):
        return list(self)


def within_quarter(o32, o64):
    q, worst, ok = 0.25, {}, True
    for k in o64:
        if k.endswith("total") or k.endswith("loss"):
            worst[k] = abs(float(o32[k]) - float(o64[k])) / abs(float(o64[k]))
            ok &= worst[k] <= q * C.TOL["loss"]
    for k in ("logits", "val_logits", "features"):
        worst[k] = rel(o32[k].numpy(), o64[k].numpy())
        ok &= worst[k] <= q * C.TOL["loss"]
    worst["grad"] = worst["param"] = 0.0
    grads = _Grads({k: v.numpy() for k, v in o64.items() if k.startswith("grad:")})
    for k in o64:
        a, r = o32[k].double(), o64[k].double()
        if k.startswith("grad:"):
            e = grad_rel_err(grads, k[5:], a.numpy())
            worst["grad"] = max(worst["grad"], e)
            ok &= e <= q * C.TOL["grad"]
        elif k.startswith("step1:") and o64[k].is_floating_point():
            rt, at = C.TOL["param"]
            e = float(((a - r).abs() / (at + rt * r.abs())).max())
            worst["param"] = max(worst["param"], e)
            ok &= e <= q
    return bool(ok), worst


def gen_steps(bounds):
    for name in C.NETS:
        found = None
        for gain in (2.0, 1.5, 1.0, 3.0):
            for seed in range(7, 7 + 6):
                x = C.step_input(name, seed)
                o64, names, keys, rates, groups = run_step(name, gain, x, torch.float64)
                o32 = run_step(name, gain, x, torch.float32)[0]
                ok, worst = within_quarter(o32, o64)
                spread = float(o64["logits"].std(0).mean())
                # no constant feature column: the reference's gradient must be finite
                live = bool((o64["features"].std(0) > 0).all())
                finite = all(bool(torch.isfinite(v).all()) for v in o64.values()
                             if v.is_floating_point())
                if ok and spread > 1e-3 and live and finite:
                    found = (gain, seed)
                    break
            if found:
                break
        if not found:
            raise SystemExit(f"{name}: no (gain, seed) keeps the reference's fp32 step within a "
                             f"quarter of the tolerances; last worst {worst}")
        bounds[name] = worst
        out = {"x": x, "y": np.array(C.NETS[name][2]), "gain": np.float64(found[0]),
               "seed": np.int32(found[1]), "dropout_rates": np.array(rates, dtype=np.float64),
               "param_keys": np.array(names), "state_keys": np.array(keys),
               "groups:n": np.int32(len(groups))}
        for i, (members, wd) in enumerate(groups):
            out[f"groups:{i}:names"] = np.array(members, dtype=str)
            out[f"groups:{i}:wd"] = np.float64(wd)
        for k, v in o64.items():
            if k.endswith("total") or k.endswith("loss"):
                out[k] = v.numpy()                      # fp64
            elif v.is_floating_point():
                out[k] = v.float().numpy()
            else:
                out[k] = v.numpy()
        print(f"{name}: gain {found[0]}, seed {found[1]}, terms "
              f"{[round(float(o64[k]), 6) for k in ('loss', 'cat_loss', 'cont_loss', 'feat_loss') if k in o64]}"
              f", logit spread {spread:.3e}, fp32 vs fp64 (param: 1 = the tolerance): {worst}")
        path = os.path.join(OUT, f"deconfounded_step_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1 << 20


# ---- surface -------------------------------------------------------------------------------------------
def source_signature(path, cls, fn):
    """[name, default source text | None] per parameter of a function read from source text."""
    with open(os.path.join(REF, path)) as fh:
        tree = ast.parse(fh.read())
    body = tree.body
    if cls is not None:
        body = next(n for n in body if isinstance(n, ast.ClassDef) and n.name == cls).body
    node = next(n for n in body if isinstance(n, ast.FunctionDef) and n.name == fn)
    a = node.args
    pos = a.posonlyargs + a.args
    defaults = [None] * (len(pos) - len(a.defaults)) + [ast.unparse(d) for d in a.defaults]
    out = [[p.arg, d] for p, d in zip(pos, defaults)]
    if a.vararg:
        out.append(["*" + a.vararg.arg, None])
    out += [[p.arg, None if d is None else ast.unparse(d)] for p, d in zip(a.kwonlyargs, a.kw_defaults)]
    if a.kwarg:
        out.append(["**" + a.kwarg.arg, None])
    return out


def gen_surface():
    surface = {
        "signatures": {f"{cls.__name__}.{fn}": C.signature_of(getattr(cls, fn))
                       for cls in (DeconfoundedNetGeneric, CategoricalConversion)
                       for fn in ("__init__", "forward")},
        "source_signatures": {
            "DeconfoundedNetPL.__init__": source_signature(
                "adell_mri/modules/classification/pl.py", "DeconfoundedNetPL", "__init__"),
            "get_deconfounded_classification_network": source_signature(
                "adell_mri/utils/network_factories.py", None,
                "get_deconfounded_classification_network"),
        },
        "methods": {"DeconfoundedNetPL": sorted(
            n.name for n in next(
                c for c in ast.parse(open(os.path.join(
                    REF, "adell_mri/modules/classification/pl.py")).read()).body
                if isinstance(c, ast.ClassDef) and c.name == "DeconfoundedNetPL").body
            if isinstance(n, ast.FunctionDef))},
        "state": {name: {k: list(v.shape) for k, v in build(name).state_dict().items()}
                  for name in C.NETS},
    }
    path = os.path.join(OUT, "deconfounded_surface.json")
    with open(path, "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes")


# ---- kernel cases --------------------------------------------------------------------------------------
def corr_record(x, n, dt, grad):
    t = torch.from_numpy(x).to(dt).requires_grad_(grad)
    loss = correlation_loss(t, n)
    if grad:
        loss.backward()
    return loss.detach(), (t.grad if grad else None)


def gen_kernels(bounds):
    gold, worst = {}, {"corr_loss": 0.0, "corr_grad": 0.0, "heads_loss": 0.0, "heads_grad": 0.0}
    for B, Fe, n in C.CORR_CASES + [C.CORR_DUP]:
        tag = f"corr:{B}:{Fe}:{n}"
        x = C.dup_input() if (B, Fe, n) == C.CORR_DUP else C.corr_input(B, Fe, n)
        l64, _ = corr_record(x, n, torch.float64, False)
        l32, _ = corr_record(x, n, torch.float32, False)
        gold[tag + ":loss"] = l64.numpy()
        worst["corr_loss"] = max(worst["corr_loss"], abs(float(l32) - float(l64)) / float(l64))
        if (B, Fe, n) == C.CORR_DUP or B * Fe > 1000:
            continue
        # the gradient where the reference has one: the same input without constant columns
        x = C.corr_input(B, Fe, n, zero_columns=False)
        l64, g64 = corr_record(x, n, torch.float64, True)
        _, g32 = corr_record(x, n, torch.float32, True)
        assert bool(torch.isfinite(g64).all())
        gold[tag + ":live:loss"], gold[tag + ":live:grad"] = l64.numpy(), g64.numpy()
        worst["corr_grad"] = max(worst["corr_grad"], rel(g32.numpy(), g64.numpy()))
        # the rule of tests/deconfounded_ref.py changes nothing where the reference is finite
        lr, gr = R.correlation_loss_and_grad(x, n)
        assert abs(lr - float(l64)) <= 1e-14 and rel(gr, g64.numpy()) <= 1e-12
    # with a constant column the reference's gradient is NaN there, in fp32 and in fp64 (in a
    # training step the NaN then reaches every parameter of the extractor)
    x = C.corr_input(5, 24, 8)
    for dt in (torch.float32, torch.float64):
        g = corr_record(x, 8, dt, True)[1]
        assert bool(torch.isnan(g[:, [1, 9]]).all())
        print(f"reference gradient with constant columns 1 and 9, {dt}: NaN in columns "
              f"{sorted(set(torch.isnan(g).nonzero()[:, 1].tolist()))}")
    for (B, n, heads, mult) in [(5, 8, "both", 0.5), (3, 1, "two", 1.0), (70, 65, "cont", 1.0)]:
        classes, n_cont = C.HEADS[heads]
        tag = f"heads:{B}:{n}:{heads}"
        x, cat, labels, cont, target = C.heads_case(B, n + 3, n, classes, n_cont)
        rec = {}
        for dt in (torch.float64, torch.float32):
            leaf = lambda a: torch.from_numpy(a).to(dt).requires_grad_(True)  # noqa: E731
            xt = leaf(x)
            conf = xt[:, :n]
            leaves, terms = {"x": xt}, {}
            if cat:
                ws = [(leaf(W), leaf(b)) for W, b in cat]
                for h, (W, b) in enumerate(ws):
                    leaves[f"W{h}"], leaves[f"b{h}"] = W, b
                terms["cat"] = sum(F.cross_entropy(F.linear(conf, W, b), torch.from_numpy(labels[h]))
                                   / len(ws) for h, (W, b) in enumerate(ws)) * mult
            if cont is not None:
                Wc, bc = leaf(cont[0]), leaf(cont[1])
                leaves["Wc"], leaves["bc"] = Wc, bc
                terms["cont"] = F.mse_loss(F.linear(conf, Wc, bc), torch.from_numpy(target).to(dt)) * mult
            sum(terms.values()).backward()
            rec[dt] = ({k: v.detach() for k, v in terms.items()},
                       {k: v.grad for k, v in leaves.items()})
        for k, v in rec[torch.float64][0].items():
            gold[f"{tag}:{k}"] = v.numpy()
            worst["heads_loss"] = max(worst["heads_loss"],
                                      abs(float(rec[torch.float32][0][k]) - float(v)) / abs(float(v)))
        for k, v in rec[torch.float64][1].items():
            gold[f"{tag}:grad:{k}"] = v.numpy()
            worst["heads_grad"] = max(worst["heads_grad"], rel(rec[torch.float32][1][k].numpy(), v.numpy()))
        gold[f"{tag}:conf_mult"] = np.float64(mult)
    bounds["kernels"] = {k: bound_entry(e) for k, e in sorted(worst.items())}
    print("kernel quantities, the reference's fp32 against fp64:", worst)
    path = os.path.join(OUT, "deconfounded_kernels.npz")
    np.savez_compressed(path, **gold)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 19


if __name__ == "__main__":
    bounds = {"SUM_BOUND": C.SUM_BOUND, "TOL": C.TOL}
    gen_surface()
    gen_kernels(bounds)
    gen_steps(bounds)
    with open(os.path.join(OUT, "deconfounded_bounds.json"), "w") as fh:
        json.dump(bounds, fh, indent=1, sort_keys=True)
        fh.write("\n")
