#!/usr/bin/env python3
"""Fixtures of the batch-ensemble layers and networks from the REAL reference (needs a checkout of the
reference, ADELL_REFERENCE; no test reads it, the tests read the fixtures):

    python tools/make_batch_ensemble_golden.py -> tests/golden/batch_ensemble_surface.json,
                                                  tests/golden/batch_ensemble_layers.npz,
                                                  tests/golden/batch_ensemble_step_<net>.npz,
                                                  tests/golden/batch_ensemble_bounds.json

The reference is imported through the stub recipe of tools/make_ensemble_golden.py (empty package
stubs with the right __path__, then the leaf modules): ``BatchEnsemble``, ``BatchEnsembleWrapper``,
``ResNetBackbone``, ``CatNet`` and ``OrdNet`` are the real ones. Lightning is not installed, so the
arithmetic of the wrappers (classification/pl.py) is restated as in tools/make_classification_golden.py.

* surface: constructor and forward signatures, ``state_dict`` keys and shapes.
* layers (tests/batch_ensemble_cases.py LAYERS x MODES), in fp64: input, tables, the members drawn
  (``np.random.randint`` is recorded while the reference runs), output and every gradient.
* steps: ``np.random.seed(STEP_SEED)``, one training step (AdamW over the groups of
  ``configure_optimizers``; the member tables are in the ordinary group), a validation step in
  ``eval()`` mode (the mean over the members) and, for ``CatNet``, a forward with ``batch_idx=1``. The
  members every stage drew are recorded in call order.

Bounds: the reference's own fp32 run against its fp64 run. Every step is ASSERTED to stay within a
quarter of the step tolerances (the fill gain and the input seed are walked until that holds). The
layer quantities are measured against ``SUM_BOUND``; where one uses more than a quarter of it, four
times the reference's error is recorded as the bound the tests use (batch_ensemble_bounds.json).
"""
import json
import os
import sys
import types

import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference checkout: ADELL_REFERENCE, else a `reference` directory beside this repository
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

from adell_mri.modules.classification.classification import classification as RC  # noqa: E402
from adell_mri.modules.classification.losses import OrdinalSigmoidalLoss  # noqa: E402
from adell_mri.modules.layers.adn_fn import get_adn_fn  # noqa: E402
from adell_mri.modules.layers.batch_ensemble import (BatchEnsemble,  # noqa: E402
                                                     BatchEnsembleWrapper)
from adell_mri.modules.layers.res_net import ResNetBackbone  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import batch_ensemble_cases as C  # noqa: E402
from cases import grad_rel_err  # noqa: E402  (the gradient metric of the step tests)
from classification_cases import step_groups, zero_dropout  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


class recorded_draws:
    """Every ``np.random.randint`` result while the block runs, in call order."""

    def __enter__(self):
        self.draws, self._orig = [], np.random.randint

        def randint(*args, **kwargs):
            out = self._orig(*args, **kwargs)
            self.draws.append(np.array(out))
            return out

        np.random.randint = randint
        return self.draws

    def __exit__(self, *exc):
        np.random.randint = self._orig


def rel(a, r):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-300))


def bound_entry(err):
    """The recorded error and the bound the tests use for the quantity."""
    return {"fp32_vs_fp64": err, "ratio_to_SUM_BOUND": err / C.SUM_BOUND,
            "bound": C.SUM_BOUND if err <= 0.25 * C.SUM_BOUND else 4.0 * err}


# ---- surface -------------------------------------------------------------------------------------------
def tree(net):
    return {k: list(v.shape) for k, v in net.state_dict().items()}


def gen_surface():
    adn = get_adn_fn(3, "batch", "swish", 0.0)
    structure = C.net_kwargs("cat")["resnet_structure"]
    surface = {
        "signatures": {f"{cls.__name__}.{fn}": C.signature_of(getattr(cls, fn))
                       for cls in (BatchEnsemble, BatchEnsembleWrapper)
                       for fn in ("__init__", "forward")},
        "state": {
            "BatchEnsemble": tree(BatchEnsemble(3, C.N, 4, 6, adn)),
            "BatchEnsemble.res_blocks": tree(BatchEnsemble(
                3, C.N, 4, 6, adn, {"kernel_size": 3, "adn_fn": adn}, res_blocks=True)),
            "BatchEnsembleWrapper": tree(BatchEnsembleWrapper(torch.nn.Linear(6, 5), C.N, 6, 5)),
            "ResNetBackbone": tree(ResNetBackbone(3, 1, structure, adn_fn=adn, batch_ensemble=C.N)),
            "ResNetBackbone2d": tree(ResNetBackbone(2, 1, structure,
                                                    adn_fn=get_adn_fn(2, "batch", "swish", 0.0),
                                                    batch_ensemble=C.N)),
            "ResNetBackbone.0": tree(ResNetBackbone(3, 1, structure, adn_fn=adn)),
        }}
    for name in C.NETS:
        surface["state"][name] = tree(getattr(RC, C.NETS[name][0])(adn_fn=adn, **C.net_kwargs(name)))
    path = os.path.join(OUT, "batch_ensemble_surface.json")
    with open(path, "w") as fh:
        json.dump(surface, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{path}: {os.path.getsize(path)} bytes")


# ---- layers --------------------------------------------------------------------------------------------
def reference_layer(layer, n):
    cls, dim, cin, cout, _ = C.LAYERS[layer]
    if cls == "BatchEnsemble":
        net = BatchEnsemble(dim, n, cin, cout)
    else:
        net = BatchEnsembleWrapper(torch.nn.Linear(cin, cout), n, cin, cout)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in C.layer_state(layer, n).items()})
    return net


def layer_records(layer, mode, dt):
    n, training, idx = C.MODES[mode]
    net = reference_layer(layer, n).to(dt).train(training)
    x = torch.from_numpy(C.layer_input(layer)).to(dt).requires_grad_(True)
    np.random.seed(C.DRAW_SEED)
    with recorded_draws() as draws:
        y = net(x) if idx is None else net(x, idx)
    out = {"y": y.detach()}
    if draws:
        assert len(draws) == 1
        out["idxs"] = torch.from_numpy(draws[0].astype(np.int64))
    if y.requires_grad:                     # the wrapper's eval mean runs under no_grad
        y.backward(torch.from_numpy(C.layer_dy(layer, y.shape)).to(dt))
        out["dx"] = x.grad
        for k, p in net.named_parameters():
            out["d" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
    return out


def gen_layers(bounds):
    gold, worst = {}, {}
    for layer, mode in C.layer_cases():
        o64, o32 = layer_records(layer, mode, torch.float64), layer_records(layer, mode, torch.float32)
        for k, v in o64.items():
            gold[f"{layer}:{mode}:{k}"] = v.numpy()
            if k == "idxs":
                assert np.array_equal(o32[k].numpy(), v.numpy())
                continue
            worst[k] = max(worst.get(k, 0.0), rel(o32[k].numpy(), v.numpy()))
        n = C.MODES[mode][0]
        if mode == "train":
            assert len(set(o64["idxs"].tolist())) > 1, "the draw picked one member only"
        if mode == "one" and C.LAYERS[layer][0] == "BatchEnsembleWrapper":
            assert "idxs" not in o64 and n == 1
    bounds["layers"] = {k: bound_entry(e) for k, e in sorted(worst.items())}
    print("layer quantities, the reference's fp32 against fp64:", worst)
    path = os.path.join(OUT, "batch_ensemble_layers.npz")
    np.savez_compressed(path, **gold)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 19


# ---- networks ------------------------------------------------------------------------------------------
def losses_of(name, net, x, y):
    """The wrapper's step arithmetic: (what is returned, the logits)."""
    n_classes = C.NETS[name][1]["n_classes"]
    if name == "ord":
        prediction, pre_bias = net(x, return_pre_bias=True)
        prediction = torch.squeeze(prediction, 1)
        loss, roc = OrdinalSigmoidalLoss(n_classes, None)(prediction, y.to(torch.int64),
                                                          pre_bias=pre_bias)
        return loss.mean() + roc.mean(), prediction
    prediction = torch.squeeze(net(x), 1)
    return torch.nn.BCEWithLogitsLoss()(prediction, y.to(x.dtype)).mean(), prediction


def run_step(name, gain, x, dt):
    np.random.seed(0)
    net = getattr(RC, C.NETS[name][0])(adn_fn=get_adn_fn(3, "batch", "swish", 0.0),
                                       **C.net_kwargs(name))
    rates = zero_dropout(net)
    keys = list(net.state_dict().keys())
    named = [(k, p) for k, p in net.named_parameters()]
    net.load_state_dict(C.fill(net.state_dict(), gain))
    if name == "ord":                   # OrdNet's constructor zeroes it; the fill must not undo that
        with torch.no_grad():
            net.classification_layer.op[-1].bias.zero_()
    net = net.to(dt).train()
    x = torch.from_numpy(x).to(dt)
    y = torch.tensor(C.NETS[name][3])
    np.random.seed(C.STEP_SEED)
    with recorded_draws() as draws:
        total, logits = losses_of(name, net, x, y)
    assert len(draws) == len(C.NETS[name][1]["resnet_structure"])
    total.backward()
    out = {"total": total.detach(), "logits": logits.detach(),
           "idxs": torch.from_numpy(np.stack(draws).astype(np.int64))}
    for k, p in net.named_parameters():
        if p.grad is None:              # the norm of a stage's last block, whose activation is skipped
            assert ".adn_op." in k and ".operations." in k, k
            continue
        out["grad:" + k] = p.grad.clone()
    groups, base_wd = step_groups(named, C.NETS[name][4])
    by_name = dict(net.named_parameters())
    torch.optim.AdamW([{"params": [by_name[n] for n in names], "weight_decay": wd}
                       for names, wd in groups], lr=C.STEP_LR, weight_decay=base_wd,
                      eps=C.STEP_EPS).step()
    net.eval()
    with torch.no_grad(), recorded_draws() as draws:
        for k, v in net.state_dict().items():
            if not k.startswith("feature_extraction."):      # the same tensors as ``res_net.*``
                out["step1:" + k] = v.detach().clone()
        vtotal, vlogits = losses_of(name, net, x, y)
        out["val_total"], out["val_logits"] = vtotal.detach(), vlogits.detach()
        if name == "cat":
            out["idx_logits"] = torch.squeeze(net(x, batch_idx=C.BATCH_IDX), 1).detach()
        assert not draws                                     # eval draws nothing
    return out, [k for k, _ in named], keys, rates, groups, base_wd


class _Grads(dict):
    """What tests/cases.py::grad_rel_err reads from a fixture: ``files`` and items."""

    @property
    def files(self):
        return list(self)


def within_quarter(o32, o64):
    """The reference's fp32 step against its fp64 step, at a quarter of every step tolerance."""
    q = 0.25
    worst, ok = {}, True
    for k in ("total", "val_total"):
        worst[k] = abs(float(o32[k]) - float(o64[k])) / abs(float(o64[k]))
        ok &= worst[k] <= q * C.TOL["loss"]
    for k in ("logits", "val_logits", "idx_logits"):
        if k in o64:
            worst[k] = rel(o32[k].numpy(), o64[k].numpy())
            ok &= worst[k] <= q * C.TOL["loss"]
    worst["grad"] = worst["param"] = 0.0
    grads = _Grads({k: v.numpy() for k, v in o64.items() if k.startswith("grad:")})
    for k in o64:
        a, r = o32[k].double(), o64[k].double()
        if k.startswith("grad:"):
            e = grad_rel_err(grads, k[5:], o32[k].double().numpy())
            worst["grad"] = max(worst["grad"], e)
            ok &= e <= q * C.TOL["grad"]
        elif k.startswith("step1:") and o64[k].is_floating_point():
            rt, at = C.TOL["param"]
            e = float(((a - r).abs() / (at + rt * r.abs())).max())     # <= 1 passes assert_allclose
            worst["param"] = max(worst["param"], e)
            ok &= e <= q
    return bool(ok), worst


def gen_steps(bounds):
    for name in C.NETS:
        found = None
        for gain in (2.0, 1.5, 1.0, 3.0):
            for seed in range(7, 7 + 6):
                x = C.step_input(name, seed)
                o64, names, keys, rates, groups, base_wd = run_step(name, gain, x, torch.float64)
                o32 = run_step(name, gain, x, torch.float32)[0]
                assert torch.equal(o32["idxs"], o64["idxs"])
                ok, worst = within_quarter(o32, o64)
                # the logits must differ between items and every stage must draw several members,
                # or the step pins nothing
                spread = float(o64["logits"].std(0).mean())
                mixed = all(len(set(row.tolist())) > 1 for row in o64["idxs"])
                if ok and spread > 1e-3 and mixed:
                    found = (gain, seed)
                    break
            if found:
                break
        if not found:
            raise SystemExit(f"{name}: no (gain, seed) keeps the reference's fp32 step within a "
                             f"quarter of the tolerances; last worst {worst}")
        bounds[name] = worst
        out = {"x": x, "y": np.array(C.NETS[name][3]), "gain": np.float64(found[0]),
               "seed": np.int32(found[1]), "dropout_rates": np.array(rates, dtype=np.float64),
               "param_keys": np.array(names), "state_keys": np.array(keys),
               "groups:n": np.int32(len(groups)), "groups:base_wd": np.float64(base_wd)}
        for i, (members, wd) in enumerate(groups):
            out[f"groups:{i}:names"] = np.array(members, dtype=str)
            out[f"groups:{i}:wd"] = np.float64(wd)
        for k, v in o64.items():
            if k.endswith("total"):
                out[k] = v.numpy()                      # fp64
            elif v.is_floating_point():
                out[k] = v.float().numpy()
            else:
                out[k] = v.numpy()
        print(f"{name}: gain {found[0]}, seed {found[1]}, total {float(o64['total']):.6f}, val "
              f"{float(o64['val_total']):.6f}, logit spread {spread:.3e}, drawn "
              f"{o64['idxs'].tolist()}, fp32 vs fp64 (param: 1 = the tolerance; others relative): "
              f"{worst}")
        path = os.path.join(OUT, f"batch_ensemble_step_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    bounds = {"SUM_BOUND": C.SUM_BOUND, "TOL": C.TOL}
    gen_surface()
    gen_layers(bounds)
    gen_steps(bounds)
    with open(os.path.join(OUT, "batch_ensemble_bounds.json"), "w") as fh:
        json.dump(bounds, fh, indent=1, sort_keys=True)
        fh.write("\n")
