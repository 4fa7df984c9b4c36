#!/usr/bin/env python3
"""Fixture of the classification networks and losses from the REAL reference (needs a checkout of the
reference, ADELL_REFERENCE; no test reads it, the tests read the fixture):

    python tools/make_classification_golden.py       -> tests/golden/classification_step_*.npz

The reference is imported through the stub recipe of tools/make_mae_golden.py (empty package stubs
with the right __path__, then the leaf modules): its ``CatNet``, ``OrdNet``, ``ViTClassifier`` and
``OrdinalSigmoidalLoss`` are the real ones, ``classification.py``, ``losses.py`` and their layer
imports being pure torch. Lightning is not installed, so the arithmetic of the wrappers
(``ClassPLABC`` / ``OrdNetPL``, classification/pl.py) is restated here: ``squeeze(net(x), 1)``, the
label casts of ``calculate_loss``, the mean of the loss (the sum ``loss + roc_loss`` for the ordinal
network), one step of AdamW (``learning_rate`` 1e-4 and ``optimizer_eps`` 1e-2: see
tests/classification_cases.py) over the groups of ``configure_optimizers`` -- the
empty no-decay group, ``ordinal_bias`` at a hundredth of the weight decay, the rest; the head / body
split when the weight decay is a pair -- with ``weight_decay=base_wd``, then a validation step in
``eval()`` mode (what Lightning's validation loop sets).

Five networks (tests/classification_cases.py). After construction every ``torch.nn.Dropout`` has its
``p`` set to 0 (the heads' 0.1 is hard-coded and would make the step random), so the training step
runs in ``train()`` mode: batch norm uses the batch statistics and updates its running buffers,
which are recorded with the parameters. For each network this script ASSERTS that the reference's
own fp32 step stays within a quarter of the step tolerances of tests/test_classification_gpu.py
against its fp64 step, walking the fill gain and the input seed until that holds; the ratios are
recorded.

Besides the steps the file holds small loss cases (``l*``: fp32 inputs, fp64 results and gradients)
from the real ``OrdinalSigmoidalLoss`` (with ``relative_order_consistency``),
``torch.nn.BCEWithLogitsLoss`` and ``torch.nn.CrossEntropyLoss``, to which
tests/classification_ref.py is pinned, the recorded numpy draws of ``BatchPreprocessing``, and a
table of ``label_to_ordinal`` / ``ordinal_prediction_to_class``.
"""
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
from adell_mri.utils.batch_preprocessing import BatchPreprocessing  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from cases import grad_rel_err  # noqa: E402  (the gradient metric of the step tests)
from classification_cases import (CONFIGS, NETS, STEP_EPS, STEP_LR, fill, net_kwargs,  # noqa: E402
                                  step_groups, zero_dropout)

OUT = os.path.join(ROOT, "tests", "golden")
# the step tolerances of tests/test_classification_gpu.py (those of tests/test_mae_gpu.py)
TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6))


def build(name):
    cls, _, _, _, _, _ = CONFIGS[name]
    kw = net_kwargs(name)
    if cls != "ViTClassifier":
        kw["adn_fn"] = get_adn_fn(3, "batch", "swish", 0.0)
    net = getattr(RC, cls)(**kw)
    rates = zero_dropout(net)
    return net, rates


def loss_fn_for(name, dt):
    _, kw, _, _, weights, _ = CONFIGS[name]
    w = None if weights is None else torch.tensor(weights, dtype=dt)
    if kw["n_classes"] == 2:
        return torch.nn.BCEWithLogitsLoss(w)
    if name.startswith("ord"):
        return OrdinalSigmoidalLoss(kw["n_classes"], w)
    return torch.nn.CrossEntropyLoss(w)


def step_inputs(name, seed):
    shape = CONFIGS[name][2]
    g = torch.Generator().manual_seed(seed)
    grids = torch.meshgrid(*[torch.arange(float(s)) for s in shape[2:]], indexing="ij")
    x = torch.stack([torch.stack([torch.sin((b + 1) * 0.37 * grids[0] + c) *
                                  torch.cos((b + 2) * 0.23 * grids[1]) for c in range(shape[1])])
                     for b in range(shape[0])])
    return x + 0.2 * torch.rand(shape, generator=g)


def losses_of(name, net, loss_fn, x, y):
    """The wrapper's step arithmetic: (what is returned, its parts, the logits)."""
    n_classes = CONFIGS[name][1]["n_classes"]
    y = y.to(torch.int64) if n_classes > 2 else y.to(x.dtype)      # calculate_loss's casts
    if name.startswith("ord"):
        prediction, pre_bias = net(x, return_pre_bias=True)
        prediction = torch.squeeze(prediction, 1)
        loss, roc = loss_fn(prediction, y, pre_bias=pre_bias)
        loss, roc = loss.mean(), roc.mean()
        return loss + roc, {"loss": loss, "roc_loss": roc}, prediction, pre_bias
    prediction = torch.squeeze(net(x), 1)
    loss = loss_fn(prediction, y).mean()
    return loss, {"loss": loss}, prediction, None


def run_step(name, gain, x, dt):
    net, rates = build(name)
    keys = list(net.state_dict().keys())
    named = [(k, p) for k, p in net.named_parameters()]
    net.load_state_dict(fill(net.state_dict(), gain))
    if name.startswith("ord"):          # OrdNet's constructor zeroes it; the fill must not undo that
        with torch.no_grad():
            net.classification_layer.op[-1].bias.zero_()
    net = net.to(dt).train()
    x = x.to(dt)
    y = torch.tensor(CONFIGS[name][3])
    loss_fn = loss_fn_for(name, dt)
    total, parts, logits, pre_bias = losses_of(name, net, loss_fn, x, y)
    total.backward()
    out = {"total": total.detach(), "logits": logits.detach()}
    out.update({k: v.detach() for k, v in parts.items()})
    if pre_bias is not None:
        out["pre_bias"] = pre_bias.detach()
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        out["grad:" + k] = p.grad.clone()
    groups, base_wd = step_groups(named, CONFIGS[name][5])
    by_name = dict(net.named_parameters())
    torch.optim.AdamW([{"params": [by_name[n] for n in names], "weight_decay": wd}
                       for names, wd in groups], lr=STEP_LR, weight_decay=base_wd,
                      eps=STEP_EPS).step()
    net.eval()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if not k.startswith("feature_extraction."):      # the same tensors as ``res_net.*``
                out["step1:" + k] = v.detach().clone()
        vtotal, vparts, vlogits, _ = losses_of(name, net, loss_fn, x, y)
        out["val_total"] = vtotal.detach()
        out["val_logits"] = vlogits.detach()
        out.update({"val_" + k: v.detach() for k, v in vparts.items()})
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
    for k in o64:
        if k.endswith("total") or k.endswith("loss"):
            worst[k] = abs(float(o32[k]) - float(o64[k])) / abs(float(o64[k]))
            ok &= worst[k] <= q * TOL["loss"]
    worst["grad"] = worst["param"] = 0.0
    grads = _Grads({k: v.numpy() for k, v in o64.items() if k.startswith("grad:")})
    for k in o64:
        a, r = o32[k].double(), o64[k].double()
        if k.startswith("grad:"):
            e = grad_rel_err(grads, k[5:], o32[k].double().numpy())
            worst["grad"] = max(worst["grad"], e)
            ok &= e <= q * TOL["grad"]
        elif k.startswith("step1:") and o64[k].is_floating_point():
            rt, at = TOL["param"]
            e = float(((a - r).abs() / (at + rt * r.abs())).max())     # <= 1 passes assert_allclose
            worst["param"] = max(worst["param"], e)
            ok &= e <= q
    return bool(ok), worst


# ---- small loss cases: fp32 inputs, the reference's fp64 results and gradients ----------------------
# name: (kind, B, K, weights, seed); logits include +-90
LOSS_CASES = {
    "l_bce": ("bce", 5, 1, None, 1), "l_bce_w1": ("bce", 3, 1, "one", 2),
    "l_bce_wb": ("bce", 4, 1, "item", 3), "l_ce": ("ce", 5, 3, None, 4),
    "l_ce_w": ("ce", 6, 5, "class", 5), "l_ord": ("ordinal", 6, 4, None, 6),
    "l_ord_w": ("ordinal", 5, 5, "class", 7),
}


def loss_case_inputs(kind, B, K, weights, seed):
    g = torch.Generator().manual_seed(seed)
    W = {"bce": 1, "ce": K, "ordinal": K - 1}[kind]
    x = (torch.rand((B, W), generator=g) * 8 - 4)
    x[0, 0], x[-1, -1] = 90.0, -90.0
    if kind == "bce":
        y = torch.rand((B,), generator=g)              # soft targets
        y[0] = 1.0
    else:
        y = torch.randint(0, K, (B,), generator=g)
        y[0], y[-1] = K - 1, 0
    w = None
    if weights == "one":
        w = torch.tensor([0.7])
    elif weights == "item":
        w = torch.rand((B,), generator=g) + 0.25
    elif weights == "class":
        w = torch.rand((K,), generator=g) + 0.25
        w[1] = 0.0                                     # a class weight of zero
    return x, y, w


def gen_loss_cases():
    out = {"loss_cases": np.array(list(LOSS_CASES))}
    for name, (kind, B, K, weights, seed) in LOSS_CASES.items():
        x, y, w = loss_case_inputs(kind, B, K, weights, seed)
        xd = x.double().requires_grad_(True)
        wd = None if w is None else w.double()
        rec = {"kind": np.array(kind), "K": np.int32(K), "x": x.numpy(), "y": y.numpy()}
        if w is not None:
            rec["w"] = w.numpy()
        if kind == "bce":
            loss = torch.nn.BCEWithLogitsLoss(wd)(xd[:, 0], y.double())
            item = torch.nn.BCEWithLogitsLoss(wd, reduction="none")(xd[:, 0], y.double())
        elif kind == "ce":
            loss = torch.nn.CrossEntropyLoss(wd)(xd, y)
            item = torch.nn.CrossEntropyLoss(wd, reduction="none")(xd, y)
        else:
            pre = x[:, :1].double().requires_grad_(True)
            item, roc = OrdinalSigmoidalLoss(K, wd)(xd, y, pre_bias=pre)
            loss = item.mean()
            dpre, = torch.autograd.grad(roc, pre)
            rec.update({"roc": roc.detach().numpy(), "dpre": dpre.numpy()})
        dx, = torch.autograd.grad(loss, xd)
        rec.update({"item": item.detach().numpy(), "loss": loss.detach().numpy(), "dx": dx.numpy()})
        out.update({f"{name}:{k}": v for k, v in rec.items()})
    return out


def gen_draws():
    """The numpy draws of the real ``BatchPreprocessing`` for two calls each, read off the labels:
    with y = one-hot rows the mixed labels give the factor and the partner of every item."""
    out = {}
    for name, (alpha, partial, seed) in {"mixup": (0.4, None, 42), "partial": (0.4, 0.5, 7)}.items():
        bp = BatchPreprocessing(None, alpha, partial, seed)
        g = np.random.default_rng(seed)
        for call in range(2):
            B = 6
            if partial is None:
                factor = g.beta(alpha, alpha, B)
                perm = g.permutation(B)
                selected = np.ones(B, dtype=bool)
            else:
                selected = g.binomial(1, partial, B).astype(bool)
                factor = np.ones(B)
                factor[selected] = g.beta(alpha, alpha, selected.sum())
                perm = g.permutation(B)
            x = torch.arange(B * 3, dtype=torch.float32).reshape(B, 3)
            want = x.clone()
            f32 = torch.as_tensor(factor, dtype=torch.float32)[:, None]
            mixed = x * f32 + x[perm] * (1.0 - f32)
            want[selected] = mixed[selected]
            got, _ = bp(x.clone(), torch.zeros(B))
            assert torch.equal(got, want), f"{name}: the restated draw order is not the reference's"
            out.update({f"draws:{name}:{call}:factor": factor, f"draws:{name}:{call}:perm": perm,
                        f"draws:{name}:{call}:selected": selected})
        out[f"draws:{name}:args"] = np.array([alpha, -1.0 if partial is None else partial, seed])
    return out


def gen_tables():
    labels = torch.tensor([[0], [1], [2], [3], [4]])
    probs = torch.tensor([[0.9, 0.8, 0.2], [0.1, 0.2, 0.3], [0.6, 0.6, 0.6], [0.5, 0.7, 0.4]])
    return {"table:labels": labels.numpy(),
            "table:ordinal": RC.label_to_ordinal(labels, 5).numpy(),
            "table:ordinal_keep0": RC.label_to_ordinal(labels, 5, ignore_0=False).numpy(),
            "table:probs": probs.numpy(),
            "table:classes": RC.ordinal_prediction_to_class(probs).numpy()}


def gen_step():
    out = gen_loss_cases()
    out.update(gen_draws())
    out.update(gen_tables())
    out["nets"] = np.array(list(NETS))
    for name in NETS:
        found = None
        for gain in (2.0, 1.5, 1.0, 3.0, 5.0):
            for seed in range(7, 7 + 6):
                x = step_inputs(name, seed)
                o64, names, keys, rates, groups, base_wd = run_step(name, gain, x, torch.float64)
                o32, _, _, _, _, _ = run_step(name, gain, x, torch.float32)
                ok, worst = within_quarter(o32, o64)
                # the logits must differ between items, or the step pins nothing
                spread = float(o64["logits"].std(0).mean())
                if ok and spread > 1e-3:
                    found = (gain, seed)
                    break
            if found:
                break
        if not found:
            raise SystemExit(f"{name}: no (gain, seed) keeps the reference's fp32 step within a "
                             f"quarter of the tolerances; last worst {worst}")
        other = (0.05, 0.1) if not isinstance(CONFIGS[name][5], tuple) else 0.05
        net, _ = build(name)
        other_groups, other_base = step_groups(list(net.named_parameters()), other)
        out.update({f"{name}:x": x.numpy(), f"{name}:gain": np.float64(found[0]),
                    f"{name}:seed": np.int32(found[1]), f"{name}:dropout_rates": np.array(rates),
                    f"{name}:param_keys": np.array(names), f"{name}:state_keys": np.array(keys),
                    f"{name}:fp32_vs_fp64": np.array([worst[k] for k in sorted(worst)]),
                    f"{name}:fp32_vs_fp64_names": np.array(sorted(worst))})
        for tag, (grp, base) in {"groups": (groups, base_wd), "groups_other": (other_groups,
                                                                                 other_base)}.items():
            out[f"{name}:{tag}:n"] = np.int32(len(grp))
            out[f"{name}:{tag}:base_wd"] = np.float64(base)
            for i, (members, wd) in enumerate(grp):
                out[f"{name}:{tag}:{i}:names"] = np.array(members, dtype=str)
                out[f"{name}:{tag}:{i}:wd"] = np.float64(wd)
        for k, v in o64.items():
            if k.endswith("total") or k.endswith("loss"):
                out[f"{name}:{k}"] = v.numpy()
            elif v.is_floating_point():
                out[f"{name}:{k}"] = v.float().numpy()
            else:
                out[f"{name}:{k}"] = v.numpy()
        print(f"{name}: gain {found[0]}, seed {found[1]}, total {float(o64['total']):.6f}, val "
              f"{float(o64['val_total']):.6f}, logit spread {spread:.3e}, "
              f"fp32 vs fp64 (1 = the tolerance; loss / grad relative): {worst}")
    # one file per network (a committed file stays below 1 MiB) and one for everything else
    files = {name: {k: v for k, v in out.items() if k.startswith(name + ":")} for name in NETS}
    files["cases"] = {k: v for k, v in out.items() if k.split(":")[0] not in NETS}
    for tag, part in files.items():
        path = os.path.join(OUT, f"classification_step_{tag}.npz")
        np.savez_compressed(path, **part)
        print(f"{path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    gen_step()
