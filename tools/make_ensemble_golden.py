#!/usr/bin/env python3
"""Fixtures of the ensemble classifiers and the Gaussian-process head from the REAL reference (needs a
checkout of the reference, ADELL_REFERENCE; no test reads it, the tests read the fixtures):

    python tools/make_ensemble_golden.py   -> tests/golden/ensemble_step_<net>.npz,
                                              tests/golden/ensemble_kernels.npz,
                                              tests/golden/ensemble_bounds.json

The reference is imported through the stub recipe of tools/make_classification_golden.py (empty
package stubs with the right __path__, then the leaf modules). ``ensemble.py`` imports ``CatNet``
from the package ``__init__``: the leaf ``classification.classification`` is imported first and
``CatNet`` set on the stub package. ``GenericEnsemble``, ``AveragingEnsemble``,
``GaussianProcessLayer``, ``UNet``, ``ResNetBackbone`` and ``CatNet`` are the real ones. Lightning is
not installed, so the arithmetic of the wrappers (classification/pl.py) is restated as in that tool:
``squeeze(net(x), 1)``, the label casts of ``calculate_loss``, the mean of the loss, one step of AdamW
(``STEP_LR``, ``STEP_EPS`` of tests/classification_cases.py) over the groups of
``configure_optimizers`` (the Gaussian-process head's parameters without decay), then a validation
step in ``eval()`` mode. ``gen2d_gp32`` is the real ``GenericEnsemble`` with its head replaced by the
real ``GaussianProcessLayer(10, 32, 3, n_outputs=3)``.

For the two Gaussian-process ensembles the precision matrix is then fitted as ``on_train_end`` does
(reset, ``forward_with_phi`` and ``update_inv_cov_from_phi`` over three batches, ``get_cov``) and
``predict_step_gp`` is restated with given standard-normal draws (``mean + sqrt(var) eps``: what
``MultivariateNormal.rsample`` computes for the diagonal covariance of ``get_parameters``; the
probabilities are taken over the class axis).

For each network this script ASSERTS that the reference's own fp32 step stays within a quarter of
the step tolerances of tests/test_ensemble_gpu.py against its fp64 step, walking the fill gain and
the input seed until that holds (``fp32_vs_fp64``). For the kernel quantities and the fitted
quantities the same ratio against ``SUM_BOUND`` is recorded in ensemble_bounds.json; where it is
above a quarter the bound the tests use is four times the recorded error.

ensemble_kernels.npz holds the fp64 intermediates the restatements of tests/ensemble_ref.py are
pinned to, from the real classes on the inputs of tests/ensemble_cases.py.
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

sys.modules["adell_mri.modules.classification.classification"].CatNet = RC.CatNet
from adell_mri.modules.activations import activation_factory  # noqa: E402
from adell_mri.modules.classification.classification import ensemble as RE  # noqa: E402
from adell_mri.modules.layers.adn_fn import get_adn_fn  # noqa: E402
from adell_mri.modules.layers.gaussian_process import GaussianProcessLayer  # noqa: E402
from adell_mri.modules.layers.res_net import ResNetBackbone  # noqa: E402
from adell_mri.modules.segmentation.unet import UNet  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ensemble_cases as C  # noqa: E402
from cases import grad_rel_err  # noqa: E402  (the gradient metric of the step tests)

OUT = os.path.join(ROOT, "tests", "golden")
# the tolerances of tests/test_ensemble_gpu.py
TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6))
SUM_BOUND = 5e-5


def rel(a, r):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-300))


def bound_entry(err):
    """The recorded error and the bound the tests use for the quantity."""
    return {"fp32_vs_fp64": err, "ratio_to_SUM_BOUND": err / SUM_BOUND,
            "bound": SUM_BOUND if err <= 0.25 * SUM_BOUND else 4.0 * err}


# ---- networks ------------------------------------------------------------------------------------------
def build(name):
    members = C.build_members(name, UNet, ResNetBackbone, RC.CatNet, get_adn_fn, activation_factory)
    kw = C.ensemble_kwargs(name, members, get_adn_fn)
    if name == "avg3":
        net = RE.AveragingEnsemble(**kw)
    else:
        net = RE.GenericEnsemble(**kw)
        n_classes, n_rff = C.CONFIGS[name][1], C.CONFIGS[name][4]
        if n_rff is not None:
            nc = 1 if n_classes == 2 else n_classes
            net.gaussian_process_head = GaussianProcessLayer(C.HEAD_STRUCTURE[-1], n_rff, n_classes,
                                                             n_outputs=nc)
    rates = C.zero_dropout(net)
    return net, rates


def loss_fn_for(name):
    return (torch.nn.BCEWithLogitsLoss() if C.CONFIGS[name][1] == 2 else torch.nn.CrossEntropyLoss())


def step_inputs(name, seed):
    shape = C.input_shape(name)
    g = torch.Generator().manual_seed(seed)
    grids = torch.meshgrid(*[torch.arange(float(s)) for s in shape[2:]], indexing="ij")
    x = torch.stack([torch.stack([torch.sin((b + 1) * 0.37 * grids[0] + c) *
                                  torch.cos((b + 2) * 0.23 * grids[1]) *
                                  (torch.cos(0.45 * grids[2] + b) if len(grids) > 2 else 1.0)
                                  for c in range(shape[1])]) for b in range(shape[0])])
    return x + 0.2 * torch.rand(shape, generator=g)


def loss_of(name, net, x, y):
    y = y.to(torch.int64) if C.CONFIGS[name][1] > 2 else y.to(x.dtype)
    prediction = torch.squeeze(net(x), 1)
    return loss_fn_for(name)(prediction, y).mean(), prediction


def probabilities(name, logits):
    return torch.sigmoid(logits) if C.CONFIGS[name][1] == 2 else torch.softmax(logits, -1)


def gp_records(name, net, x, dt):
    """Fit over three batches as ``on_train_end`` does, then ``predict_step_gp`` with given draws."""
    head = net.gaussian_process_head
    out = {}
    head.reset_inv_cov()
    for k in range(C.FIT_BATCHES):
        xb = torch.from_numpy(C.fit_inputs(x.float().numpy(), k)).to(dt)
        rows = net.prediction_head(net.forward_features(xb))
        logits, phi = head.forward_with_phi(rows)
        head.update_inv_cov_from_phi(phi, probabilities(name, logits))
    out["fit:inv_conv"] = head.inv_conv.detach().clone()
    head.get_cov()
    out["fit:cov"] = head.cov.detach().clone()
    rows = net.prediction_head(net.forward_features(x))
    gp_mean, gp_cov = head.get_parameters(rows)
    var = torch.diagonal(gp_cov, dim1=-2, dim2=-1)
    eps = torch.from_numpy(C.predict_eps(*gp_mean.shape)).to(dt)
    samples = gp_mean[None] + var.sqrt()[None] * eps[0]
    mean_samples = gp_mean[None] + var.sqrt()[None] * eps[1]
    out.update({
        "gp:prediction": net(x), "gp:gp_mean": gp_mean, "gp:gp_samples": samples,
        "gp:predictive_mean": samples.mean(0), "gp:predictive_std": samples.std(0),
        "gp:epistemic_uncertainty": var,
        "gp:predictive_std_pred": probabilities(name, samples).std(0),
        "gp:epistemic_uncertainty_pred": probabilities(name, mean_samples).std(0)})
    return {k: v.detach().clone() for k, v in out.items()}


def run_step(name, gain, x, dt):
    net, rates = build(name)
    keys = list(net.state_dict().keys())
    shapes = [tuple(v.shape) for v in net.state_dict().values()]
    named = [(k, p) for k, p in net.named_parameters()]
    net.load_state_dict(C.fill(net.state_dict(), gain))
    net = net.to(dt).train()
    x = x.to(dt)
    y = torch.tensor(C.CONFIGS[name][5])
    total, logits = loss_of(name, net, x, y)
    with torch.no_grad():
        features = None if name == "avg3" else net.forward_features(x).detach().clone()
    total.backward()
    out = {"total": total.detach(), "logits": logits.detach()}
    if features is not None:
        out["features"] = features
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        out["grad:" + k] = p.grad.clone()
    groups, base_wd = C.step_groups(named, C.CONFIGS[name][6])
    by_name = dict(net.named_parameters())
    torch.optim.AdamW([{"params": [by_name[n] for n in names], "weight_decay": wd}
                       for names, wd in groups], lr=C.STEP_LR, weight_decay=base_wd,
                      eps=C.STEP_EPS).step()
    net.eval()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            out["step1:" + k] = v.detach().clone()
        vtotal, vlogits = loss_of(name, net, x, y)
        out["val_total"] = vtotal.detach()
        out["val_logits"] = vlogits.detach()
        if name in C.GP_NETS:
            out.update(gp_records(name, net, x, dt))
    return out, [k for k, _ in named], keys, shapes, rates, groups, base_wd


class _Grads(dict):
    """What tests/cases.py::grad_rel_err reads from a fixture: ``files`` and items."""

    @property
    def files(self):
        return list(self)


def within_quarter(o32, o64):
    """The reference's fp32 step against its fp64 step, at a quarter of every step tolerance; the
    fitted quantities as ratios of their own largest magnitude."""
    q = 0.25
    worst, ok, fitted = {}, True, {}
    for k in ("total", "val_total"):
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
        elif k.startswith(("fit:", "gp:")) or k == "features":
            fitted[k] = rel(a.numpy(), r.numpy())
    return bool(ok), worst, fitted


def gen_steps(bounds):
    for name in C.NETS:
        found = None
        for gain in (2.0, 1.5, 1.0, 3.0, 5.0):
            for seed in range(7, 7 + 6):
                x = step_inputs(name, seed)
                o64, names, keys, shapes, rates, groups, base_wd = run_step(name, gain, x,
                                                                            torch.float64)
                o32 = run_step(name, gain, x, torch.float32)[0]
                ok, worst, fitted = within_quarter(o32, o64)
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
        if "fit:inv_conv" in o64:
            P = o64["fit:inv_conv"][0].numpy()
            print(f"{name}: condition number of the fitted precision {np.linalg.cond(P):.2f}")
        bounds[name] = {k: bound_entry(e) for k, e in sorted(fitted.items())}
        out = {"x": x.numpy(), "y": np.array(C.CONFIGS[name][5]), "gain": np.float64(found[0]),
               "seed": np.int32(found[1]), "dropout_rates": np.array(rates, dtype=np.float64),
               "param_keys": np.array(names), "state_keys": np.array(keys),
               "state_shapes": np.array([",".join(str(d) for d in s) for s in shapes]),
               "fp32_vs_fp64": np.array([worst[k] for k in sorted(worst)]),
               "fp32_vs_fp64_names": np.array(sorted(worst)),
               "groups:n": np.int32(len(groups)), "groups:base_wd": np.float64(base_wd)}
        for i, (members, wd) in enumerate(groups):
            out[f"groups:{i}:names"] = np.array(members, dtype=str)
            out[f"groups:{i}:wd"] = np.float64(wd)
        for k, v in o64.items():
            if k.endswith("total") or k.startswith(("fit:", "gp:")) or k == "features":
                out[k] = v.numpy()                      # fp64
            elif v.is_floating_point():
                out[k] = v.float().numpy()
            else:
                out[k] = v.numpy()
        print(f"{name}: gain {found[0]}, seed {found[1]}, total {float(o64['total']):.6f}, val "
              f"{float(o64['val_total']):.6f}, logit spread {spread:.3e}, "
              f"fp32 vs fp64 (1 = the tolerance; loss / grad relative): {worst}; fitted {fitted}")
        path = os.path.join(OUT, f"ensemble_step_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: {os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1 << 20


# ---- kernel cases --------------------------------------------------------------------------------------
def gp_layer(shape, case, normalize, dt, n_classes=2, ordinal=False, m=0.999):
    N, i, r, o = shape
    layer = GaussianProcessLayer(i, r, n_classes, n_outputs=o, m=m, ordinal=ordinal,
                                 normalize_input=normalize)
    sd = layer.state_dict()
    sd["W"], sd["b"] = torch.from_numpy(case["W"]), torch.from_numpy(case["b"])
    sd["weights"] = torch.from_numpy(case["weights"])
    if normalize:
        sd["input_norm.weight"] = torch.from_numpy(case["gamma"])
        sd["input_norm.bias"] = torch.from_numpy(case["beta"])
    layer.load_state_dict(sd)
    return layer.to(dt)


def kernel_records(dt):
    out = {}
    with torch.no_grad():
        for shape in C.GP_SHAPES + [C.GP_COMPOSED_SHAPE]:
            case = C.gp_case(shape)
            tag = "x".join(str(v) for v in shape)
            for normalize in (True, False):
                layer = gp_layer(shape, case, normalize, dt)
                logits, phi = layer.forward_with_phi(torch.from_numpy(case["x"]).to(dt))
                out[f"gp:{tag}:{int(normalize)}:phi"] = phi
                out[f"gp:{tag}:{int(normalize)}:logits"] = logits
        case = C.gp_case(C.PRECISION_SHAPE)
        for kind, (n_classes, ordinal, _) in C.PRECISION_KINDS.items():
            probs = C.precision_batches(kind)
            for momentum in (False, True):
                layer = gp_layer(C.PRECISION_SHAPE, case, True, dt, n_classes, ordinal, C.PRECISION_M)
                for k, p in enumerate(probs):
                    x = torch.from_numpy(C.gp_case(C.PRECISION_SHAPE, seed=200 + k)["x"]).to(dt)
                    layer.update_inv_cov(x, torch.from_numpy(p).to(dt), use_momentum=momentum)
                out[f"prec:{kind}:{int(momentum)}:P"] = layer.inv_conv[0].clone()
                if not momentum and kind in ("binary", "multi3"):
                    layer.get_cov()
                    x0 = torch.from_numpy(C.gp_case(C.PRECISION_SHAPE, seed=200)["x"]).to(dt)
                    _, cov = layer.get_parameters(x0)
                    out[f"prec:{kind}:cov"] = layer.cov[0].clone()
                    out[f"prec:{kind}:var"] = torch.diagonal(cov, dim1=-2, dim2=-1)[:, 0].clone()
        members = [torch.from_numpy(C.pool_member(s)).to(dt) for s in C.POOL_MEMBERS]
        ens = RE.GenericEnsemble(3, [torch.nn.Identity() for _ in members],
                                 [s[1] for s in C.POOL_MEMBERS], [4], 2,
                                 head_adn_fn=get_adn_fn(1, "batch", "swish", 0.0))
        out["pool:features"] = ens.forward_features(members)
    return {k: v.double().numpy() for k, v in out.items()}


def gen_kernels(bounds):
    k64, k32 = kernel_records(torch.float64), kernel_records(torch.float32)
    worst = {}
    for k in k64:
        if k.startswith("pool:"):
            assert np.array_equal(k32[k], k64[k])
            continue
        q = k.split(":")[-1]
        q = {"P": "precision", "cov": "covariance", "var": "variance"}.get(q, q)
        worst[q] = max(worst.get(q, 0.0), rel(k32[k], k64[k]))
    bounds["kernels"] = {q: bound_entry(e) for q, e in sorted(worst.items())}
    print("kernel quantities, the reference's fp32 against fp64:", worst)
    path = os.path.join(OUT, "ensemble_kernels.npz")
    np.savez_compressed(path, **k64)
    print(f"{path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < 1 << 19


if __name__ == "__main__":
    bounds = {"SUM_BOUND": SUM_BOUND}
    gen_kernels(bounds)
    gen_steps(bounds)
    with open(os.path.join(OUT, "ensemble_bounds.json"), "w") as fh:
        json.dump(bounds, fh, indent=1, sort_keys=True)
        fh.write("\n")
