#!/usr/bin/env python3
"""Fixtures of DINO from the REAL reference (needs a checkout of the reference, ADELL_REFERENCE; no
test reads it, the tests read the fixtures):

    python tools/make_dino_golden.py        -> tests/golden/dino_loss.npz
                                               tests/golden/ssl_dino_step.npz

The reference is imported through the stub recipe of SURVEY.md section 8c (empty package stubs with
the right __path__, then the leaf modules): its ``DINO`` and ``DinoLoss`` are the real classes.
Lightning is not installed, so the arithmetic of ``DINOPL.step`` (pl.py:1241-1270: both views stacked
through the student, the teacher under no_grad on the same stack, L(s1, t2) / 2 + L(s2, t1) / 2, the
centre update from cat[t1, t2]), the AdamW step of ``configure_optimizers`` and the EMA update
(utils/utils.py:484-487) are restated here, as oracle/make_golden.py does for the ConvNeXt step.

``dino_loss.npz``: small loss cases -- inputs, centres, temperatures, the reference in fp64 (loss, da,
db), its own fp32 results, and the Sinkhorn-Knopp scores as it returns them.

``ssl_dino_step.npz``: one training step of two networks (2-D without a class token: the
feature-mean path; 3-D with a class token and two registers). Softmaxes at temperature 0.1 are
sharp, so whether fp32 can follow fp64 through a step is a condition on the inputs: for each network
this script ASSERTS and records that the reference's own fp32 step stays within a quarter of the
step tolerances of tests/test_dino_gpu.py against its fp64 step, and walks the fill gain and the
seed until that holds (what breaks it first are the parameters whose gradient is zero in exact
arithmetic, the k-norm biases: AdamW turns their fp32 rounding noise into a step of its own size)
and the student's outputs still differ between the items of the batch.
"""
import copy
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
    ("adell_mri.modules.self_supervised", "adell_mri/modules/self_supervised"),
    ("adell_mri.modules.self_supervised.losses", "adell_mri/modules/self_supervised/losses"),
]:
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(REF, path)]
    sys.modules[name] = m
import einops.layers.torch  # noqa: E402,F401  (the reference uses it via bare `import einops`)
import torch  # noqa: E402

from adell_mri.modules.layers.adn_fn import get_adn_fn  # noqa: E402
from adell_mri.modules.self_supervised.dino import DINO  # noqa: E402
from adell_mri.modules.self_supervised.losses.dino import DinoLoss  # noqa: E402

from oracle.weights import fill_state_dict  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from cases import grad_rel_err  # noqa: E402  (the gradient metric of the step tests)

OUT = os.path.join(ROOT, "tests", "golden")

# name: (shape, (t1, t2), seed); inputs uniform in [-1, 1] as the normalised head produces them
LOSS_CASES = {
    "r1k5": ((1, 5), (0.1, 0.04), 1),
    "r3k37": ((3, 37), (0.1, 0.04), 2),
    "r6k300": ((6, 300), (0.1, 0.1), 3),
    "nd": ((2, 3, 257), (0.1, 0.04), 4),
}


def rel(a, r):
    return float((a.double() - r.double()).abs().max() / (r.double().abs().max() + 1e-300))


def gen_loss_cases():
    out = {"cases": np.array(list(LOSS_CASES))}
    for name, (shape, (t1, t2), seed) in LOSS_CASES.items():
        g = torch.Generator().manual_seed(seed)
        a = torch.rand(shape, generator=g) * 2 - 1
        b = torch.rand(shape, generator=g) * 2 - 1
        centers = 0.2 * (torch.rand((shape[-1],), generator=g) * 2 - 1)
        out.update({f"{name}:a": a.numpy(), f"{name}:b": b.numpy(),
                    f"{name}:centers": centers.numpy(),
                    f"{name}:t": np.array([t1, t2], dtype=np.float64)})
        for method in ("center", "sk"):
            res = {}
            for dt in (torch.float64, torch.float32):
                crit = DinoLoss((t1, t2), shape[-1], teacher_score_method=method).to(dt)
                crit.centers.copy_(centers.to(dt))
                x = a.to(dt).clone().requires_grad_(True)
                y = b.to(dt).clone().requires_grad_(method == "center")
                loss = crit(x, y)
                loss.backward()
                res[dt] = (loss.detach(), x.grad, y.grad)
            l64, da64, db64 = res[torch.float64]
            l32, da32, db32 = res[torch.float32]
            out[f"{name}:{method}:loss"] = l64.numpy()
            out[f"{name}:{method}:da"] = da64.numpy()
            out[f"{name}:{method}:loss_fp32"] = l32.numpy()
            out[f"{name}:{method}:da_fp32"] = da32.numpy()
            msg = f"{name} {method}: loss {float(l64):.6f}, fp32 own error loss " \
                  f"{abs(float(l32) - float(l64)) / abs(float(l64)):.1e}, da {rel(da32, da64):.1e}"
            if method == "center":
                out[f"{name}:{method}:db"] = db64.numpy()
                out[f"{name}:{method}:db_fp32"] = db32.numpy()
                msg += f", db {rel(db32, db64):.1e}"
            else:
                crit = DinoLoss((t1, t2), shape[-1], teacher_score_method="sk")
                out[f"{name}:sk:scores"] = crit.sinkhorn_knopp_teacher(b).numpy()   # fp32, as returned
            print(msg)
    np.savez_compressed(os.path.join(OUT, "dino_loss.npz"), **out)


# ---- one training step ---------------------------------------------------------------------------
STEP_OPT = dict(lr=1e-3, weight_decay=1e-6, eps=1e-8)      # DINOPL's defaults
EMA_DECAY = 0.99
CENTER_M = 0.9
TEMPERATURE = 0.1
B = 3
# the step tolerances of tests/test_dino_gpu.py (those of tests/test_ssl.py:221-246)
TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6), ema=(1e-5, 1e-7), centers=1e-4)


def step_nets():
    adn = get_adn_fn(1, "identity", "gelu", 0.0)
    return {
        "net2d": dict(backbone_args=dict(image_size=[32, 32], patch_size=[4, 4], in_channels=1,
                                         number_of_blocks=2, attention_dim=64, hidden_dim=64,
                                         n_heads=4, mlp_structure=[64], adn_fn=adn,
                                         use_class_token=False),
                      projection_head_args=dict(structure=[64, 32], adn_fn=adn), out_dim=48),
        "net3d": dict(backbone_args=dict(image_size=[16, 16, 8], patch_size=[4, 4, 4], in_channels=2,
                                         number_of_blocks=2, attention_dim=32, hidden_dim=32,
                                         embedding_size=32, n_heads=4, mlp_structure=[64],
                                         adn_fn=adn, use_class_token=True, n_registers=2),
                      projection_head_args=dict(structure=[48, 24], adn_fn=adn), out_dim=40),
    }


def step_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    ba = cfg["backbone_args"]
    shape = (B, ba["in_channels"], *ba["image_size"])
    grids = torch.meshgrid(*[torch.arange(float(s)) for s in ba["image_size"]], indexing="ij")
    x1 = torch.stack([torch.stack([torch.sin((b + 1) * 0.37 * grids[0] + c) *
                                   torch.cos((b + 2) * 0.23 * grids[1]) for c in range(shape[1])])
                      for b in range(B)])
    x1 = x1 + 0.2 * torch.rand(shape, generator=g)
    x2 = x1.flip(2) + 0.3 * torch.randn(shape, generator=g)
    centers = 0.1 * (torch.rand((cfg["out_dim"],), generator=g) * 2 - 1)
    return x1, x2, centers


def run_step(cfg, gain, x1, x2, centers, dt):
    """DINOPL.step + AdamW + EMA + centre update in dtype ``dt`` on the real DINO / DinoLoss."""
    net = DINO(**copy.deepcopy({k: v for k, v in cfg.items()}))
    net.load_state_dict(fill_state_dict(net.state_dict(), gain=gain))
    net = net.to(dt).train()
    net.last_layer_.parametrizations.weight.original0.requires_grad = False
    shadow = copy.deepcopy(net).eval()
    crit = DinoLoss((TEMPERATURE, TEMPERATURE), cfg["out_dim"], center_m=CENTER_M).to(dt)
    crit.centers.copy_(centers.to(dt))
    stacked = torch.cat([x1, x2]).to(dt)
    s_1, s_2 = net(stacked).split([B, B], dim=0)
    with torch.no_grad():
        t_1, t_2 = shadow(stacked).detach().split([B, B], dim=0)
    loss = torch.add(crit(s_1, t_2) / 2.0, crit(s_2, t_1) / 2.0)
    loss.backward()
    out = {"loss": loss.detach(), "student": torch.cat([s_1, s_2]).detach(),
           "teacher": torch.cat([t_1, t_2]).detach()}
    names = [k for k, _ in net.named_parameters()]
    for k, p in net.named_parameters():
        if p.grad is not None:
            out["grad:" + k] = p.grad.clone()
    decay, no_decay = [], []
    for k, p in net.named_parameters():
        (no_decay if "normalization" in k else decay).append(p)
    torch.optim.AdamW(decay + no_decay, **STEP_OPT).step()
    sh = dict(shadow.named_parameters())
    with torch.no_grad():
        for k, p in net.named_parameters():
            out["step1:" + k] = p.detach().clone()
            sh[k].sub_((1 - EMA_DECAY) * (sh[k] - p.detach()))
            out["ema1:" + k] = sh[k].detach().clone()
    crit.update_centers(torch.cat([t_1, t_2]))
    out["center_sum"] = crit.async_batch_center.detach().clone()
    crit.apply_center_update()
    out["centers1"] = crit.centers.detach().reshape(-1).clone()
    return out, names, list(net.state_dict().keys())


class _Grads(dict):
    """What tests/cases.py::grad_rel_err reads from a fixture: ``files`` and items."""

    @property
    def files(self):
        return list(self)


def within_quarter(o32, o64):
    """The reference's fp32 step against its fp64 step, at a quarter of every step tolerance."""
    q = 0.25
    worst = {"loss": abs(float(o32["loss"]) - float(o64["loss"])) / abs(float(o64["loss"]))}
    ok = worst["loss"] <= q * TOL["loss"]
    worst["grad"] = worst["param"] = worst["ema"] = 0.0
    grads = _Grads({k: v.numpy() for k, v in o64.items() if k.startswith("grad:")})
    for k in o64:
        a, r = o32[k].double(), o64[k].double()
        if k.startswith("grad:"):
            e = grad_rel_err(grads, k[5:], o32[k].double().numpy())
            worst["grad"] = max(worst["grad"], e)
            ok &= e <= q * TOL["grad"]
        elif k.startswith("step1:") or k.startswith("ema1:"):
            rt, at = TOL["param"] if k.startswith("step1:") else TOL["ema"]
            e = float(((a - r).abs() / (at + rt * r.abs())).max())     # <= 1 passes assert_allclose
            key = "param" if k.startswith("step1:") else "ema"
            worst[key] = max(worst[key], e)
            ok &= e <= q
    for k in ("center_sum", "centers1"):
        a, r = o32[k].double().reshape(-1), o64[k].double().reshape(-1)
        e = float(((a - r).abs() / (TOL["centers"] * r.abs())).max())
        worst[k] = e
        ok &= e <= q
    return bool(ok), worst


def gen_step():
    out = {"B": np.int32(B), "ema_decay": np.float64(EMA_DECAY), "center_m": np.float64(CENTER_M),
           "temperature": np.float64(TEMPERATURE), "nets": np.array(list(step_nets()))}
    for name, cfg in step_nets().items():
        found = None
        for gain in (3.0, 2.0, 1.5, 1.0, 0.7, 0.5):
            for seed in range(7, 7 + 6):
                x1, x2, centers = step_inputs(cfg, seed)
                o64, names, keys = run_step(cfg, gain, x1, x2, centers, torch.float64)
                o32, _, _ = run_step(cfg, gain, x1, x2, centers, torch.float32)
                ok, worst = within_quarter(o32, o64)
                # the outputs must differ between items, or the step pins nothing
                spread = float(o64["student"].std(0).mean())
                if ok and spread > 1e-4:
                    found = (gain, seed)
                    break
            if found:
                break
        if not found:
            raise SystemExit(f"{name}: no (gain, seed) keeps the reference's fp32 step within a "
                             f"quarter of the tolerances; last worst {worst}")
        assert ok
        out.update({f"{name}:x1": x1.numpy(), f"{name}:x2": x2.numpy(),
                    f"{name}:centers0": centers.numpy(), f"{name}:gain": np.float64(found[0]),
                    f"{name}:seed": np.int32(found[1]),
                    f"{name}:param_keys": np.array(names), f"{name}:state_keys": np.array(keys),
                    f"{name}:fp32_vs_fp64": np.array([worst[k] for k in sorted(worst)]),
                    f"{name}:fp32_vs_fp64_names": np.array(sorted(worst))})
        for k, v in o64.items():
            out[f"{name}:{k}"] = v.float().numpy() if k != "loss" else v.numpy()
        print(f"{name}: gain {found[0]}, seed {found[1]}, loss {float(o64['loss']):.6f}, student "
              f"spread {spread:.3e}, fp32 vs fp64 (1 = the tolerance, loss / grad relative): {worst}")
    np.savez_compressed(os.path.join(OUT, "ssl_dino_step.npz"), **out)


if __name__ == "__main__":
    gen_loss_cases()
    gen_step()
