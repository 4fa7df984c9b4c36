#!/usr/bin/env python3
"""Fixture of iBOT from the REAL reference (needs a checkout of the reference, ADELL_REFERENCE; no
test reads it, the tests read the fixture):

    python tools/make_ibot_golden.py        -> tests/golden/ibot_step.npz
                                               tests/golden/ibot_step_params.npz

(the second file holds the parameters and the EMA after the step, ``<net>:step1:*`` and
``<net>:ema1:*``: with them one file would pass the size limit of a committed file.)

The reference is imported through the stub recipe of tools/make_dino_golden.py (empty package stubs
with the right __path__, then the leaf modules): its ``iBOT``, ``DinoLoss`` and
``GenericTransformerMasker`` are the real classes. Besides the step the file holds two small per-view
cases (``v2d``, ``v3d``: the real masker's draw and splice, ``iBOT.reduce`` and ``DinoLoss`` in either
teacher mode on random fp32 logits, the reference's results in fp64) to which tests/ibot_ref.py is
pinned. Lightning is not installed, so the arithmetic of
``iBOTPL.step`` (the student on both views with two consecutive masker draws, the teacher under
no_grad without masking, both centre updates BEFORE the losses, L_g(s_red_1, t_red_2) / 2 +
L_g(s_red_2, t_red_1) / 2 across the views, L_m(s_1[:, m1], t_1[:, m1]) / 2 + L_m(s_2[:, m2],
t_2[:, m2]) / 2 within them, their sum), the AdamW step of ``configure_optimizers`` and the EMA
update are restated here, as make_dino_golden.py does for ``DINOPL``.

Two networks, the two of tests/dino_cases.py with a masker (tests/ibot_cases.py::step_config): 2-D
without a class token and "mean"; 3-D with a class token, two registers and "cls" -- there the
coordinates keep their ``+ skip_n`` offset of 3 on the patch tokens, as the reference has it. For
each network this script ASSERTS and records that the reference's own fp32 step stays within a
quarter of the step tolerances of tests/test_ibot_gpu.py against its fp64 step, walking the fill
gain and the seed until that holds and the student's outputs differ between the items; and that no
drawn coordinate set reaches the number of patch tokens (an IndexError in the reference).
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

from adell_mri.modules.self_supervised.ibot import iBOT  # noqa: E402
from adell_mri.modules.self_supervised.losses.dino import DinoLoss  # noqa: E402

from oracle.weights import fill_state_dict  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from cases import grad_rel_err  # noqa: E402  (the gradient metric of the step tests)
from ibot_cases import MASK_SEED, NETS, step_config  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

STEP_OPT = dict(lr=1e-3, weight_decay=1e-6, eps=1e-8)      # iBOTPL's defaults
EMA_DECAY = 0.99
CENTER_M = 0.9
TEMPERATURE = 0.1
B = 3
EXTRA_DRAWS = 4
# the step tolerances of tests/test_ibot_gpu.py (those of tests/test_dino_gpu.py)
TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6), ema=(1e-5, 1e-7), centers=1e-4)
LOSSES = ("loss", "loss_mask", "loss_global")
CENTERS = ("mask:center_sum", "mask:centers1", "global:center_sum", "global:centers1")


def step_nets():
    """The reference's classes take the reference's ADN factory: same arguments, its own module."""
    from adell_mri.modules.layers.adn_fn import get_adn_fn

    adn = get_adn_fn(1, "identity", "gelu", 0.0)
    nets = {}
    for name in NETS:
        cfg = step_config(name)
        cfg["backbone_args"]["adn_fn"] = adn
        cfg["projection_head_args"]["adn_fn"] = adn
        nets[name] = cfg
    return nets


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
    centers_mask = 0.1 * (torch.rand((cfg["out_dim"],), generator=g) * 2 - 1)
    centers_global = 0.1 * (torch.rand((cfg["out_dim"],), generator=g) * 2 - 1)
    return x1, x2, centers_mask, centers_global


def run_step(cfg, gain, x1, x2, centers, dt):
    """iBOTPL.step + AdamW + EMA in dtype ``dt`` on the real iBOT / DinoLoss."""
    net = iBOT(**copy.deepcopy(cfg))
    net.load_state_dict(fill_state_dict(net.state_dict(), gain=gain))
    net = net.to(dt).train()
    net.last_layer_.parametrizations.weight.original0.requires_grad = False
    shadow = copy.deepcopy(net).eval()
    crit = {}
    for which, c0 in zip(("mask", "global"), centers):
        crit[which] = DinoLoss((TEMPERATURE, TEMPERATURE), cfg["out_dim"], center_m=CENTER_M).to(dt)
        crit[which].centers.copy_(c0.to(dt))
    x1, x2 = x1.to(dt), x2.to(dt)
    s_red_1, s_1, mc_1 = net.forward_training(x1, mask=True)
    s_red_2, s_2, mc_2 = net.forward_training(x2, mask=True)
    with torch.no_grad():
        t_red_1, t_1 = shadow.forward_training(x1)
        t_red_2, t_2 = shadow.forward_training(x2)
    T = s_1.shape[1]
    assert int(mc_1.max()) < T and int(mc_2.max()) < T, "a drawn row reaches T: IndexError"
    crit["global"].update_centers(torch.cat([t_red_1, t_red_2]))
    crit["mask"].update_centers(torch.cat([t_1, t_2]))
    out = {"global:center_sum": crit["global"].async_batch_center.detach().clone(),
           "mask:center_sum": crit["mask"].async_batch_center.detach().clone()}
    loss_global = torch.add(crit["global"](a=s_red_1, b=t_red_2.detach()) / 2.0,
                            crit["global"](a=s_red_2, b=t_red_1.detach()) / 2.0)
    loss_mask = torch.add(crit["mask"](s_1[:, mc_1], t_1[:, mc_1].detach()) / 2.0,
                          crit["mask"](s_2[:, mc_2], t_2[:, mc_2].detach()) / 2.0)
    loss = loss_mask + loss_global
    loss.backward()
    out.update({"loss": loss.detach(), "loss_mask": loss_mask.detach(),
                "loss_global": loss_global.detach(),
                "student_red": torch.cat([s_red_1, s_red_2]).detach(),
                "student_tokens": torch.cat([s_1, s_2]).detach(),
                "teacher_red": torch.cat([t_red_1, t_red_2]).detach(),
                "teacher_tokens": torch.cat([t_1, t_2]).detach(),
                "global:centers1": crit["global"].centers.detach().reshape(-1).clone(),
                "mask:centers1": crit["mask"].centers.detach().reshape(-1).clone()})
    draws = [np.asarray(mc_1), np.asarray(mc_2)]
    width = net.mask_token_.shape[0]
    for _ in range(EXTRA_DRAWS):        # further draws of the same masker, in order
        _, more = net.patch_masker_(torch.zeros((1, T + net.extra_tokens[0], width)),
                                    mask_vector=torch.zeros(width), n_patches=net.n_patches,
                                    skip_n=net.extra_tokens)
        draws.append(np.asarray(more))
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
    return out, names, list(net.state_dict().keys()), draws, T


class _Grads(dict):
    """What tests/cases.py::grad_rel_err reads from a fixture: ``files`` and items."""

    @property
    def files(self):
        return list(self)


def within_quarter(o32, o64):
    """The reference's fp32 step against its fp64 step, at a quarter of every step tolerance."""
    q = 0.25
    worst, ok = {}, True
    for k in LOSSES:
        worst[k] = abs(float(o32[k]) - float(o64[k])) / abs(float(o64[k]))
        ok &= worst[k] <= q * TOL["loss"]
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
    for k in CENTERS:
        a, r = o32[k].double().reshape(-1), o64[k].double().reshape(-1)
        e = float(((a - r).abs() / (TOL["centers"] * r.abs())).max())
        worst[k] = e
        ok &= e <= q
    return bool(ok), worst


# ---- small per-view cases: fp32 inputs, the reference's fp64 results ----------------------------------
# name: (B, feature map, min / max patch, patches, K, class token, reduce_fn, (t1, t2), seed)
VIEW_CASES = {
    "v2d": (2, [5, 4], [1, 1], [3, 2], 2, 37, False, "mean", (0.1, 0.04), 1),
    "v3d": (2, [4, 3, 3], [1, 1, 1], [2, 2, 2], 3, 19, True, "cls", (0.1, 0.1), 2),
}
VIEW_E = 6


def gen_view_cases():
    """The real masker (draw + splice), ``iBOT.reduce`` and ``DinoLoss`` on random logits: inputs in
    fp32, results of the reference in fp64 -- what tests/ibot_ref.py is pinned to."""
    from adell_mri.utils.masking import get_masker

    out = {"view_cases": np.array(list(VIEW_CASES))}
    for name, (nb, dims, lo, hi, n_patches, K, cls, reduce_fn, (t1, t2), seed) in VIEW_CASES.items():
        g = torch.Generator().manual_seed(seed)
        c, T = int(cls), int(np.prod(dims))
        masker = get_masker("generic_transformer", image_dimensions=dims, min_patch_size=lo,
                            max_patch_size=hi, n_patches=n_patches, n_features=VIEW_E, seed=seed)
        x = torch.rand((nb, c + T, VIEW_E), generator=g) * 2 - 1
        token = torch.rand((VIEW_E,), generator=g)
        r = torch.rand((nb, c + T, VIEW_E), generator=g) * 2 - 1
        xd, td = x.double().requires_grad_(True), token.double().requires_grad_(True)
        y, m = masker(xd * 1.0, mask_vector=td, n_patches=n_patches, skip_n=(c,))
        (y * r.double()).sum().backward()
        assert int(m.max()) < T
        s = torch.rand((nb, c + T, K), generator=g) * 2 - 1
        t = torch.rand((nb, c + T, K), generator=g) * 2 - 1
        t_other = torch.rand((nb, c + T, K), generator=g) * 2 - 1
        centers = 0.2 * (torch.rand((K,), generator=g) * 2 - 1)
        w = torch.rand((nb, K), generator=g) * 2 - 1
        fake = types.SimpleNamespace(encoder_=types.SimpleNamespace(use_class_token=cls),
                                     reduce_fn=reduce_fn)
        out.update({f"{name}:conf": np.array([nb, T, K, c, n_patches], dtype=np.int64),
                    f"{name}:dims": np.array(dims), f"{name}:min": np.array(lo),
                    f"{name}:max": np.array(hi), f"{name}:reduce_fn": np.array(reduce_fn),
                    f"{name}:seed": np.int64(seed), f"{name}:t": np.array([t1, t2]),
                    f"{name}:x": x.numpy(), f"{name}:token": token.numpy(), f"{name}:r": r.numpy(),
                    f"{name}:coords": np.asarray(m).astype(np.int64),
                    f"{name}:spliced": y.detach().numpy(), f"{name}:dx": xd.grad.numpy(),
                    f"{name}:dtoken": td.grad.numpy(), f"{name}:s": s.numpy(), f"{name}:y": t.numpy(),
                    f"{name}:y_other": t_other.numpy(), f"{name}:centers": centers.numpy(),
                    f"{name}:w": w.numpy()})
        for method in ("center", "sk"):
            crit = DinoLoss((t1, t2), K, teacher_score_method=method).double()
            crit.centers.copy_(centers.double())
            sd = s.double().requires_grad_(True)
            s_red, sp = iBOT.reduce(fake, sd)
            _, tp = iBOT.reduce(fake, t.double())
            _, tp_other = iBOT.reduce(fake, t_other.double())
            loss = crit(sp[:, m], tp[:, m].detach())
            (loss + (s_red * w.double()).sum()).backward()
            out.update({f"{name}:{method}:loss": loss.detach().numpy(),
                        f"{name}:{method}:ds": sd.grad.numpy()})
            if method == "center":
                crit.update_centers(torch.cat([tp, tp_other]))
                out.update({f"{name}:s_red": s_red.detach().numpy(),
                            f"{name}:center_sum": crit.async_batch_center.reshape(-1).numpy(),
                            f"{name}:center_rows": np.int64(crit.len_teacher_output)})
            print(f"{name} {method}: rows {np.asarray(m).tolist()} of {T}, loss {float(loss.detach()):.6f}")
    return out


def gen_step():
    out = gen_view_cases()
    out.update({"B": np.int32(B), "ema_decay": np.float64(EMA_DECAY), "center_m": np.float64(CENTER_M),
           "temperature": np.float64(TEMPERATURE), "nets": np.array(list(NETS)),
           "mask_seed": np.int32(MASK_SEED)})
    for name, cfg in step_nets().items():
        found = None
        for gain in (3.0, 2.0, 1.5, 1.0, 0.7, 0.5):
            for seed in range(7, 7 + 6):
                x1, x2, c_mask, c_global = step_inputs(cfg, seed)
                o64, names, keys, draws, T = run_step(cfg, gain, x1, x2, (c_mask, c_global),
                                                      torch.float64)
                o32, _, _, draws32, _ = run_step(cfg, gain, x1, x2, (c_mask, c_global), torch.float32)
                assert all(np.array_equal(u, v) for u, v in zip(draws, draws32))
                ok, worst = within_quarter(o32, o64)
                # the outputs must differ between items, or the step pins nothing
                spread = float(o64["student_tokens"].std(0).mean())
                if ok and spread > 1e-4:
                    found = (gain, seed)
                    break
            if found:
                break
        if not found:
            raise SystemExit(f"{name}: no (gain, seed) keeps the reference's fp32 step within a "
                             f"quarter of the tolerances; last worst {worst}")
        assert ok and all(int(d.max()) < T for d in draws), [int(d.max()) for d in draws]
        out.update({f"{name}:x1": x1.numpy(), f"{name}:x2": x2.numpy(),
                    f"{name}:mask:centers0": c_mask.numpy(),
                    f"{name}:global:centers0": c_global.numpy(),
                    f"{name}:gain": np.float64(found[0]), f"{name}:seed": np.int32(found[1]),
                    f"{name}:patch_tokens": np.int32(T), f"{name}:draws": np.int32(len(draws)),
                    f"{name}:param_keys": np.array(names), f"{name}:state_keys": np.array(keys),
                    f"{name}:fp32_vs_fp64": np.array([worst[k] for k in sorted(worst)]),
                    f"{name}:fp32_vs_fp64_names": np.array(sorted(worst))})
        for i, d in enumerate(draws):
            out[f"{name}:coords{i}"] = d.astype(np.int64)
        for k, v in o64.items():
            out[f"{name}:{k}"] = v.float().numpy() if k not in LOSSES else v.numpy()
        print(f"{name}: gain {found[0]}, seed {found[1]}, losses "
              f"{[round(float(o64[k]), 6) for k in LOSSES]}, student spread {spread:.3e}, rows "
              f"{[len(d) for d in draws]} of {T}, fp32 vs fp64 (1 = the tolerance, loss / grad "
              f"relative): {worst}")
    after = {k: v for k, v in out.items() if ":step1:" in k or ":ema1:" in k}
    np.savez_compressed(os.path.join(OUT, "ibot_step.npz"),
                        **{k: v for k, v in out.items() if k not in after})
    np.savez_compressed(os.path.join(OUT, "ibot_step_params.npz"), **after)


if __name__ == "__main__":
    gen_step()
