#!/usr/bin/env python3
"""Fixture of the ViT masked autoencoder from the REAL reference (needs a checkout of the reference,
ADELL_REFERENCE; no test reads it, the tests read the fixture):

    python tools/make_mae_golden.py       -> tests/golden/mae_step.npz

The reference is imported through the stub recipe of tools/make_ijepa_golden.py (empty package stubs
with the right __path__, then the leaf modules; ``conv_next``, which the autoencoder module imports
for the ConvNeXt autoencoder that is not mirrored, is a stub with a placeholder class): its
``ViTMaskedAutoEncoder`` and ``random_masking`` are the real ones. Lightning is not installed, so the
arithmetic of ``ViTMaskedAutoEncoderPL`` is restated here: ``MSELoss()(model(x)[0], x)``, one step of
AdamW with betas (0.9, 0.95), lr 1e-3, weight decay 1e-6 over ``parameters()``, then a validation
step, which draws the second shuffle of the model's one rng.

Both steps run in ``eval()`` mode. The two ``TransformerBlockStack``s are built from four keys of
``encoder_args`` / ``decoder_args`` only, so their MLPs carry the stack's default ``adn_fn``, whose
dropout is 0.1 and cannot be configured away: in ``train()`` mode the reference's step is random.
``eval()`` turns exactly that dropout off and changes nothing else (there is no batch norm).

Two networks (tests/mae_cases.py), batch 3. For each this script ASSERTS that numpy's stable argsort
of the noise the rng draws (re-drawn here from the same seed) equals the ids the reference's
``torch.argsort`` made, for both draws, and that the reference's own fp32 step stays within a quarter
of the step tolerances of tests/test_mae_gpu.py against its fp64 step, walking the fill gain and the
input seed until that holds; the ratios are recorded.

Besides the steps the file holds small cases to which tests/mae_ref.py is pinned (``r*``): the real
``ViTMaskedAutoEncoder.forward`` with the embedding replaced by a stub that hands in given tokens,
the encoder and the head by identities and the decoder by a recorder -- what remains is
``random_masking``, the un-shuffle, the view / permute and, here, ``MSELoss``; fp32 inputs, fp64
results and gradients.
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
]:
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(REF, path)]
    sys.modules[name] = m
# only ConvNeXtAutoEncoder, which is not mirrored, uses it
stub = types.ModuleType("adell_mri.modules.layers.conv_next")
stub.ConvNeXtV2Backbone = type("ConvNeXtV2Backbone", (), {})
sys.modules["adell_mri.modules.layers.conv_next"] = stub
import einops.layers.torch  # noqa: E402,F401  (the reference uses it via bare `import einops`)
import torch  # noqa: E402

from adell_mri.modules.self_supervised.autoencoders import ViTMaskedAutoEncoder  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from cases import grad_rel_err  # noqa: E402  (the gradient metric of the step tests)
from mae_cases import B, CONFIGS, NETS, fill, step_config  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

STEP_OPT = dict(lr=1e-3, weight_decay=1e-6, betas=(0.9, 0.95), eps=1e-8)   # the wrapper's defaults
SEED = 42               # ViTMaskedAutoEncoder's default: the wrapper does not pass one
# the step tolerances of tests/test_mae_gpu.py (those of tools/make_ijepa_golden.py)
TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6))
LOSSES = ("loss", "val_loss")


def step_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (B, cfg["in_channels"], *cfg["image_size"])
    grids = torch.meshgrid(*[torch.arange(float(s)) for s in cfg["image_size"]], indexing="ij")
    x = torch.stack([torch.stack([torch.sin((b + 1) * 0.37 * grids[0] + c) *
                                  torch.cos((b + 2) * 0.23 * grids[1]) for c in range(shape[1])])
                     for b in range(B)])
    return x + 0.2 * torch.rand(shape, generator=g)


def recording(rng):
    """The noise ``rng.uniform`` hands out, in order."""
    drawn, inner = [], rng.uniform

    class _Rng:
        def uniform(self, *args, **kwargs):
            out = inner(*args, **kwargs)
            drawn.append(out.copy())
            return out

    return _Rng(), drawn


def argsort_ids(noise, mask_fraction):
    """numpy's side of the assertion: stable argsorts of the recorded noise."""
    ids_shuffle = np.argsort(noise, axis=1, kind="stable")
    ids_restore = np.argsort(ids_shuffle, axis=1, kind="stable")
    L = noise.shape[1]
    mask = (ids_restore >= int(L * (1 - mask_fraction))).astype(np.float32)
    return ids_shuffle, ids_restore, mask


def run_step(cfg, gain, x, dt):
    """The wrapper's training step + AdamW, then a validation step, in dtype ``dt`` on the real
    ViTMaskedAutoEncoder."""
    net = ViTMaskedAutoEncoder(**copy.deepcopy(cfg))
    assert net.seed == SEED
    keys = list(net.state_dict().keys())
    names = [k for k, _ in net.named_parameters()]
    net.load_state_dict(fill(net.state_dict(), gain))
    assert net.positional_embedding is net.proj.positional_embedding
    net = net.to(dt).eval()         # dropout off (module docstring); gradients flow all the same
    net.rng, drawn = recording(net.rng)
    x = x.to(dt)
    crit = torch.nn.MSELoss()
    # the token predictions, before the view / permute
    seen = {}
    hook = net.decoder_pred.register_forward_hook(lambda m, i, o: seen.__setitem__("pred", o.detach()))
    recon, mask = net(x)
    hook.remove()
    loss = crit(recon, x)
    loss.backward()
    out = {"loss": loss.detach(), "pred": seen["pred"], "recon": recon.detach(),
           "mask0": mask.detach()}
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        out["grad:" + k] = p.grad.clone()
    torch.optim.AdamW(net.parameters(), **STEP_OPT).step()
    with torch.no_grad():
        for k, p in net.named_parameters():
            out["step1:" + k] = p.detach().clone()
        recon, mask = net(x)
        out["val_loss"] = crit(recon, x).detach()
        out["mask1"] = mask.detach()
    assert len(drawn) == 2 and drawn[0].dtype == np.float64
    # what torch.argsort made of the noise: ids_restore is the forward's own, through the mask
    for i, noise in enumerate(drawn):
        ids_shuffle, ids_restore, mask_np = argsort_ids(noise, cfg["mask_fraction"])
        t_shuffle = torch.argsort(torch.as_tensor(noise), dim=1, stable=True)
        t_restore = torch.argsort(t_shuffle, dim=1, stable=True)
        assert np.array_equal(ids_shuffle, t_shuffle.numpy()), "numpy and torch argsort differ"
        assert np.array_equal(ids_restore, t_restore.numpy())
        assert np.array_equal(mask_np, out[f"mask{i}"].float().numpy()), "mask differs"
        out[f"ids_shuffle{i}"] = torch.as_tensor(ids_shuffle)
        out[f"noise{i}"] = torch.as_tensor(noise)
    return out, names, keys


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
    worst["grad"] = worst["param"] = 0.0
    grads = _Grads({k: v.numpy() for k, v in o64.items() if k.startswith("grad:")})
    for k in o64:
        a, r = o32[k].double(), o64[k].double()
        if k.startswith("grad:"):
            e = grad_rel_err(grads, k[5:], o32[k].double().numpy())
            worst["grad"] = max(worst["grad"], e)
            ok &= e <= q * TOL["grad"]
        elif k.startswith("step1:"):
            rt, at = TOL["param"]
            e = float(((a - r).abs() / (at + rt * r.abs())).max())     # <= 1 passes assert_allclose
            worst["param"] = max(worst["param"], e)
            ok &= e <= q
    return bool(ok), worst


# ---- small cases: fp32 inputs, the reference's fp64 results ------------------------------------------
# name: (B, image_size, patch_size, C, mask_fraction, seed)
SMALL_CASES = {"r1": (1, [1, 2], [1, 1], 1, 0.5, 1), "r2": (3, [4, 6], [2, 2], 2, 0.6, 2),
               "r3": (2, [4, 6], [2, 3], 3, 0.0, 3)}


class _Given(torch.nn.Module):
    def __init__(self, tokens):
        super().__init__()
        self.tokens = tokens

    def forward(self, x):
        return self.tokens


class _Recorder(torch.nn.Module):
    def forward(self, x):
        self.seen = x
        x.retain_grad()
        return x


def gen_small_cases():
    out = {"small_cases": np.array(list(SMALL_CASES))}
    for name, (nb, image, patch, C, fraction, seed) in SMALL_CASES.items():
        g = torch.Generator().manual_seed(seed)
        L = (image[0] // patch[0]) * (image[1] // patch[1])
        E = patch[0] * patch[1] * C
        stack = dict(number_of_blocks=1, hidden_dim=E, n_heads=1, mlp_structure=[E])
        net = ViTMaskedAutoEncoder(image, patch, C, 96, stack, stack, mask_fraction=fraction,
                                   seed=seed).double()
        e = torch.rand((nb, L, E), generator=g) * 2 - 1
        r = torch.rand((nb, L, E), generator=g) * 2 - 1
        x = torch.rand((nb, C, *image), generator=g) * 2 - 1
        pos = torch.rand((1, L, E), generator=g)
        mask_token = torch.rand((1, 1, E), generator=g) - 0.5
        scale = torch.tensor([0.75])
        ed = e.double().requires_grad_(True)
        net.proj = _Given(ed)
        net.encoder, net.decoder_pred, net.decoder = torch.nn.Identity(), torch.nn.Identity(), _Recorder()
        net.positional_embedding = torch.nn.Parameter(pos.double())
        with torch.no_grad():
            net.mask_token.copy_(mask_token.double())
            net.mask_token_scale.copy_(scale.double())
        noise = np.random.default_rng(seed).uniform(size=[nb, L])
        ids_shuffle, _, mask_np = argsort_ids(noise, fraction)
        recon, mask = net(x.double())
        assert np.array_equal(mask.float().numpy(), mask_np)
        restored = net.decoder.seen
        K = int(L * (1 - fraction))
        assert int((mask_np == 0).sum()) == nb * K
        leaves = (ed, net.positional_embedding, net.mask_token, net.mask_token_scale)
        grads = torch.autograd.grad((restored * r.double()).sum(), leaves, retain_graph=True,
                                    allow_unused=True)
        grads = [torch.zeros_like(p) if d is None else d for d, p in zip(grads, leaves)]
        loss = torch.nn.MSELoss()(recon, x.double())
        dpred, = torch.autograd.grad(loss, restored)
        out.update({f"{name}:ids_shuffle": ids_shuffle.astype(np.int64), f"{name}:K": np.int32(K),
                    f"{name}:image_shape": np.array(x.shape), f"{name}:patch": np.array(patch),
                    f"{name}:mask": mask_np, f"{name}:e": e.numpy(), f"{name}:r": r.numpy(),
                    f"{name}:x": x.numpy(), f"{name}:pos": pos.numpy(),
                    f"{name}:mask_token": mask_token.numpy(), f"{name}:scale": scale.numpy(),
                    f"{name}:out": restored.detach().numpy(), f"{name}:recon": recon.detach().numpy(),
                    f"{name}:de": grads[0].numpy(), f"{name}:dpos": grads[1].numpy(),
                    f"{name}:dmask_token": grads[2].numpy(), f"{name}:dscale": grads[3].numpy(),
                    f"{name}:loss": loss.detach().numpy(), f"{name}:dpred": dpred.numpy()})
    return out


def gen_step():
    out = gen_small_cases()
    out.update({"B": np.int32(B), "nets": np.array(list(NETS)), "seed": np.int32(SEED)})
    for name in NETS:
        cfg = step_config(name)
        _, L, E, K = CONFIGS[name]
        found = None
        for gain in (3.0, 2.0, 1.5, 1.0, 0.7, 0.5):
            for seed in range(7, 7 + 6):
                x = step_inputs(cfg, seed)
                o64, names, keys = run_step(cfg, gain, x, torch.float64)
                o32, _, _ = run_step(cfg, gain, x, torch.float32)
                for i in range(2):
                    assert torch.equal(o64[f"ids_shuffle{i}"], o32[f"ids_shuffle{i}"])
                ok, worst = within_quarter(o32, o64)
                # the predictions must differ between items, or the step pins nothing
                spread = float(o64["pred"].std(0).mean())
                if ok and spread > 1e-4:
                    found = (gain, seed)
                    break
            if found:
                break
        if not found:
            raise SystemExit(f"{name}: no (gain, seed) keeps the reference's fp32 step within a "
                             f"quarter of the tolerances; last worst {worst}")
        assert tuple(o64["pred"].shape) == (B, L, E) and o64["ids_shuffle0"].shape == (B, L)
        assert int((o64["mask0"] == 0).sum()) == B * K
        assert "positional_embedding" in keys and "proj.positional_embedding" in keys
        assert names[:3] == ["positional_embedding", "mask_token_scale", "mask_token"]
        assert "proj.positional_embedding" not in names
        out.update({f"{name}:x": x.numpy(), f"{name}:gain": np.float64(found[0]),
                    f"{name}:seed": np.int32(found[1]),
                    f"{name}:param_keys": np.array(names), f"{name}:state_keys": np.array(keys),
                    f"{name}:fp32_vs_fp64": np.array([worst[k] for k in sorted(worst)]),
                    f"{name}:fp32_vs_fp64_names": np.array(sorted(worst))})
        for k, v in o64.items():
            if k in LOSSES or k.startswith("noise"):
                out[f"{name}:{k}"] = v.numpy()
            elif k.startswith("ids_shuffle"):
                out[f"{name}:{k}"] = v.numpy().astype(np.int64)
            else:
                out[f"{name}:{k}"] = v.float().numpy()
        print(f"{name}: gain {found[0]}, seed {found[1]}, losses "
              f"{[round(float(o64[k]), 6) for k in LOSSES]}, prediction spread {spread:.3e}, "
              f"fp32 vs fp64 (1 = the tolerance; loss / grad relative): {worst}")
    path = os.path.join(OUT, "mae_step.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    gen_step()
