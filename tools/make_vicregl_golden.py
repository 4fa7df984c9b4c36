#!/usr/bin/env python3
"""Fixtures of the local VICReg loss from the REAL reference (needs a checkout of the reference,
ADELL_REFERENCE; no test reads it, the tests read the fixtures):

    python tools/make_vicregl_golden.py        -> tests/golden/vicregl_loss.npz
                                                  tests/golden/ssl_resnet2d_vicregl.npz

The reference is imported through the stub recipe of SURVEY.md section 8c (empty package stubs
with the right __path__, then the leaf modules). The fixtures hold inputs, boxes, the four loss
terms, input / parameter gradients (the reference run in fp64 on the fp32 inputs) and the
multisets of selected row indices.

The loss ranks distances, so a fixture pins it only where the ranking is itself pinned. For every
case, item, kind (location / feature) and direction this script ASSERTS and records
  (a) the fp64 relative gap between the gamma-th and the (gamma + 1)-th largest distance:
      >= 1e-4 for the loss-level cases (fed by fp32 inputs, distance error at the 1e-6 level),
      >= 5e-3 for the training-step case (fed by a representation the tests pin to 1e-4);
  (b) that the reference's own fp32 selection equals its fp64 one (as multisets of rows);
and walks the seeds until both hold.
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
    ("adell_mri.modules.self_supervised", "adell_mri/modules/self_supervised"),
    ("adell_mri.modules.self_supervised.losses", "adell_mri/modules/self_supervised/losses"),
]:
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(REF, path)]
    sys.modules[name] = m
import einops.layers.torch  # noqa: E402,F401  (the reference uses it via bare `import einops`)
import torch  # noqa: E402

from adell_mri.modules.layers.adn_fn import get_adn_fn  # noqa: E402
from adell_mri.modules.layers.res_net import ResNet  # noqa: E402
from adell_mri.modules.self_supervised.losses.vicreg import VICRegLocalLoss  # noqa: E402

from oracle.weights import fill_state_dict  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SSL_GAIN = 3.0            # tests/test_ssl.py

# name: (shape of each view, gamma, first seed)
LOSS_CASES = {
    "a3d": ((2, 8, 4, 4, 4), 5, 0),
    "b2d": ((3, 16, 4, 4), 10, 101),
    "c3d": ((8, 24, 2, 3, 3), 10, 0),     # B gamma = 80 rows: beyond 64 and beyond C
}
LOSS_GAP, STEP_GAP = 1e-4, 5e-3
STEP_GAMMA = 5


def selections(loss, y1, y2, b1, b2):
    """The four rankings of one forward, as the reference makes them (its own transform_coords,
    torch.cdist and torch.topk calls on its own token grids): {tag: (sorted rows [B, gamma],
    relative gap of the gamma-th to the (gamma + 1)-th largest distance [B])}."""
    g = loss.gamma
    out = {}
    with torch.no_grad():
        c1 = loss.transform_coords(loss.get_sparse_coords(y1).to(y1.dtype), b1.to(y1.dtype))
        c2 = loss.transform_coords(loss.get_sparse_coords(y2).to(y1.dtype), b2.to(y1.dtype))
        f1 = y1.flatten(start_dim=2).swapaxes(1, 2)
        f2 = y2.flatten(start_dim=2).swapaxes(1, 2)
        for tag, a, b in (("loc12", c1, c2), ("loc21", c2, c1), ("feat12", f1, f2),
                          ("feat21", f2, f1)):
            d = torch.cdist(a, b, p=2)
            T = d.shape[-1]
            idx = torch.topk(d.flatten(start_dim=1), g, 1).indices
            rows = torch.sort(torch.div(idx, T, rounding_mode="floor"), 1).values
            v = torch.sort(d.flatten(start_dim=1), 1, descending=True).values
            gap = (v[:, g - 1] - v[:, g]) / v[:, g - 1] if v.shape[1] > g else torch.full(
                (v.shape[0],), float("inf"), dtype=v.dtype)
            out[tag] = (rows.numpy().astype(np.int32), gap.double().numpy())
    return out


def pinned(sel32, sel64, need):
    """(a) and (b) of the module docstring."""
    for tag in sel64:
        if not (sel64[tag][1] >= need).all():
            return False
        if not np.array_equal(sel32[tag][0], sel64[tag][0]):
            return False
    return True


def loss_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    B, ndim = shape[0], len(shape) - 2
    x1 = torch.randn(shape, generator=g)
    x2 = 0.5 * x1 + torch.randn(shape, generator=g)
    lo1 = 20.0 * torch.rand((B, ndim), generator=g)
    lo2 = 20.0 * torch.rand((B, ndim), generator=g)
    b1 = torch.cat([lo1, lo1 + 16.0 + 32.0 * torch.rand((B, ndim), generator=g)], 1)
    b2 = torch.cat([lo2, lo2 + 16.0 + 32.0 * torch.rand((B, ndim), generator=g)], 1)
    return x1, x2, b1, b2


def gen_loss_cases():
    out = {"cases": np.array(list(LOSS_CASES))}
    for name, (shape, gamma, seed0) in LOSS_CASES.items():
        for seed in range(seed0, seed0 + 20000):
            x1, x2, b1, b2 = loss_inputs(shape, seed)
            sel32 = selections(VICRegLocalLoss(gamma=gamma), x1, x2, b1, b2)
            sel64 = selections(VICRegLocalLoss(gamma=gamma), x1.double(), x2.double(), b1.double(),
                               b2.double())
            if pinned(sel32, sel64, LOSS_GAP):
                break
        else:
            raise SystemExit(f"{name}: no seed with a pinned ranking")
        assert pinned(sel32, sel64, LOSS_GAP)
        a = x1.double().requires_grad_(True)
        b = x2.double().requires_grad_(True)
        terms = VICRegLocalLoss(gamma=gamma)(a, b, b1.double(), b2.double())
        sum(terms).backward()
        terms32 = VICRegLocalLoss(gamma=gamma)(x1, x2, b1, b2)
        out.update({f"{name}:x1": x1.numpy(), f"{name}:x2": x2.numpy(), f"{name}:box1": b1.numpy(),
                    f"{name}:box2": b2.numpy(), f"{name}:gamma": np.int32(gamma),
                    f"{name}:seed": np.int32(seed),
                    f"{name}:terms": torch.stack(terms).detach().numpy(),
                    f"{name}:terms_fp32": torch.stack(terms32).detach().numpy(),
                    f"{name}:dx1": a.grad.float().numpy(), f"{name}:dx2": b.grad.float().numpy()})
        for tag, (rows, gap) in sel64.items():
            out[f"{name}:rows_{tag}"] = rows
            out[f"{name}:gap_{tag}"] = gap
        print(f"{name}: seed {seed}, terms {[float(t.detach()) for t in terms]}, smallest gap "
              f"{min(float(g.min()) for _, g in sel64.values()):.2e}")
    np.savez_compressed(os.path.join(OUT, "vicregl_loss.npz"), **out)


def step_net():
    """The 2-D ResNet of tests/test_ssl.py::test_resnet2d_vicreg_step_matches_reference."""
    adn = get_adn_fn(2, "batch", "swish", 0.0)
    adn1 = get_adn_fn(1, "layer", "gelu", 0.0)
    net = ResNet(dict(spatial_dim=2, in_channels=1, structure=[[8, 8, 5, 2], [16, 16, 3, 2]],
                      maxpool_structure=[[2, 2], [2, 2]], res_type="resnet", adn_fn=adn),
                 dict(in_channels=16, structure=[32, 24], adn_fn=adn1),
                 dict(in_channels=24, structure=[32, 24], adn_fn=adn1))
    net.load_state_dict(fill_state_dict(net.state_dict(), gain=SSL_GAIN))
    return net.train()


def step_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(40.0), torch.arange(48.0), indexing="ij")
    x1 = torch.stack([torch.sin((b + 1) * 0.31 * yy) * torch.cos((b + 2) * 0.17 * xx)
                      + 0.02 * (b - 1.5) * xx for b in range(4)])[:, None]
    x1 = x1 + 0.2 * torch.rand(x1.shape, generator=g)
    x2 = (x1 + 0.3 * torch.randn(x1.shape, generator=g)).flip(2)
    lo1 = 20.0 * torch.rand((4, 2), generator=g)
    lo2 = 20.0 * torch.rand((4, 2), generator=g)
    b1 = torch.cat([lo1, lo1 + 16.0 + 32.0 * torch.rand((4, 2), generator=g)], 1)
    b2 = torch.cat([lo2, lo2 + 16.0 + 32.0 * torch.rand((4, 2), generator=g)], 1)
    return x1, x2, b1, b2


def gen_step():
    for seed in range(41, 41 + 5000):
        x1, x2, b1, b2 = step_inputs(seed)
        net32, net64 = step_net(), step_net().double()
        with torch.no_grad():
            r32 = [net32(x, ret="representation") for x in (x1, x2)]
            r64 = [net64(x.double(), ret="representation") for x in (x1, x2)]
        sel32 = selections(VICRegLocalLoss(gamma=STEP_GAMMA), r32[0], r32[1], b1, b2)
        sel64 = selections(VICRegLocalLoss(gamma=STEP_GAMMA), r64[0], r64[1], b1.double(),
                           b2.double())
        if pinned(sel32, sel64, STEP_GAP):
            break
    else:
        raise SystemExit("step: no seed with a pinned ranking")
    net = step_net().double()
    y1, y2 = net(x1.double(), ret="representation"), net(x2.double(), ret="representation")
    losses = VICRegLocalLoss(gamma=STEP_GAMMA)(y1, y2, b1.double(), b2.double())
    sum(losses).backward()
    out = {"x1": x1.numpy(), "x2": x2.numpy(), "box1": b1.numpy(), "box2": b2.numpy(),
           "gamma": np.int32(STEP_GAMMA), "seed": np.int32(seed),
           "losses": torch.stack(losses).detach().numpy(),
           "representation_shape": np.array(y1.shape, dtype=np.int32)}
    keys = []
    for k, p in net.named_parameters():
        if p.grad is not None:      # the heads take no part in this loss
            out["grad:" + k] = p.grad.float().numpy().copy()
            keys.append(k)
    out["grad_keys"] = np.array(keys)
    for tag, (rows, gap) in sel64.items():
        out[f"rows_{tag}"] = rows
        out[f"gap_{tag}"] = gap
    np.savez_compressed(os.path.join(OUT, "ssl_resnet2d_vicregl.npz"), **out)
    print(f"step: seed {seed}, representation {tuple(y1.shape)}, terms "
          f"{[float(t.detach()) for t in losses]}, smallest gap "
          f"{min(float(g.min()) for _, g in sel64.values()):.2e}, {len(keys)} gradients")


if __name__ == "__main__":
    gen_loss_cases()
    gen_step()
