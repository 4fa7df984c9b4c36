#!/usr/bin/env python3
"""Fixtures of spectral normalisation from the REAL reference (needs a checkout of the reference,
ADELL_REFERENCE; no test reads it, the tests read the fixture):

    python tools/make_spectral_norm_golden.py   -> tests/golden/spectral_norm.npz (kernel-level cases),
                                                   tests/golden/spectral_norm_unet.npz, _cat.npz

The reference is imported through the stub recipe of tools/make_classification_golden.py (empty
package stubs with the right __path__, then the leaf modules); ``lightning`` is stubbed (the callback
only subclasses ``pl.Callback``), as are ``adell_mri.utils.utils`` (it imports MONAI and SimpleITK; the
two names the leaves take from it are never called here) and ``tqdm``. ``SpectralNorm``,
``reshape_weight_to_matrix``, ``calculate_sn_weights``, ``UNet``, ``CatNet`` and the focal loss are
the real ones, and so is torch's ``_SpectralNorm``.

Kernel-level cases (tests/spectral_norm_cases.py: shapes, dim, inputs from a seed), in fp64 with ``u``
and ``v`` rounded to fp32 where torch stores them: n power iterations, sigma = u^T W v, W_sn = W /
sigma on the reference's ``reshape_weight_to_matrix`` matrix, and dW by torch's autograd for the given
G; train mode for n in (1, 3) and eval mode. sigma is kept, and of ``u``, ``v``, W_sn and dW every
``sample_stride``-th element (arrays of up to 1024 elements whole). ERROR YARDSTICK per case and mode: torch's own fp32 CPU
``_SpectralNorm`` (buffers set to the same u0, v0) against those values -- forward and backward as
fractions of the largest magnitude, u and v absolute.

Applied networks: the callback on a small 3-D ``UNet`` (instance norm, transposed-conv upscaling,
depths 4 / 16 / 32) and on the ``cat2`` ``CatNet`` of tests/classification_cases.py: the parametrised
parameter names, the whole initial ``state_dict``, two training steps (loss and ``state_dict`` after
each) and one validation step with every dropout at 0, in fp64 and in fp32; the fp64 records are
kept (as fp32 arrays, losses as fp64) and the fp32-against-fp64 errors are the yardstick of the step
tests. Then the ``bake_on_save`` checkpoint keys and ``calculate_sn_weights`` of the final state (for
the transposed conv, whose ``_u`` has ``size(1)`` entries, the reference's function fails: its value
is restated with the reference's ``reshape_weight_to_matrix(w, 1)``).
"""
import copy
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


def _stub(name, **names):
    mod = types.ModuleType(name)
    mod.__dict__.update(names)
    sys.modules[name] = mod
    return mod


_Callback = type("Callback", (), {})
_stub("lightning")
_stub("lightning.pytorch", Callback=_Callback, LightningModule=object, Trainer=object)
_stub("lightning.pytorch.callbacks", Callback=_Callback)
_stub("lightning.pytorch.callbacks.model_checkpoint", ModelCheckpoint=_Callback)
sys.modules["lightning"].pytorch = sys.modules["lightning.pytorch"]
_stub("adell_mri.utils.utils", ExponentialMovingAverage=object, return_classes=None)
try:
    import tqdm  # noqa: F401
except ImportError:
    _stub("tqdm", tqdm=lambda it, *a, **k: it)
import einops.layers.torch  # noqa: E402,F401
import torch  # noqa: E402
from torch.nn.utils.parametrizations import _SpectralNorm  # noqa: E402

from adell_mri.modules.activations import activation_factory  # noqa: E402
from adell_mri.modules.classification.classification import classification as RC  # noqa: E402
from adell_mri.modules.layers.adn_fn import get_adn_fn  # noqa: E402
from adell_mri.modules.segmentation.losses import binary_focal_loss  # noqa: E402
from adell_mri.modules.segmentation.unet import UNet  # noqa: E402
from adell_mri.utils.pl_callbacks import SpectralNorm, reshape_weight_to_matrix  # noqa: E402
from adell_mri.utils.torch_utils import calculate_sn_weights  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import classification_cases as CC  # noqa: E402
import spectral_norm_cases as C  # noqa: E402

OUT = C.GOLD


def rel(a, r):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    if not np.isfinite(r).all():
        return 0.0
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-300))


# ---- kernel-level cases ------------------------------------------------------------------------------------
def kernel_fp64(W, u0, v0, G, n, dim, training):
    W = torch.from_numpy(W).double().requires_grad_(True)
    u, v = torch.from_numpy(u0).clone(), torch.from_numpy(v0).clone()
    mat = reshape_weight_to_matrix(W, dim)
    if training:
        with torch.no_grad():
            for _ in range(n):
                a = torch.mv(mat, v.double())
                u = (a / max(float(a.norm()), C.EPS)).float()
                b = torch.mv(mat.t(), u.double())
                v = (b / max(float(b.norm()), C.EPS)).float()
    sigma = torch.dot(u.double(), torch.mv(mat, v.double()))
    out = W / sigma
    out.backward(torch.from_numpy(G).double())
    return out.detach().numpy(), u.numpy(), v.numpy(), float(sigma.detach()), W.grad.numpy()


def kernel_fp32(W, u0, v0, G, n, dim, training):
    W = torch.from_numpy(W).clone().requires_grad_(True)
    sn = _SpectralNorm(W.detach(), n, dim, C.EPS)
    with torch.no_grad():
        sn._u.copy_(torch.from_numpy(u0))
        sn._v.copy_(torch.from_numpy(v0))
    sn.train(training)
    out = sn(W)
    out.backward(torch.from_numpy(G))
    return out.detach().numpy(), sn._u.numpy().copy(), sn._v.numpy().copy(), W.grad.numpy()


def gen_kernels(out):
    worst = {"fwd": 0.0, "bwd": 0.0, "uv": 0.0}
    for name, (shape, dim) in C.KERNEL_CASES.items():
        W, u0, v0, G = C.kernel_inputs(name)
        st = C.sample_stride(W.size)
        for mode, n in C.MODES:
            training = mode == "train"
            key = f"k:{name}:{mode}{n}:"
            o, u, v, sigma, dW = kernel_fp64(W, u0, v0, G, n, dim, training)
            o32, u32, v32, dW32 = kernel_fp32(W, u0, v0, G, n, dim, training)
            err = [rel(o32, o), rel(dW32, dW),
                   max(float(np.abs(u32.astype(np.float64) - u).max()),
                       float(np.abs(v32.astype(np.float64) - v).max()))]
            for k, e in zip(("fwd", "bwd", "uv"), err):
                worst[k] = max(worst[k], e)
            out[key + "w_sn"] = o.reshape(-1)[::st]
            out[key + "dw"] = dW.reshape(-1)[::st]
            out[key + "u"], out[key + "v"] = u[::C.sample_stride(u.size)], v[::C.sample_stride(v.size)]
            out[key + "sigma"] = np.float64(sigma)
            out[key + "yardstick"] = np.array(err, dtype=np.float64)     # fwd, bwd, u / v
            print(f"{name:18s} {mode}{n}: sigma {sigma:.6f}, torch fp32 vs fp64: fwd {err[0]:.2e} bwd "
                  f"{err[1]:.2e} u/v {err[2]:.2e}")
    print("largest yardsticks:", worst)


# ---- applied networks ---------------------------------------------------------------------------------------
def build_unet():
    net = UNet(activation_fn=activation_factory["swish"], **copy.deepcopy(C.UNET_KW))
    net.load_state_dict(CC.fill(net.state_dict(), C.UNET_GAIN))
    x, y = C.unet_batch()

    def loss_of(net, dt):
        pred = net(torch.from_numpy(x).to(dt))[0]
        return binary_focal_loss(pred, torch.from_numpy(y).to(dt), **C.FOCAL).mean()

    def optimizer(net):
        return torch.optim.SGD(net.parameters(), lr=C.UNET_LR, momentum=0.99, nesterov=True,
                               weight_decay=C.UNET_WD)
    return net, loss_of, optimizer


def build_cat():
    kw = CC.net_kwargs(C.CAT_NAME)
    net = RC.CatNet(adn_fn=get_adn_fn(3, "batch", "swish", 0.0), **kw)
    CC.zero_dropout(net)
    net.load_state_dict(CC.fill(net.state_dict(), C.CAT_GAIN))
    x = C.cat_input()
    y = torch.tensor(CC.CONFIGS[C.CAT_NAME][3])

    def loss_of(net, dt):
        pred = torch.squeeze(net(torch.from_numpy(x).to(dt)), 1)
        return torch.nn.BCEWithLogitsLoss()(pred, y.to(dt)).mean()

    def optimizer(net):
        named = list(net.named_parameters())
        groups, base_wd = CC.step_groups(named, CC.CONFIGS[C.CAT_NAME][5])
        by_name = dict(named)
        return torch.optim.AdamW([{"params": [by_name[n] for n in names], "weight_decay": wd}
                                  for names, wd in groups], lr=CC.STEP_LR, weight_decay=base_wd,
                                 eps=CC.STEP_EPS)
    return net, loss_of, optimizer


def run_network(build, dt, init=None):
    torch.manual_seed(5)
    net, loss_of, optimizer = build()
    plain = [k for k, _ in net.named_parameters()]
    SpectralNorm(n_power_iterations=1).setup(None, net, "fit")
    names = [k[:-len(".original")].replace("parametrizations.", "")
             for k, _ in net.named_parameters() if k.endswith(".original")]
    if init is not None:
        net.load_state_dict(init, strict=True)
    net = net.to(dt).train()
    rec = {"init": {k: v.detach().clone() for k, v in net.state_dict().items()}}
    opt = optimizer(net)
    for s in range(C.N_STEPS):
        opt.zero_grad()
        loss = loss_of(net, dt)
        loss.backward()
        opt.step()
        rec[f"loss{s + 1}"] = float(loss.detach())
        rec[f"step{s + 1}"] = {k: v.detach().clone() for k, v in net.state_dict().items()}
    net.eval()
    with torch.no_grad():
        rec["val"] = float(loss_of(net, dt))
    return net, rec, names, plain


def gen_network(tag, build):
    out = {}
    net32, rec32, names, plain = run_network(build, torch.float32)
    init = rec32["init"]
    net64, rec64, _, _ = run_network(build, torch.float64, init={k: v.double() if v.is_floating_point()
                                                                  else v for k, v in init.items()})
    out["names"] = np.array(names)
    out["plain_keys"] = np.array(plain)
    out["state_keys"] = np.array(list(init.keys()))
    # a module registered under two names (CatNet's ``feature_extraction`` / ``res_net``) has every
    # entry twice: the records keep the first key of each tensor
    first, seen = [], set()
    for k, v in net64.state_dict().items():
        if v.data_ptr() not in seen or v.numel() == 0:
            first.append(k)
        seen.add(v.data_ptr())
    out["record_keys"] = np.array(first)
    # the initial state: the weights are the fill of tests/spectral_norm_cases.py; the vectors are draws
    for k, v in init.items():
        if k.endswith(("._u", "._v")):
            out[f"init:{k}"] = v.numpy()
    yard = {"loss": 0.0, "param": 0.0, "uv": 0.0}
    for s in ("step1", "step2"):
        for k in first:
            v = rec64[s][k]
            out[f"{s}:{k}"] = (v.float() if v.is_floating_point() else v).numpy()
            if not v.is_floating_point():
                continue
            a = rec32[s][k].double().numpy()
            if k.endswith(("._u", "._v")):
                yard["uv"] = max(yard["uv"], float(np.abs(a - v.numpy()).max()))
            elif k.endswith(".original"):
                yard["param"] = max(yard["param"], rel(a, v.numpy()))
    for k in ("loss1", "loss2", "val"):
        out[k] = np.float64(rec64[k])
        yard["loss"] = max(yard["loss"], abs(rec32[k] - rec64[k]) / abs(rec64[k]))
    out["yardstick"] = np.array([yard["loss"], yard["param"], yard["uv"]])      # loss, original, u / v
    print(f"{tag}: {len(names)} parametrised, losses {rec64['loss1']:.6f} {rec64['loss2']:.6f} val "
          f"{rec64['val']:.6f}; reference fp32 vs fp64 {yard}")
    # the bake_on_save checkpoint and calculate_sn_weights of the final state (fp64 network)
    final = {k: v.detach().clone() for k, v in net64.state_dict().items()}
    ckpt = {"state_dict": dict(final)}
    net64.eval()      # the bake reads module.weight: no further power iteration
    SpectralNorm(bake_on_save=True).on_save_checkpoint(None, net64, ckpt)
    out["baked_keys"] = np.array(list(ckpt["state_dict"].keys()))
    sn = {}
    for k in list(final):
        if not k.endswith(".original"):
            continue
        stem = k[:-len(".original")]
        one = {kk: final[kk].clone() for kk in (k, stem + ".0._u", stem + ".0._v")}
        w, u = one[k], one[stem + ".0._u"]
        if w.size(0) == u.numel():
            sn.update(calculate_sn_weights(one))
        else:       # a transposed conv: the reference's view fails; its value on the dim = 1 matrix
            mat = reshape_weight_to_matrix(w, 1)
            sn[stem.replace(".parametrizations", "")] = w / torch.dot(u, torch.mv(mat, one[stem + ".0._v"]))
    out["sn_keys"] = np.array(list(sn.keys()))
    for k, v in sn.items():
        if stem_recorded(k, first):
            out[f"sn:{k}"] = v.float().numpy().reshape(-1)[::C.sample_stride(v.numel())]
        # (baked under the first name only: ``named_modules`` yields a module once)
        assert k not in ckpt["state_dict"] or torch.allclose(v, ckpt["state_dict"][k]), k
    path = C.NET_GOLD[tag]
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


def stem_recorded(key, first):
    """Whether the parametrised weight ``key`` is recorded under this name (not an alias)."""
    mod, _, name = key.rpartition(".")
    return f"{mod}.parametrizations.{name}.original" in first


def main():
    out = {}
    gen_kernels(out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")
    assert os.path.getsize(OUT) < (1 << 20)
    gen_network("unet", build_unet)
    gen_network("cat", build_cat)


if __name__ == "__main__":
    main()
