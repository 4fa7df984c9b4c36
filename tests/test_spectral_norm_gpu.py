"""Spectral normalisation on the device: the fused kernels of every route against the fp64
restatement (tests/spectral_norm_ref.py), bounded by four times the error of torch's own fp32
``_SpectralNorm`` recorded for the same case (tools/make_spectral_norm_golden.py), and two training
steps plus a validation step of the parametrised networks against the reference's records, bounded by
four times the reference's own fp32-against-fp64 error."""
import functools

import numpy as np
import pytest
import torch

import spectral_norm_cases as C
import spectral_norm_nets as N
import spectral_norm_ref as R
from adell_mri_amd import functional as HF
from adell_mri_amd.modules.layers.spectral_norm import _SpectralNorm

pytestmark = pytest.mark.gpu
KERNEL_PARAMS = [(name, mode, n) for name in C.KERNEL_CASES for mode, n in C.MODES]


@functools.lru_cache(maxsize=None)
def gold():
    return np.load(C.GOLD, allow_pickle=False)


@functools.lru_cache(maxsize=None)
def reference(name, mode, n):
    """(W_sn, u, v, sigma, dW) of the restatement, computed once per case and left unchanged."""
    shape, dim = C.KERNEL_CASES[name]
    W, u0, v0, G = C.kernel_inputs(name)
    w_sn, u, v, sigma = R.forward(W, u0, v0, n, C.EPS, dim, mode == "train")
    return w_sn, u, v, sigma, R.backward(G, w_sn, u, v, sigma, dim)


def relmax(a, r):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return float(np.abs(a - r).max() / np.abs(r).max())


def run_case(name, mode, n, cuda):
    shape, dim = C.KERNEL_CASES[name]
    W, u0, v0, G = (torch.from_numpy(a).to(cuda) for a in C.kernel_inputs(name))
    W.requires_grad_(True)
    out = HF.spectral_normalize(W, u0, v0, n, C.EPS, dim, mode == "train")
    out.backward(G)
    return out.detach(), u0, v0, W.grad


@pytest.mark.parametrize("name,mode,n", KERNEL_PARAMS)
def test_kernels_match_the_restatement(cuda, name, mode, n):
    w_sn, u, v, sigma, dw = reference(name, mode, n)
    yard = gold()[f"k:{name}:{mode}{n}:yardstick"]          # torch fp32 against fp64: fwd, bwd, u / v
    out, gu, gv, gw = run_case(name, mode, n, cuda)
    e_fwd, e_bwd = relmax(out.cpu().numpy(), w_sn), relmax(gw.cpu().numpy(), dw)
    e_uv = max(float(np.abs(gu.cpu().numpy().astype(np.float64) - u).max()),
               float(np.abs(gv.cpu().numpy().astype(np.float64) - v).max()))
    print(f"{name} {mode}{n} [{C.ROUTES[name]}]: fwd {e_fwd:.2e} (yardstick {yard[0]:.2e}) bwd "
          f"{e_bwd:.2e} ({yard[1]:.2e}) u/v {e_uv:.2e} ({yard[2]:.2e})")
    assert e_fwd <= 4 * yard[0]
    assert e_bwd <= 4 * yard[1]
    assert e_uv <= 4 * yard[2]


@pytest.mark.parametrize("name", ["odd", "convt", "lin", "grid_low_d1"])
def test_buffers_in_place_eval_unchanged_and_bit_reproducible(cuda, name):
    shape, dim = C.KERNEL_CASES[name]
    W, u0, v0, _ = (torch.from_numpy(a).to(cuda) for a in C.kernel_inputs(name))
    u, v = u0.clone(), v0.clone()
    pu, pv = u.data_ptr(), v.data_ptr()
    a = HF.spectral_normalize(W, u, v, 1, C.EPS, dim, True)
    assert (u.data_ptr(), v.data_ptr()) == (pu, pv)
    assert not torch.equal(u, u0) and not torch.equal(v, v0)
    u2, v2 = u0.clone(), v0.clone()
    b = HF.spectral_normalize(W, u2, v2, 1, C.EPS, dim, True)
    assert torch.equal(a, b) and torch.equal(u, u2) and torch.equal(v, v2)       # bit-equal runs
    ue, ve = u.clone(), v.clone()
    HF.spectral_normalize(W, ue, ve, 1, C.EPS, dim, False)
    assert torch.equal(ue, u) and torch.equal(ve, v)                             # eval: only read


@pytest.mark.parametrize("shape,dim", [((8, 4, 3, 3, 3), 0), ((130, 300), 0), ((16, 8, 2, 2, 2), 1)])
def test_zero_weight_gives_nan_and_no_error(cuda, shape, dim):
    outer, h, inner = C.matrix_dims(shape, dim)
    W = torch.zeros(shape, device=cuda, requires_grad=True)
    u = torch.full((h,), h ** -0.5, device=cuda)
    v = torch.full((outer * inner,), (outer * inner) ** -0.5, device=cuda)
    out = HF.spectral_normalize(W, u, v, 1, C.EPS, dim, True)
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(W.grad).all()
    assert torch.equal(u, torch.zeros_like(u)) and torch.equal(v, torch.zeros_like(v))   # as torch


@pytest.mark.parametrize("name", ["odd", "lin"])
def test_two_accesses_then_backward_use_each_access_own_vectors(cuda, name):
    """loss = <G, W_sn(first access)> - <G, W_sn(second access)>: the second access advances the
    buffers, the first gradient still uses the first access's u, v."""
    shape, dim = C.KERNEL_CASES[name]
    W0, u0, v0, G = C.kernel_inputs(name)
    a1, u1, v1, s1 = R.forward(W0, u0, v0, 1, C.EPS, dim, True)
    a2, u2, v2, s2 = R.forward(W0, u1, v1, 1, C.EPS, dim, True)
    want = R.backward(G, a1, u1, v1, s1, dim) - R.backward(G, a2, u2, v2, s2, dim)
    W, u, v, Gd = (torch.from_numpy(a).to(cuda) for a in (W0, u0, v0, G))
    W.requires_grad_(True)
    first = HF.spectral_normalize(W, u, v, 1, C.EPS, dim, True)
    second = HF.spectral_normalize(W, u, v, 1, C.EPS, dim, True)
    ((first * Gd).sum() - (second * Gd).sum()).backward()
    yard = gold()[f"k:{name}:train1:yardstick"]
    scale = max(np.abs(R.backward(G, a1, u1, v1, s1, dim)).max(), np.abs(want).max())
    err = float(np.abs(W.grad.cpu().numpy() - want).max() / scale)
    print(f"{name}: two accesses, gradient error {err:.2e} of the largest single gradient")
    assert err <= 2 * 4 * yard[1]        # two gradients, each within its bound
    assert np.abs(u.cpu().numpy().astype(np.float64) - u2).max() <= 4 * yard[2]


def test_module_forward_runs_the_fused_route_on_the_device(cuda):
    w = torch.randn(8, 4, 3, 3, 3, device=cuda)
    sn = _SpectralNorm(w, 1, 0, 1e-12).to(cuda)
    assert sn.route(w) == "block" and sn.route(w.double()) == "composed"
    u0 = sn._u.clone()
    out = sn(w)
    assert getattr(out, "_adell_transient", False) and not torch.equal(sn._u, u0)
    ref = torch.nn.utils.parametrizations._SpectralNorm(w, 1, 0, 1e-12).to(cuda)
    ref.load_state_dict(sn.state_dict())
    torch.testing.assert_close(sn.eval()(w), ref.eval()(w), rtol=1e-5, atol=1e-6)


def _run_steps(tag, cuda, steps):
    from adell_mri_amd.trainer import StepRunner

    g = N.net_gold(tag)
    net = N.build(tag).to(cuda).train()
    runner = StepRunner(net, spectral_norm=1)
    net.load_state_dict(N.initial_state(net, g, tag), strict=True)
    batch = N.batch(tag, cuda)
    for _ in range(steps):
        runner.train_step(batch)        # (the loss is not kept: nothing of a step outlives it)
    return g, net, runner, batch


@pytest.mark.parametrize("tag", ["unet", "cat"])
def test_step_parity_with_the_reference(cuda, tag):
    """Two ``StepRunner(spectral_norm=1)`` steps and one ``validate_steps`` from the golden state
    against the reference's fp64 records; bounds: four times the reference's own fp32-against-fp64
    error (loss relative, ``original`` as a fraction of its largest magnitude, ``_u`` / ``_v``
    absolute). A second evaluation of a parametrization per forward would show in ``_u`` / ``_v``."""
    from adell_mri_amd.trainer import validate_steps

    g, net, runner, batch = _run_steps(tag, cuda, 0)
    yard = g["yardstick"]
    worst = {"loss": 0.0, "param": 0.0, "uv": 0.0}
    failures = []
    for s in range(C.N_STEPS):
        loss = float(runner.train_step(batch).detach())
        e = abs(loss - float(g[f"loss{s + 1}"])) / abs(float(g[f"loss{s + 1}"]))
        worst["loss"] = max(worst["loss"], e)
        sd = net.state_dict()
        for k in g["record_keys"]:
            k = str(k)
            got = sd[N.PREFIX[tag] + k]
            if not got.is_floating_point():
                continue
            got, want = got.double().cpu().numpy(), g[f"step{s + 1}:{k}"].astype(np.float64)
            if k.endswith(("._u", "._v")):
                e, kind = float(np.abs(got - want).max()), "uv"
            elif k.endswith(".original"):
                e, kind = relmax(got, want), "param"
            else:
                continue
            worst[kind] = max(worst[kind], e)
            if e > 4 * yard[{"param": 1, "uv": 2}[kind]]:
                failures.append((s + 1, k, e))
    val = validate_steps(net, [batch])["val_loss"]
    e_val = abs(val - float(g["val"])) / abs(float(g["val"]))
    print(f"{tag}: loss {worst['loss']:.2e} val {e_val:.2e} (yardstick {yard[0]:.2e}), original "
          f"{worst['param']:.2e} ({yard[1]:.2e}), u/v {worst['uv']:.2e} ({yard[2]:.2e})")
    assert not failures, failures[:5]
    assert worst["loss"] <= 4 * yard[0] and e_val <= 4 * yard[0]


def test_no_growth_per_step(cuda):
    """Six steps of the parametrised U-Net: the f16x3 pack registry and the device memory are after
    step 6 what they were after step 3."""
    g, net, runner, batch = _run_steps("unet", cuda, 3)
    torch.cuda.synchronize()
    reg3, mem3 = len(HF._PACK_REG), torch.cuda.memory_allocated()
    for _ in range(3):
        runner.train_step(batch)
    torch.cuda.synchronize()
    assert (len(HF._PACK_REG), torch.cuda.memory_allocated()) == (reg3, mem3)
