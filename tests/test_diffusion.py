"""DDPM diffusion without a GPU: the fp64 restatements of tests/diffusion_ref.py against the recorded
outputs of the real reference (tools/make_diffusion_golden.py), signatures and ``state_dict`` keys, the
host tables bit for bit, and everything that must raise on the host."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import diffusion_cases as C  # noqa: E402
import diffusion_ref as R  # noqa: E402

from adell_mri_amd import functional as HF  # noqa: E402
from adell_mri_amd._lib import AdellHipError  # noqa: E402
from adell_mri_amd.modules.activations import activation_factory  # noqa: E402
from adell_mri_amd.modules.diffusion import (DDPMUNetPL, Diffusion, DiffusionUNet,  # noqa: E402
                                             get_timestep_embedding)
from adell_mri_amd.modules.diffusion import diffusion_process as DP  # noqa: E402
from adell_mri_amd.modules.layers.class_attention import (  # noqa: E402
    EfficientConditioningAttentionBlock)

RT = 1e-12          # fp64 round-off, relative to the largest magnitude
SCHEDULES = ("cosine", "linear", "scaled_linear", "quadratic", "sigmoid")


@pytest.fixture(scope="module")
def meta():
    with open(os.path.join(C.GOLD, "diffusion_meta.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def process():
    return C.Gold("diffusion_process.npz")


def _close(got, ref, rt=RT):
    assert got.shape == ref.shape
    assert C.rel_err(got, ref) <= rt, C.rel_err(got, ref)


# ---- the restatements against the reference ----------------------------------------------------------
@pytest.mark.parametrize("case", C.GATE_CASES, ids=C.gate_name)
def test_ref_gates_match_the_reference(case):
    g = C.Gold("diffusion_gates.npz")
    name = C.gate_name(case)
    T = case[0]
    t, cls, sites = C.gate_inputs(case)
    emb = R.timestep_embedding(t, T)
    if cls is not None:
        emb = emb + cls
    dcls = 0.0
    for width, (p, gz) in zip(C.GATE_WIDTHS, sites):
        z, saved = R.eca_gates(emb, p)
        grads, de = R.eca_gates_backward(gz, p, saved)
        dcls = dcls + de
        if width not in C.GATE_RECORDED:
            continue
        _close(z, g[f"{name}:{width}:z"])
        ref = [g[f"{name}:{width}:grad:{k}"] for k in R.PARAM_KEYS]
        assert C.site_grad_err(grads, ref) <= 1e-11
    if cls is not None:
        _close(dcls, g[f"{name}:dcls"], 1e-11)


def test_ref_embedding_matches_the_reference(process):
    """The reference evaluates its embedding in fp32 (``t.float()``): its argument alone is off by
    |t| 2^-24, so the fp64 restatement is pinned to it at that accuracy, not at fp64 round-off."""
    for T in (1, 2, 7, 32):
        for tag in ("fraction", "integer"):
            t = process[f"emb:{T}:{tag}:t"]
            ref = process[f"emb:{T}:{tag}"]
            got = R.timestep_embedding(t, T)
            assert got.shape == ref.shape == (4, T)
            assert np.abs(got - ref).max() <= 4 * 2.0 ** -24 * max(1.0, np.abs(t).max()) + 1e-6
            if T % 2 == 1:
                assert (got[:, -1] == 0).all()
    assert (R.timestep_embedding(np.array([0.3]), 1) == 0).all()
    torch.testing.assert_close(HF.timestep_embedding(torch.tensor([0.3, 999.0]), 7).double().numpy(),
                               R.timestep_embedding(np.array([0.3, 999.0], np.float32), 7),
                               rtol=0, atol=1e-7)
    assert tuple(get_timestep_embedding(torch.tensor([0.3, 0.5]), 7).shape) == (2, 7)


def test_ref_apply_matches_the_reference():
    g = C.Gold("diffusion_apply.npz")
    seen = 0
    for shape in C.APPLY_SHAPES:
        for one_row in (False, True):
            tag = "x".join(str(v) for v in shape) + (":one" if one_row else ":all")
            if tag + ":y" not in g:
                continue
            x, z, dy = C.apply_inputs(shape, one_row)
            _close(R.eca_apply(x, z), g[tag + ":y"])
            dx, dz = R.eca_apply_backward(x, z, dy)
            _close(dx, g[tag + ":dx"])
            _close(dz, g[tag + ":dz"])
            seen += 1
    assert seen >= 6


def test_ref_noising_and_steps_match_the_reference(process):
    x, eps, eps_u, noise, tt = C.process_inputs()
    tables = {k: process["table:" + k].astype(np.float64) for k in ("beta", "alpha", "alpha_bar")}
    _close(R.noise_images(x, eps, tables["alpha_bar"], tt), process["noise:y"])
    for case in C.STEP_CASES:
        kind, t, eta, guided = case
        got = R.reverse_step(kind, x, eps, t, tables, noise=noise, eps_uncond=eps_u if guided else None,
                             scale=C.GUIDANCE_SCALE, eta=eta)
        _close(got, process["step:" + C.step_name(case)])
    bad = R.noise_images(x, eps, tables["alpha_bar"], np.array([0, 50, -1]))
    assert np.isnan(bad[1:]).all() and not np.isnan(bad[0]).any()


def test_step_coefficients_restate_the_steps(process):
    """functional.diffusion_step_coefficients (what the kernel is given) reproduces every case."""
    x, eps, eps_u, noise, _ = C.process_inputs()
    tables = {k: process["table:" + k].astype(np.float64) for k in ("beta", "alpha", "alpha_bar")}
    for case in C.STEP_CASES:
        kind, t, eta, guided = case
        (sb, sa, c_x0, c_x, c_e, c_n), flags = HF.diffusion_step_coefficients(kind, t, tables, eta, True)
        e = eps_u + C.GUIDANCE_SCALE * (eps - eps_u) if guided else eps
        out = c_x * x + c_e * e + c_n * noise
        if flags & 1:
            x0 = (x - sb * e) / sa
            out = out + c_x0 * (np.clip(x0, -1, 1) if flags & 2 else x0)
        _close(out, process["step:" + C.step_name(case)], 1e-11)
    with pytest.raises(ValueError):
        HF.diffusion_step_coefficients("euler", 1, tables)
    with pytest.raises(ValueError):
        HF.diffusion_step_coefficients("ddpm", 50, tables)


def test_ref_mse():
    rng = np.random.default_rng(0)
    a, b = rng.normal(size=63), rng.normal(size=63)
    loss, grad = R.mse(a, b)
    ta = torch.from_numpy(a).requires_grad_(True)
    ref = torch.nn.MSELoss()(ta, torch.from_numpy(b))
    ref.backward()
    assert abs(loss - float(ref)) <= RT * float(ref)
    _close(grad, ta.grad.numpy())


# ---- signatures, keys, host tables ---------------------------------------------------------------------
def _signature(cls):
    return {k: [repr(p.default) if p.default is not inspect.Parameter.empty else None, str(p.kind)]
            for k, p in inspect.signature(cls.__init__).parameters.items()}


def test_signatures_equal_the_reference(meta):
    sig = meta["signatures"]
    assert _signature(EfficientConditioningAttentionBlock) == sig["EfficientConditioningAttentionBlock"]
    assert _signature(DiffusionUNet) == sig["DiffusionUNet"]
    assert _signature(Diffusion) == sig["Diffusion"]
    assert list(inspect.signature(get_timestep_embedding).parameters) == sig["get_timestep_embedding"]
    for k in ("noise_images", "__call__", "sample_timesteps", "sample", "get_shape"):
        assert list(inspect.signature(getattr(Diffusion, k)).parameters) == sig["Diffusion." + k], k
    # the step methods keep the reference's arguments in front of the two additions
    for k in ("ddpm_reverse_step", "ddim_reverse_step", "alpha_deblending_step", "step"):
        assert list(inspect.signature(getattr(Diffusion, k)).parameters) == [
            "self", "x", "epsilon", "t", "eta", "epsilon_uncond", "scale"], k


def test_state_dict_keys_and_strict_load(meta):
    eca = EfficientConditioningAttentionBlock(32, 5, op_type="linear")
    assert {k: list(v.shape) for k, v in eca.state_dict().items()} == meta["state"]["eca_linear_32_5"]
    assert set(eca.state_dict()) == {f"{m}.{p}" for m in ("class_to_channels", "op.1", "op.2", "op.4")
                                     for p in ("weight", "bias")}
    for name in C.NETS:
        net = DiffusionUNet(**C.net_kwargs(name, activation_factory))
        ref = meta["state"][name]
        assert {k: list(v.shape) for k, v in net.state_dict().items()} == ref
        net.load_state_dict({k: torch.zeros(s) for k, s in ref.items()}, strict=True)
        L = len(net.depth)
        assert len(net.encoder_eca) == L and len(net.decoder_eca) == len(net.link_eca) == L - 1
        assert (net.embedding is None) == (not net.classifier_free_guidance)
        assert net.n_classes == net.in_channels and net.feature_conditioning is None
        assert not isinstance(net.final_layer[-1], (torch.nn.Sigmoid, torch.nn.Softmax))
        assert len(net.final_layer) == 3
    pl = DDPMUNetPL(Diffusion(noise_steps=C.NET_STEPS, img_size=(16, 16)),
                    **C.net_kwargs("net2d", activation_factory))
    assert set(pl.state_dict()) == set(meta["state"]["net2d"])


def test_schedules_and_tables_bit_for_bit(process):
    for n in (1, 2, 50):
        for s in SCHEDULES:
            d = Diffusion(noise_steps=n, img_size=(8, 8), scheduler=s)
            assert np.array_equal(d.beta.numpy(), process[f"beta:{s}:{n}"], equal_nan=True), (s, n)
            assert np.array_equal(d.alpha_bar.numpy(), process[f"alpha_bar:{s}:{n}"], equal_nan=True)
            assert np.array_equal(getattr(DP, s + "_beta_schedule")(n).numpy(), process[f"beta:{s}:{n}"],
                                  equal_nan=True)
    d = Diffusion(noise_steps=C.PROCESS_STEPS, img_size=C.PROCESS_SHAPE[2:], scheduler="cosine")
    assert list(d.get_shape()) == list(process["get_shape:none"])
    assert list(d.get_shape(torch.zeros(2, 1, 3, 3))) == list(process["get_shape:x4"])
    for k in ("beta", "alpha", "alpha_bar"):
        assert np.array_equal(getattr(d, k).numpy(), process["table:" + k])
        assert d.tables[k] == process["table:" + k].astype(np.float64).tolist()
    assert d.sample_timesteps(5).shape == (5,)


# ---- raises, all on the host ------------------------------------------------------------------------------
def test_raises_on_the_host():
    kw = C.net_kwargs("net2d", activation_factory)
    missing = {k: v for k, v in kw.items() if k != "in_channels"}
    with pytest.raises(Exception, match="in_channels must be defined"):
        DiffusionUNet(**missing)
    with pytest.raises(NotImplementedError, match="conv"):
        EfficientConditioningAttentionBlock(8, 4)           # op_type="conv" is the class default
    with pytest.raises(NotImplementedError, match="conv"):
        EfficientConditioningAttentionBlock(8, 4, op_type="conv")
    for bad in (dict(noise_steps=10.0), dict(beta_start=1), dict(beta_end=1), dict(img_size=8),
                dict(img_size=(8,)), dict(img_size=(8, 8.0))):
        with pytest.raises(TypeError):
            Diffusion(**{**dict(noise_steps=10, img_size=(8, 8), scheduler="linear"), **bad})
    with pytest.raises(TypeError):
        DDPMUNetPL("not a diffusion", **kw)


def test_cpu_tensors_are_refused():
    net = DiffusionUNet(**C.net_kwargs("net2d", activation_factory))
    x = torch.zeros(C.NETS["net2d"]["shape"])
    with pytest.raises(AdellHipError):
        net(x, torch.tensor([0.5]))
    eca = EfficientConditioningAttentionBlock(8, 4, op_type="linear")
    with pytest.raises(AdellHipError):
        HF.eca_gates(torch.tensor([0.5]), [eca])
    with pytest.raises(AdellHipError):
        HF.eca_apply(torch.zeros(1, 4, 2, 2, 2), torch.zeros(1, 4))
    with pytest.raises(AdellHipError):
        HF.diffusion_noise(x, x, torch.ones(5), torch.zeros(2, dtype=torch.int64))
    tables = Diffusion(noise_steps=5, img_size=(16, 16)).tables
    with pytest.raises(AdellHipError):
        HF.diffusion_reverse_step("ddim", x, x, 1, tables, noise=x)
    with pytest.raises(AdellHipError):
        HF.mse_loss(x, x)
    with pytest.raises(ValueError, match="adds noise"):
        HF.diffusion_reverse_step("ddpm", x, x, 1, tables)


def test_cls_without_guidance_raises():
    net = DiffusionUNet(**C.net_kwargs("net2d", activation_factory))
    assert net.classifier_free_guidance is False and net.embedding is None
    with pytest.raises(Exception, match="cls can only be defined"):
        net(torch.zeros(C.NETS["net2d"]["shape"]), torch.tensor([0.5]), torch.tensor([0, 1]))
