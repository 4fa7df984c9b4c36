"""DDPM diffusion on the GPU: the kernels of csrc/diffusion.hip against the fp64 restatements
(tests/diffusion_ref.py, pinned to the reference by tests/test_diffusion.py), every kernel result
computed twice and compared bit for bit; the two fixture networks (forward, two training steps, a
validation step) and the three sampling chains against the real reference (tests/golden/diffusion_*).

Tolerances are the project's for these kinds of quantity (tests/test_mil_gpu.py): ``SUM_BOUND`` = 5e-5
of the largest reference magnitude for kernel outputs and gradients; in the step tests loss 1e-4,
gradients 5e-3 by ``cases.grad_rel_err``, parameters (2e-4, 2e-6). Where the reference's own
fp32-against-fp64 error uses more than a quarter of one of them, tools/make_diffusion_golden.py stored
four times that error as the bound (``bound:*``) and the test reads it. The sampling chains have no
other bound than that: four times the reference's recorded fp32-against-fp64 error of the chain."""
import numpy as np
import pytest
import torch

import diffusion_cases as C
import diffusion_ref as R
from cases import grad_rel_err

pytestmark = pytest.mark.gpu


def dev_t(a, cuda, dtype=torch.float32):
    return torch.from_numpy(np.asarray(a)).to(dtype).to(cuda)


def channels_last(t):
    return t.contiguous(memory_format=torch.channels_last_3d if t.dim() == 5 else torch.channels_last)


def host(t):
    return t.detach().double().cpu().numpy()


def twice(fn):
    """fn() run two times: the first result, after asserting that the second is bit-identical."""
    a, b = fn(), fn()
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:     # bit for bit (a NaN equals the same NaN)
            assert u.dtype == v.dtype == torch.float32 and u.shape == v.shape
            assert torch.equal(u.contiguous().view(torch.int32), v.contiguous().view(torch.int32)), \
                "two runs differ"
    return a


@pytest.fixture(scope="module")
def process():
    return C.Gold("diffusion_process.npz")


# ---- gate apply ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_row", [False, True], ids=["rows", "one_row"])
@pytest.mark.parametrize("shape", C.APPLY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_eca_apply(cuda, shape, one_row):
    from adell_mri_amd import functional as HF

    x, z, dy = C.apply_inputs(shape, one_row)
    xd, zd, dyd = channels_last(dev_t(x, cuda)), dev_t(z, cuda), channels_last(dev_t(dy, cuda))

    def run():
        xg, zg = xd.clone().requires_grad_(True), zd.clone().requires_grad_(True)
        y = HF.eca_apply(xg, zg)
        y.backward(dyd)
        return y.detach(), xg.grad, zg.grad

    y, dx, dz = twice(run)
    ry = R.eca_apply(x, z)
    rdx, rdz = R.eca_apply_backward(x, z, dy)
    errs = C.rel_err(host(y), ry), C.rel_err(host(dx), rdx), C.rel_err(host(dz), rdz)
    print(f"eca_apply {shape} one_row={one_row}: y {errs[0]:.2e} dx {errs[1]:.2e} dz {errs[2]:.2e}")
    assert y.stride() == xd.stride() and dx.stride() == xd.stride()
    assert max(errs) < C.SUM_BOUND, errs


def test_eca_apply_refuses_views_and_wrong_rows(cuda):
    from adell_mri_amd import functional as HF
    from adell_mri_amd._lib import AdellHipError

    x = channels_last(torch.randn(2, 8, 4, 6, 5, device=cuda))
    z = torch.randn(2, 8, device=cuda)
    with pytest.raises(AdellHipError):
        HF.eca_apply(x[:, :, :, ::2], z)                      # a view with gaps
    with pytest.raises(AdellHipError):
        HF.eca_apply(x, torch.randn(1, 8, device=cuda).expand(2, 8))   # an expanded gate row
    with pytest.raises(AdellHipError):
        HF.eca_apply(x, torch.randn(2, 16, device=cuda)[:, ::2])
    with pytest.raises(ValueError):
        HF.eca_apply(x, torch.randn(3, 8, device=cuda))
    with pytest.raises(AdellHipError):
        HF.eca_apply(x.double(), z)


# ---- gate logits ----------------------------------------------------------------------------------------
def _sites(case, cuda):
    from adell_mri_amd.modules.layers.class_attention import EfficientConditioningAttentionBlock

    T = case[0]
    t, cls, sites = C.gate_inputs(case)
    blocks = []
    for width, (p, _) in zip(C.GATE_WIDTHS, sites):
        blk = EfficientConditioningAttentionBlock(T, width, op_type="linear")
        blk.load_state_dict({k: torch.from_numpy(v).float() for k, v in zip(R.PARAM_KEYS, p)})
        blocks.append(blk.to(cuda))
    return t, cls, sites, blocks


def _block_params(blk):
    sd = dict(blk.named_parameters())
    return [sd[k] for k in R.PARAM_KEYS]


@pytest.mark.parametrize("case", C.GATE_CASES, ids=C.gate_name)
def test_eca_gates(cuda, case):
    """Site widths 1, 5, 33 and 130 in one call: the logits, every parameter gradient and the gradient
    of the class embedding."""
    from adell_mri_amd import functional as HF

    g = C.Gold("diffusion_gates.npz")
    name, T = C.gate_name(case), case[0]
    t, cls, sites, blocks = _sites(case, cuda)
    td = dev_t(t, cuda)
    gzs = [dev_t(gz, cuda) for _, gz in sites]

    def run():
        for blk in blocks:
            blk.zero_grad()
        cd = dev_t(cls, cuda).requires_grad_(True) if cls is not None else None
        zs = HF.eca_gates(td, blocks, cd)
        torch.autograd.backward(zs, gzs)
        grads = [p.grad.clone() for blk in blocks for p in _block_params(blk)]
        return [z.detach() for z in zs] + grads + [cd.grad if cd is not None else None]

    out = twice(run)
    n = len(blocks)
    zs, grads, dcls = out[:n], out[n:-1], out[-1]
    emb = R.timestep_embedding(t, T)
    if cls is not None:
        emb = emb + cls
    bz, bg = float(g[f"bound:{name}:z"]), float(g[f"bound:{name}:grad"])
    rdcls, worst_z, worst_g = 0.0, 0.0, 0.0
    for i, (width, (p, gz)) in enumerate(zip(C.GATE_WIDTHS, sites)):
        rz, saved = R.eca_gates(emb, p)
        rgrads, de = R.eca_gates_backward(gz, p, saved)
        rdcls = rdcls + de
        assert tuple(zs[i].shape) == rz.shape
        worst_z = max(worst_z, C.rel_err(host(zs[i]), rz))
        worst_g = max(worst_g, C.site_grad_err([host(v) for v in grads[8 * i:8 * i + 8]], rgrads))
    if cls is not None:
        worst_g = max(worst_g, C.rel_err(host(dcls), rdcls))
    print(f"eca_gates {name}: z {worst_z:.2e} (bound {bz:.2e}), gradients {worst_g:.2e} (bound {bg:.2e})")
    assert worst_z < bz and worst_g < bg


def test_eca_block_forward_and_composed_route(cuda):
    """A stand-alone block is eca_apply(X, eca_gates(...)) of its conditioning vector; sites wider than
    the grouped kernels take (1030 channels) compose the same logits from the package's Linear /
    LayerNorm / activation kernels."""
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.layers.class_attention import EfficientConditioningAttentionBlock

    case = (7, 3, True, "fraction")
    t, cls, sites, blocks = _sites(case, cuda)
    blk, (p, _) = blocks[2], sites[2]
    x, _, _ = C.apply_inputs((3, 33, 2, 3, 2), False)
    y = blk(channels_last(dev_t(x, cuda)), dev_t(cls, cuda)[:, None, :])
    rz, _ = R.eca_gates(cls, p)
    assert C.rel_err(host(y), R.eca_apply(x, rz)) < C.SUM_BOUND

    torch.manual_seed(3)
    wide = EfficientConditioningAttentionBlock(7, 1030, op_type="linear").to(cuda)
    z = HF.eca_gates(dev_t(t, cuda), [wide], dev_t(cls, cuda))[0]
    rz, _ = R.eca_gates(R.timestep_embedding(t, 7) + cls, [host(v) for v in _block_params(wide)])
    print(f"composed gates, 1030 channels: {C.rel_err(host(z), rz):.2e}")
    assert C.rel_err(host(z), rz) < 1e-4        # the Linear kernels' own bound (f16x3 GEMM)


# ---- noising and reverse steps ---------------------------------------------------------------------------
def test_diffusion_noise(cuda, process):
    from adell_mri_amd import functional as HF

    x, eps, _, _, tt = C.process_inputs()
    ab = process["table:alpha_bar"]
    abd = dev_t(ab, cuda)
    for fmt in (lambda v: v, channels_last):
        xd, ed = fmt(dev_t(x, cuda)), fmt(dev_t(eps, cuda))
        (y,) = twice(lambda: (HF.diffusion_noise(xd, ed, abd, dev_t(tt, cuda, torch.int64)),))
        assert C.rel_err(host(y), process["noise:y"]) < float(process["bound:noise"])
        (bad,) = twice(lambda: (HF.diffusion_noise(xd, ed, abd, dev_t([0, 50, -1], cuda, torch.int64)),))
        assert torch.isnan(bad[1:]).all()                       # out of range: never an index
        assert torch.equal(bad[0], HF.diffusion_noise(xd, ed, abd, dev_t([0, 0, 0], cuda, torch.int64))[0])
    # odd sizes: the scalar route
    xo, eo = dev_t(x, cuda)[:, :1, :, :, :1].contiguous(), dev_t(eps, cuda)[:, :1, :, :, :1].contiguous()
    y = HF.diffusion_noise(xo, eo, abd, dev_t(tt, cuda, torch.int64))
    assert C.rel_err(host(y), R.noise_images(host(xo), host(eo), ab.astype(np.float64), tt)) < C.SUM_BOUND


@pytest.mark.parametrize("case", C.STEP_CASES, ids=C.step_name)
def test_reverse_step(cuda, process, case):
    from adell_mri_amd import functional as HF

    kind, t, eta, guided = case
    x, eps, eps_u, noise, _ = C.process_inputs()
    tables = {k: process["table:" + k].astype(np.float64).tolist() for k in ("beta", "alpha", "alpha_bar")}
    name = C.step_name(case)
    for fmt in (lambda v: v, channels_last):
        xd, ed, ud, nd = (fmt(dev_t(v, cuda)) for v in (x, eps, eps_u, noise))
        (out,) = twice(lambda: (HF.diffusion_reverse_step(
            kind, xd, ed, t, tables, noise=nd, eps_uncond=ud if guided else None,
            scale=C.GUIDANCE_SCALE, eta=eta),))
        err = C.rel_err(host(out), process["step:" + name])
        assert err < float(process["bound:step:" + name]), (name, err)
    # odd element count: the scalar route
    cut = [v.reshape(-1)[:61] for v in (x, eps, eps_u, noise)]
    cd = [dev_t(v, cuda) for v in cut]
    out = HF.diffusion_reverse_step(kind, cd[0], cd[1], t, tables, noise=cd[3],
                                    eps_uncond=cd[2] if guided else None, scale=C.GUIDANCE_SCALE, eta=eta)
    ref = R.reverse_step(kind, cut[0], cut[1], t, tables, noise=cut[3],
                         eps_uncond=cut[2] if guided else None, scale=C.GUIDANCE_SCALE, eta=eta)
    assert C.rel_err(host(out), ref) < float(process["bound:step:" + name])


def test_diffusion_class_steps_and_mixed_layouts(cuda, process):
    """The methods of ``Diffusion`` draw through ``randn_like`` and bring a row-major x to the layout
    of a channels-last prediction."""
    from adell_mri_amd.modules.diffusion import Diffusion

    x, eps, eps_u, noise, _ = C.process_inputs()
    for kind in R.STEP_KINDS:
        d = Diffusion(noise_steps=C.PROCESS_STEPS, img_size=C.PROCESS_SHAPE[2:], scheduler="cosine",
                      step_key=kind)
        draws = []
        d.randn_like = lambda v: draws.append(1) or dev_t(noise, cuda)
        out = d.step(dev_t(x, cuda), channels_last(dev_t(eps, cuda)), 23,
                     epsilon_uncond=dev_t(eps_u, cuda), scale=C.GUIDANCE_SCALE)
        name = C.step_name((kind, 23, 1.0, True))
        assert C.rel_err(host(out), process["step:" + name]) < float(process["bound:step:" + name])
        assert len(draws) == (0 if kind == "alpha_deblending" else 1)
        assert out.is_contiguous(memory_format=torch.channels_last_3d)


# ---- mean squared error ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.MSE_SIZES)
def test_mse_loss(cuda, n):
    from adell_mri_amd import functional as HF

    rng = np.random.default_rng(n)
    a, b = C._f32(rng.normal(size=n)), C._f32(rng.normal(size=n))
    ad, bd = dev_t(a, cuda), dev_t(b, cuda)

    def run():
        ag = ad.clone().requires_grad_(True)
        loss = HF.mse_loss(ag, bd)
        (loss * 3.0).backward()
        return loss.detach(), ag.grad

    loss, grad = twice(run)
    rl, rg = R.mse(a, b)
    assert loss.dim() == 0
    assert abs(float(loss) - rl) <= C.SUM_BOUND * rl
    assert C.rel_err(host(grad), 3.0 * rg) < C.SUM_BOUND


def test_mse_loss_mixed_layouts(cuda):
    from adell_mri_amd import functional as HF

    rng = np.random.default_rng(9)
    a, b = C._f32(rng.normal(size=(2, 3, 4, 5, 6))), C._f32(rng.normal(size=(2, 3, 4, 5, 6)))
    loss = HF.mse_loss(channels_last(dev_t(a, cuda)), dev_t(b, cuda))
    assert abs(float(loss) - R.mse(a, b)[0]) <= C.SUM_BOUND * R.mse(a, b)[0]


# ---- networks ------------------------------------------------------------------------------------------------
def build_net(name, cuda, gain, noise_steps=C.NET_STEPS, step_key="ddpm"):
    from adell_mri_amd.modules.activations import activation_factory
    from adell_mri_amd.modules.diffusion import DDPMUNetPL, Diffusion

    cfg = C.NETS[name]
    d = Diffusion(noise_steps=noise_steps, img_size=cfg["img_size"], step_key=step_key)
    net = DDPMUNetPL(d, image_key="image", cls_key="cls" if cfg["cls"] is not None else None,
                     learning_rate=C.STEP_LR, weight_decay=C.STEP_WD, optimizer_eps=C.STEP_EPS,
                     **C.net_kwargs(name, activation_factory))
    net.load_state_dict(C.fill(net.state_dict(), gain))
    return net.to(cuda).train()


@pytest.mark.parametrize("name", list(C.NETS))
def test_network_steps_match_reference(cuda, name):
    """Forward output, two training steps through ``StepRunner`` (loss, every gradient, the
    parameters after each) and the validation loss; then ``step`` with noise and timesteps given
    under torch's synchronisation check."""
    from adell_mri_amd.optim import FusedAdamW
    from adell_mri_amd.trainer import StepRunner, validate_steps

    files = (f"diffusion_{name}.npz", f"diffusion_{name}_step2.npz")
    g, g2 = C.Gold(files[0]), C.Gold(files[1])
    cfg = C.NETS[name]
    net = build_net(name, cuda, float(g["gain"]))
    x, eps = C.net_inputs(name)
    xd = dev_t(x, cuda)
    cls = torch.tensor(cfg["cls"]).to(cuda) if cfg["cls"] is not None else None
    batch = {"image": xd}
    if cls is not None:
        batch["cls"] = cls
    feed = {}
    net.randn_like = lambda v: dev_t(eps[feed["i"]], cuda)
    net.timesteps_like = lambda v: torch.tensor(C.NET_TIMESTEPS[feed["i"]]).to(cuda)
    runner = StepRunner(net)
    assert isinstance(runner.optimizer, FusedAdamW)
    b_loss, b_grad = float(g["bound:loss"]), float(g["bound:grad"])
    b_param, b_pred = float(g["bound:param_scale"]), float(g["bound:pred"])
    rt, at = C.STEP_TOL["param"]

    with torch.no_grad():
        noised, _ = net.diffusion.noise_images(xd, dev_t(eps[0], cuda), torch.tensor(C.NET_TIMESTEPS[0]))
        pred = net(noised, torch.tensor(C.NET_TIMESTEPS[0]).to(cuda) / C.NET_STEPS, cls)
    e = C.rel_err(host(pred), g["pred1"].astype(np.float64))
    print(f"{name}: forward {e:.2e} (bound {b_pred:.2e})")
    assert e < b_pred

    for i, gold in ((0, g), (1, g2)):
        feed["i"] = i
        runner.optimizer.zero_grad()
        loss = net.training_step(batch, i)
        ref_loss = float(g[f"loss{i + 1}"])
        loss.backward()
        worst = 0.0
        view = _GradView(C.Gold(files[i], f"grad{i + 1}:"))
        for k, p in net.named_parameters():
            assert p.grad is not None, k
            worst = max(worst, grad_rel_err(view, k, p.grad.cpu().numpy()))
        print(f"{name} step {i + 1}: loss {abs(loss.item() - ref_loss) / ref_loss:.2e} (bound "
              f"{b_loss:.1e}), worst gradient {worst:.2e} (bound {b_grad:.1e})")
        assert abs(loss.item() - ref_loss) <= b_loss * ref_loss
        assert worst < b_grad
        runner.optimizer.step()
        for k, v in net.state_dict().items():
            if v.is_floating_point():
                np.testing.assert_allclose(v.detach().cpu().numpy(), gold[f"step{i + 1}:" + k],
                                           rtol=rt * b_param, atol=at * b_param, err_msg=k)
    feed["i"] = 2
    out = validate_steps(net, [batch])
    ref_val = float(g["val_loss"])
    print(f"{name}: validation {abs(out['val_loss'] - ref_val) / ref_val:.2e}")
    assert abs(out["val_loss"] - ref_val) <= b_loss * ref_val
    assert net.training

    # step with everything given: nothing in it may wait for the device (the network body in front
    # of the loss is exempt: it runs once outside the check, then the noising and the loss inside)
    e0, t0 = dev_t(eps[0], cuda), torch.tensor(C.NET_TIMESTEPS[0]).to(cuda)
    first = net.step(xd, timesteps=t0, cls=cls, epsilon=e0).detach()
    with torch.no_grad():
        prediction = net.diffusion(xd, net, e0, t0, cls)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        noised, _ = net.diffusion.noise_images(xd, e0, t0)
        second = net.calculate_loss(prediction, e0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first, second)


class _GradView:
    """``grad:<key>`` records of one training step (what cases.grad_rel_err reads)."""

    def __init__(self, gold):
        self._g = gold
        self.files = ["grad:" + k for k in gold.files]

    def __getitem__(self, k):
        return self._g[k[len("grad:"):]]


@pytest.mark.parametrize("kind", R.STEP_KINDS)
def test_sampling_chain_matches_reference(cuda, kind):
    """A chain of noise_steps = 6 with guidance and replayed noise against the recorded final image.
    The bound is four times the reference's own fp32-against-fp64 error of the chain."""
    g = C.Gold("diffusion_sample.npz")
    net = build_net("net3d", cuda, float(g["gain"]), noise_steps=C.SAMPLE_STEPS, step_key=kind)
    noises = [dev_t(g[f"{kind}:noise{i}"], cuda) for i in range(int(g[f"{kind}:n_noise"]))]
    drawn = []

    def replay(v):
        drawn.append(1)
        return noises[len(drawn) - 1]

    net.diffusion.randn_like = replay
    calls = []
    forward = net.forward
    net.forward = lambda *a, **k: calls.append(len(a) + len(k)) or forward(*a, **k)
    final = net.diffusion.sample(net, x=dev_t(g["x_T"], cuda), classification=torch.tensor(C.SAMPLE_CLS).to(cuda),
                                 classification_scale=C.GUIDANCE_SCALE)
    assert net.training and len(drawn) == len(noises)
    assert len(calls) == 2 * (C.SAMPLE_STEPS - 1)            # t = 5 .. 1, twice per step: guidance
    err, bound = C.rel_err(host(final), g[f"{kind}:final"]), float(g[f"bound:{kind}"])
    print(f"sample {kind}: {err:.3e} of the largest value; bound {bound:.3e} (the reference's own "
          f"fp32 chain: {float(g[f'{kind}:fp32_vs_fp64']):.3e})")
    assert err < bound


def test_fit_and_validate_steps_take_the_wrapper(cuda):
    """``fit_steps`` / ``validate_steps`` unchanged; noise drawn by the wrapper (CPU generator, then
    on the device); a batch whose ``cls`` is dropped leaves the class embedding without a gradient."""
    from adell_mri_amd.trainer import fit_steps, validate_steps

    net = build_net("net3d", cuda, 1.0)
    x, _ = C.net_inputs("net3d")
    batch = {"image": dev_t(x, cuda), "cls": torch.tensor(C.NETS["net3d"]["cls"]).to(cuda)}
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    losses = fit_steps(net, [batch, batch])
    assert len(losses) == 2 and all(np.isfinite(float(v)) for v in losses)
    assert float(losses[0]) != float(losses[1])                  # fresh noise and timesteps per step
    assert any(not torch.equal(v, before[k]) for k, v in net.state_dict().items())
    out = validate_steps(net, [batch])
    assert list(out) == ["val_loss"] and np.isfinite(out["val_loss"]) and net.training

    net.device_noise = True
    assert net.randn_like(batch["image"]).is_cuda and net.timesteps_like(batch["image"]).dtype == torch.int64
    assert np.isfinite(float(net.training_step(batch, 0)))

    net = build_net("net3d", cuda, 1.0)                          # fresh optimiser state
    net.uncondition_proba = 1.0                                  # every batch drops cls
    embedding = net.embedding.weight.detach().clone()
    assert all(np.isfinite(float(v)) for v in fit_steps(net, [batch]))
    assert net.unpack_batch(batch)[1] is None
    # untouched but for AdamW's weight decay: no gradient reached it
    assert torch.allclose(net.embedding.weight, embedding, rtol=1e-4, atol=0)
