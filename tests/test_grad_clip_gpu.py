"""Gradient-norm clipping and gradient accumulation on the device (csrc/grad_clip.hip,
optim._FusedBase.clip_grad_norm_, FlatParameters.fold, StepRunner(gradient_clip_val,
accumulate_grad_batches)) against torch.nn.utils.clip_grad_norm_ and the loop Lightning runs
(entrypoints/segmentation/train.py:807,811)."""
import itertools
import math
import os
import sys

import numpy as np
import pytest
import torch

from adell_mri_amd import functional as HF
from adell_mri_amd import ops

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

INF = float("inf")


def _clip_flat(g, max_norm, norm_inf, scale):
    """The three kernels on one buffer: returns (total, coef) as host floats."""
    ws = ops.grad_norm_workspace(1, g.device)
    out = torch.empty(2, dtype=torch.float32, device=g.device)
    ops.grad_norm_partials(g, norm_inf, ws, 0)
    ops.grad_norm_finalize(ws, 1, norm_inf, scale, max_norm, out)
    ops.grad_scale_by(g, out[1:])
    torch.cuda.synchronize()
    return out.cpu()


# ---- 1. kernel-level parity ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 255, 16384, 16385, 2 ** 20 + 7, 36_100_000])
@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_kernels_match_fp64(cuda, n, norm_type):
    norm_inf = math.isinf(norm_type)
    gen = torch.Generator().manual_seed(n)
    host = torch.randn(n, generator=gen) * 1e-2
    g0 = host.to(cuda)
    ref = host.double().numpy()
    for scale in (1.0, 0.5, 0.25):
        want = float(np.max(np.abs(scale * ref))) if norm_inf else float(np.linalg.norm(scale * ref))
        for max_norm in (0.5 * want, 2.0 * want):
            g = g0.clone()
            out = _clip_flat(g, max_norm, norm_inf, scale)
            total, coef = float(out[0]), float(out[1])
            if norm_inf:
                assert total == np.float32(want), (total, want)
            else:
                assert abs(total - want) <= 1e-6 * want, (total, want)
            # torch: coef = reciprocal(total + 1e-6) * max_norm in fp32, clamped at 1
            c = min(float(np.float32(1.0) / (np.float32(total) + np.float32(1e-6)) * np.float32(max_norm)), 1.0)
            assert coef == 1.0 if c == 1.0 else abs(coef - c) <= 1e-6 * c, (coef, c)
            got = g.cpu()
            if coef == 1.0:
                assert torch.equal(got, host)                  # bit-unchanged
            else:
                exp = ref * float(coef)
                assert np.allclose(got.double().numpy(), exp, rtol=1e-6, atol=0), n
    # reproducible: two calls on the same buffer, identical bits
    g = g0.clone()
    a = _clip_flat(g, 1e30, norm_inf, 1.0)
    b = _clip_flat(g, 1e30, norm_inf, 1.0)
    assert torch.equal(a, b)


def test_multi_accumulate_adds(cuda):
    src = [torch.randn(n, device=cuda) for n in (5, 16384, 7)]
    dst = torch.randn(16384 + 16, device=cuda)
    want = dst.clone()
    rows = [(src[0].data_ptr(), 0, 5), (src[1].data_ptr(), 8, 16384), (src[2].data_ptr() + 4, 16392, 6)]
    want[0:5] += src[0]
    want[8:16392] += src[1]
    want[16392:16398] += src[2][1:]
    table = torch.tensor(rows, dtype=torch.int64, device=cuda)
    ops.multi_accumulate(table, len(rows), dst)
    torch.cuda.synchronize()
    assert torch.equal(dst, want)


# ---- 2. non-finite gradients against torch on the CPU --------------------------------------------------
def _params(cuda, sizes, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=gen).to(cuda)) for n in sizes]


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        p.grad = g.clone().to(p.device)


@pytest.mark.parametrize("case", ["nan_2", "inf_2", "nan_inf", "inf_inf"])
def test_non_finite_like_torch(cuda, case):
    from adell_mri_amd.optim import FusedSGD

    sizes = [7, 64, 33]
    params = _params(cuda, sizes, 3)
    opt = FusedSGD(params, lr=0.1)
    gen = torch.Generator().manual_seed(5)
    grads = [torch.randn(n, generator=gen) for n in sizes]
    bad = float("nan") if case.startswith("nan") else INF
    grads[1][5] = bad
    norm_type = 2.0 if case.endswith("_2") else INF
    cpu = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
    _set_grads(cpu, grads)
    want = torch.nn.utils.clip_grad_norm_(cpu, 1.0, norm_type=norm_type)
    _set_grads(params, grads)
    got = opt.clip_grad_norm_(1.0, norm_type=norm_type)
    assert got.dim() == 0 and got.dtype == torch.float32 and got.is_cuda
    torch.testing.assert_close(got.cpu(), want, equal_nan=True, rtol=1e-6, atol=0)
    for p, c in zip(params, cpu):
        torch.testing.assert_close(p.grad.cpu(), c.grad, equal_nan=True, rtol=1e-6, atol=0)
    _set_grads(params, grads)
    with pytest.raises(RuntimeError, match="non-finite"):
        opt.clip_grad_norm_(1.0, norm_type=norm_type, error_if_nonfinite=True)


def test_norm_type_must_be_2_or_inf(cuda):
    from adell_mri_amd.optim import FusedSGD

    opt = FusedSGD(_params(cuda, [4], 0), lr=0.1)
    for bad in (1.0, 3.0, -INF, 0.0):
        with pytest.raises(ValueError):
            opt.clip_grad_norm_(1.0, norm_type=bad)


# ---- 3. optimiser level: groups, stale slots ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_optimizer_clip_over_groups_skips_stale_slots(cuda, kind):
    from adell_mri_amd.optim import FusedAdamW, FusedSGD

    sizes = [10, 37, 256, 5, 1000, 3]
    params = _params(cuda, sizes, 11)
    groups = [{"params": params[:3], "lr": 0.0}, {"params": params[3:]}]   # the lr_encoder case
    opt = (FusedSGD(groups, lr=0.1, momentum=0.9, nesterov=True) if kind == "sgd"
           else FusedAdamW(groups, lr=1e-3))
    gen = torch.Generator().manual_seed(12)
    grads = [torch.randn(n, generator=gen) for n in sizes]
    _set_grads(params, grads)
    opt.collect_grads()
    stale = 4
    params[stale].grad = None                       # dropped after collect(): stale slot
    flat = opt.flat_groups[1]
    slot_before = flat.slot(stale - 3).clone()
    cpu = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
    _set_grads(cpu, grads)
    live = [c for i, c in enumerate(cpu) if i != stale]
    want = torch.nn.utils.clip_grad_norm_(live, 0.5)
    got = opt.clip_grad_norm_(0.5)
    torch.testing.assert_close(got.cpu(), want, rtol=1e-6, atol=0)
    assert float(got) > 0.5                          # it clipped
    for i, p in enumerate(params):
        if i == stale:
            assert p.grad is None
            continue
        torch.testing.assert_close(p.grad.cpu(), cpu[i].grad, rtol=1e-6, atol=1e-9)
    assert torch.equal(flat.slot(stale - 3), slot_before)
    # an all-frozen group next to a live one is skipped
    frozen = torch.nn.Parameter(torch.zeros(4, device=cuda), requires_grad=False)
    other = _params(cuda, [10], 13)
    opt2 = FusedSGD([{"params": [frozen]}, {"params": other}], lr=0.1)
    other[0].grad = grads[0].to(cuda)
    torch.testing.assert_close(opt2.clip_grad_norm_(1e9).cpu(), grads[0].norm(), rtol=1e-6, atol=0)


# ---- 4. only adell kernels -------------------------------------------------------------------------------
def _device_kernels(prof):
    out = []
    for e in prof.events():
        if e.device_type != torch.autograd.DeviceType.CUDA:
            continue
        name = e.name
        if name.lower().startswith(("memcpy", "memset")):
            continue
        out.append(name)
    return out


def test_clip_and_fold_launch_only_adell_kernels(cuda):
    from torch.profiler import ProfilerActivity, profile

    from adell_mri_amd.optim import FusedSGD

    sizes = [10, 37, 256, 5, 1000, 3]
    params = _params(cuda, sizes, 21)
    opt = FusedSGD([{"params": params[:3]}, {"params": params[3:]}], lr=0.1)
    opt.zero_grad()
    for p in params:
        p.grad = torch.randn_like(p)
    opt.collect_grads()
    params[1].grad = None                 # two runs in group 0, one in group 1
    runs = sum(len(f.runs(f.has_grad())) for f in opt.flat_groups)
    assert runs == 3
    opt.clip_grad_norm_(1.0)              # sizes the workspace
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        opt.clip_grad_norm_(1e-3)
        torch.cuda.synchronize()
    names = _device_kernels(prof)
    assert names and all(n.startswith("adell_") for n in names), names
    assert len(names) <= 2 * runs + 1, names
    assert any("grad_norm_partials" in n for n in names)
    # an accumulation fold
    opt.zero_grad()
    fresh = [torch.randn_like(p) for p in params]
    torch.cuda.synchronize()
    for p, g in zip(params, fresh):
        p.grad = g
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        opt.fold_grads()
        torch.cuda.synchronize()
    names = _device_kernels(prof)
    assert names and all(n.startswith("adell_") for n in names), names
    assert any("multi_accumulate" in n for n in names)


# ---- 5-6. whole steps on the small U-Net ----------------------------------------------------------------
def _batches(cuda):
    g = np.load(os.path.join(ROOT, "tests", "golden", "unet3d_cfg2_small.npz"))
    x, y = torch.from_numpy(g["x"]).to(cuda), torch.from_numpy(g["y"]).to(cuda)
    return [{"image": x[i:i + 1], "mask": y[i:i + 1]} for i in range(2)]


def _net(cuda, kind):
    import ddp_worker

    from adell_mri_amd.optim import FusedAdamW

    net = ddp_worker.build(cuda)
    if kind == "sgd":
        opt = net.configure_optimizers()["optimizer"]
    else:
        opt = FusedAdamW(net.parameters(), lr=1e-3, weight_decay=5e-3)
    return net, opt


def _reference_window(net, opt, sync, micro, n, clip, idx0):
    """Today's eager loop: zero_grad; (loss_i / n).backward() for each micro-batch; all_reduce;
    stock clip_grad_norm_; step."""
    opt.zero_grad()
    for k, b in enumerate(micro):
        loss = net.training_step(b, idx0 + k)
        (loss / n if n > 1 else loss).backward()
    sync.all_reduce()
    norm = None
    if clip:
        norm = torch.nn.utils.clip_grad_norm_([p for p in net.parameters() if p.grad is not None], clip)
    opt.step()
    return norm


def _params_of(net):
    torch.cuda.synchronize()
    return {k: p.detach().cpu().clone() for k, p in net.named_parameters()}


def _assert_close(a, b):
    for k in a:
        assert torch.allclose(a[k], b[k], rtol=1e-4, atol=2e-6), (k, float((a[k] - b[k]).abs().max()))


def _first_norm(cuda, kind, batch):
    from adell_mri_amd.parallel import GradSync

    net, opt = _net(cuda, kind)
    sync = GradSync(opt)
    opt.zero_grad()
    net.training_step(batch, 0).backward()
    sync.all_reduce()
    return float(torch.nn.utils.clip_grad_norm_([p for p in net.parameters() if p.grad is not None], 1e30))


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_clipped_steps_match_stock_clip(cuda, kind, monkeypatch):
    from adell_mri_amd.parallel import GradSync
    from adell_mri_amd.trainer import StepRunner

    monkeypatch.setattr(HF, "_dropout_counter", itertools.count(100))
    b = _batches(cuda)
    full = {"image": torch.cat([b[0]["image"], b[1]["image"]]), "mask": torch.cat([b[0]["mask"], b[1]["mask"]])}
    c = 0.1 * _first_norm(cuda, kind, full)
    net, opt = _net(cuda, kind)
    runner = StepRunner(net, opt, gradient_clip_val=c)
    for _ in range(3):
        runner.train_step(full)
    assert runner.optimizer_steps == 3 and runner.step_idx == 3
    assert runner.last_grad_norm is not None
    ours = _params_of(net)
    net, opt = _net(cuda, kind)
    sync = GradSync(opt)
    for s in range(3):
        norm = _reference_window(net, opt, sync, [full], 1, c, s)
    _assert_close(ours, _params_of(net))
    assert abs(float(runner.last_grad_norm) - float(norm)) <= 1e-4 * float(norm)


@pytest.mark.parametrize("clip", [False, True])
def test_accumulation_matches_divided_losses(cuda, clip, monkeypatch):
    from adell_mri_amd.parallel import GradSync
    from adell_mri_amd.trainer import StepRunner

    monkeypatch.setattr(HF, "_dropout_counter", itertools.count(100))
    b = _batches(cuda)
    c = None
    if clip:
        full = {"image": torch.cat([b[0]["image"], b[1]["image"]]), "mask": torch.cat([b[0]["mask"], b[1]["mask"]])}
        c = 0.1 * _first_norm(cuda, "sgd", full)
    net, opt = _net(cuda, "sgd")
    runner = StepRunner(net, opt, gradient_clip_val=c, accumulate_grad_batches=2)
    for _ in range(2):
        runner.train_step(b[0])
        runner.train_step(b[1])
    assert runner.step_idx == 4 and runner.optimizer_steps == 2
    assert all(g["grad_scale"] == 1.0 for g in opt.param_groups)        # restored
    ours = _params_of(net)
    net, opt = _net(cuda, "sgd")
    sync = GradSync(opt)
    for w in range(2):
        _reference_window(net, opt, sync, b, 2, c, 2 * w)
    _assert_close(ours, _params_of(net))


def test_flush_steps_a_partial_window_with_one_over_n(cuda, monkeypatch):
    from adell_mri_amd.parallel import GradSync
    from adell_mri_amd.trainer import StepRunner

    monkeypatch.setattr(HF, "_dropout_counter", itertools.count(100))
    b = _batches(cuda)
    net, opt = _net(cuda, "sgd")
    runner = StepRunner(net, opt, accumulate_grad_batches=3)
    runner.train_step(b[0])
    runner.train_step(b[1])
    assert runner.optimizer_steps == 0
    assert runner.flush() and runner.optimizer_steps == 1
    assert not runner.flush()
    ours = _params_of(net)
    net, opt = _net(cuda, "sgd")
    sync = GradSync(opt)
    opt.zero_grad()
    for k in range(2):
        (net.training_step(b[k], k) / 3).backward()
    sync.all_reduce()
    opt.step()
    _assert_close(ours, _params_of(net))


class _Toy(torch.nn.Module):
    """``a`` receives a gradient in the first micro-batch of a window only."""

    def __init__(self, cuda):
        super().__init__()
        self.a = torch.nn.Parameter(torch.full((8,), 2.0, device=cuda))
        self.b = torch.nn.Parameter(torch.full((8,), 3.0, device=cuda))

    def training_step(self, batch, idx):
        x = batch["x"]
        if idx % 2 == 0:
            return (self.a * x).sum() + (self.b * x).sum()
        return (self.b * x).sum()


def test_parameter_with_a_gradient_in_the_first_micro_batch_only_is_stepped(cuda):
    from adell_mri_amd.optim import FusedSGD
    from adell_mri_amd.trainer import fit_steps

    toy = _Toy(cuda)
    opt = FusedSGD(toy.parameters(), lr=0.5)
    x1 = torch.arange(8, dtype=torch.float32, device=cuda)
    x2 = torch.ones(8, device=cuda)
    fit_steps(toy, [{"x": x1}, {"x": x2}], opt, accumulate_grad_batches=2)
    torch.cuda.synchronize()
    assert torch.allclose(toy.a.detach(), 2.0 - 0.5 * x1 / 2)
    assert torch.allclose(toy.b.detach(), 3.0 - 0.5 * (x1 + x2) / 2)


def test_second_micro_batch_keeps_the_side_stream(cuda, monkeypatch):
    from adell_mri_amd.trainer import StepRunner

    monkeypatch.setitem(HF.FLAGS, "wgrad_stream", True)
    monkeypatch.setattr(HF, "_dropout_counter", itertools.count(100))
    calls = []
    real = HF.side_run
    monkeypatch.setattr(HF, "side_run", lambda fn, reads: calls.append(1) or real(fn, reads))
    b = _batches(cuda)
    net, opt = _net(cuda, "sgd")
    runner = StepRunner(net, opt, accumulate_grad_batches=2)
    runner.train_step(b[0])
    n1 = len(calls)
    runner.train_step(b[1])
    n2 = len(calls) - n1
    assert n1 >= 5 and n2 == n1, (n1, n2)


# ---- 7. graph mode ---------------------------------------------------------------------------------------
def test_enable_graph_refuses_accumulation_before_capture(cuda, monkeypatch):
    from adell_mri_amd.trainer import StepRunner

    net, opt = _net(cuda, "sgd")
    runner = StepRunner(net, opt, accumulate_grad_batches=2)

    def no_capture(*a, **k):
        raise AssertionError("a capture was started")

    monkeypatch.setattr(torch.cuda, "CUDAGraph", no_capture)
    with pytest.raises(RuntimeError, match="accumulate_grad_batches"):
        runner.enable_graph(_batches(cuda)[0])
    assert runner._graph is None and runner.step_idx == 0


# ---- 8. defaults launch nothing new ------------------------------------------------------------------------
def test_default_steps_do_not_touch_the_new_kernels(cuda, monkeypatch):
    from adell_mri_amd.trainer import StepRunner

    def boom(*a, **k):
        raise AssertionError("a clipping / accumulation kernel in a default step")

    for name in ("multi_accumulate", "grad_norm_workspace", "grad_norm_partials",
                 "grad_norm_finalize", "grad_scale_by"):
        monkeypatch.setattr(ops, name, boom)
    b = _batches(cuda)
    net, opt = _net(cuda, "sgd")
    runner = StepRunner(net, opt)
    for _ in range(2):
        runner.train_step(b[0])
    torch.cuda.synchronize()
    assert runner.optimizer_steps == 2 and runner.last_grad_norm is None
