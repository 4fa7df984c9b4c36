"""The elastic-weight-consolidation penalty on the GPU: kernel parity against fp64 at every path of
csrc/ewc.hip, the reference fixture, the cached tables, ``consolidate`` and the fused trainer route
against the autograd route. C below is the library's chunk length."""
import numpy as np
import pytest
import torch

import continual_cases as C
from adell_mri_amd import ops
from adell_mri_amd.modules.continuous_learning import ElasticWeightConsolidation, create_param_groups
from adell_mri_amd.optim import FusedAdamW, FusedSGD
from adell_mri_amd.trainer import StepRunner

pytestmark = pytest.mark.gpu

PEN_TOL = 2.0 ** -22      # fp32 differences (2^-24) + the final rounding (2^-24), doubled
UPSTREAM = 0.75           # the upstream gradient of the [1] output (reaches the kernel on the device)


def grad_tol(p):
    # the difference, the norm to the power p - 1 and the division: a few units of 2^-24 each
    return 2.0 ** -21 if p in (1, 2) else 2.0 ** -20


class Bag(torch.nn.Module):
    """Parameters under the given names; a tensor is wrapped as it is (views stay views)."""

    def __init__(self, tensors):
        super().__init__()
        for k, v in tensors.items():
            self.register_parameter(k, torch.nn.Parameter(v))


def fp64_reference(live, anchor, p, upstream=1.0):
    """Penalty and gradients in fp64 on the CPU from the same fp32 inputs (torch's masked forms)."""
    total, grads = 0.0, {}
    for k, v in live.items():
        d = v.astype(np.float64) - anchor[k].astype(np.float64)
        norm = float((np.abs(d) ** p).sum() ** (1.0 / p))
        total += norm
        g = np.zeros_like(d)
        nz = d != 0
        if norm > 0:
            g[nz] = upstream * np.sign(d[nz]) * np.abs(d[nz]) ** (p - 1) / norm ** (p - 1)
        grads[k] = g
    return total, grads


def run(ewc, model, upstream=1.0):
    for q in model.parameters():
        q.grad = None
    pen = ewc(model)
    assert pen.shape == (1,) and pen.dtype == torch.float32 and pen.is_cuda
    (upstream * pen).sum().backward()
    return pen.detach().clone(), {k: q.grad.detach().clone() for k, q in model.named_parameters()}


@pytest.fixture(scope="module")
def kernel_case(cuda):
    """One set of tensors that takes every path: sizes around the f32x4 width and the chunk length,
    several chunks, a parameter at a 4-byte offset into its storage, a tensor on its anchor and a
    tensor with one element on its anchor. Built once, shared by the p cases, never modified."""
    chunk = ops.ewc_chunk()
    sizes = {"n1": 1, "n3": 3, "n4": 4, "n5": 5, "cm1": chunk - 1, "c": chunk, "cp1": chunk + 1,
             "c2p7": 2 * chunk + 7, "offset": chunk + 6, "same": chunk + 3, "one_back": 2 * chunk + 1}
    anchor = {k: C.draw("k:anchor:" + k, (n,)) for k, n in sizes.items()}
    live = {k: (v + C.draw("k:move:" + k, v.shape, 0.05)).astype(np.float32) for k, v in anchor.items()}
    live["same"] = anchor["same"].copy()
    live["one_back"][chunk + 2] = anchor["one_back"][chunk + 2]
    tensors = {}
    for k, v in live.items():
        if k == "offset":
            base = torch.zeros(v.size + 1, device=cuda)
            base[1:] = torch.from_numpy(v).to(cuda)
            tensors[k] = base[1:]
        else:
            tensors[k] = torch.from_numpy(v).to(cuda)
    model = Bag(tensors)
    assert model.offset.data_ptr() % 16 == 4
    anchor_model = Bag({k: torch.from_numpy(v).to(cuda) for k, v in anchor.items()})
    return chunk, anchor, live, model, anchor_model


@pytest.mark.parametrize("p", C.PS)
def test_kernel_parity_against_fp64(kernel_case, p):
    chunk, anchor, live, model, anchor_model = kernel_case
    ewc = ElasticWeightConsolidation(anchor_model, p=p)
    assert ewc._anchor.is_cuda and ewc._anchor.data_ptr() % 16 == 0
    pen, grads = run(ewc, model, UPSTREAM)
    pen2, grads2 = run(ewc, model, UPSTREAM)
    want, want_g = fp64_reference(live, anchor, p, UPSTREAM)
    got = float(pen)
    print(f"p={p}: penalty {got!r} fp64 {want!r} rel {abs(got - want) / want:.3e} (bound {PEN_TOL:.3e})")
    assert np.isfinite(got) and abs(got - want) <= PEN_TOL * want
    for k, g in grads.items():
        g = g.cpu().numpy().astype(np.float64)
        assert g.shape == live[k].shape and np.isfinite(g).all(), k
        top = np.abs(want_g[k]).max()
        err = np.abs(g - want_g[k]).max()
        print(f"  {k:9s} max|g| {top:.4e} err/max {err / top if top else err:.3e} (bound {grad_tol(p):.3e})")
        assert err <= grad_tol(p) * top, k
    assert not grads["same"].any()                                   # exactly 0 (norm 0)
    assert grads["one_back"][chunk + 2] == 0                         # exactly 0 (d == 0), p < 2 included
    assert int(grads["one_back"].count_nonzero()) == np.count_nonzero(want_g["one_back"]) >= 2 * chunk - 8
    # fixed grids, fixed-order sums: the same bits again
    assert torch.equal(pen, pen2)
    assert all(torch.equal(grads[k], grads2[k]) for k in grads)
    assert ewc.table_rebuilds == 1
    assert all(a.grad is None for a in ewc.anchor_parameters.values())   # the anchor collects nothing


@pytest.mark.parametrize("p", C.PS)
def test_first_step_is_exactly_zero(cuda, p):
    model = C.Named({k: C.draw("first:" + k, s) for k, s in C.SHAPES.items()}).to(cuda)
    ewc = ElasticWeightConsolidation(model, p=p)
    pen, grads = run(ewc, model)
    assert float(pen) == 0.0
    for k, g in grads.items():
        assert g.shape == C.SHAPES[k] and not g.any(), k


@pytest.mark.parametrize("p", C.PS)
@pytest.mark.parametrize("state", C.STATES)
def test_matches_the_reference_fixture(cuda, p, state):
    gold = np.load(C.GOLD)
    key = f"{p}:{state}"
    ewc = ElasticWeightConsolidation(C.Named(C.anchors()).to(cuda), p=p)
    pen, grads = run(ewc, C.Named(C.state(state)).to(cuda))
    ref = float(gold["pen32:" + key][0])
    assert abs(float(pen) - ref) <= (float(gold["err_pen:" + key]) + 2.0 ** -22) * abs(ref)
    for k, g in grads.items():
        want = gold[f"g32:{key}:{k}"].astype(np.float64)
        err = np.abs(g.cpu().numpy().astype(np.float64) - want).max()
        assert err <= (float(gold[f"err_g:{key}:{k}"]) + 2.0 ** -21) * np.abs(want).max(), k


def _moved_linear_model(cuda, seed=3):
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(9, 7), torch.nn.ReLU(), torch.nn.Linear(7, 3)).to(cuda)
    return model


def _move(model, tag):
    with torch.no_grad():
        for k, q in model.named_parameters():
            q.add_(torch.from_numpy(C.draw(tag + k, tuple(q.shape), 0.03)).to(q.device))


def _host(model):
    return {k: q.detach().cpu().numpy() for k, q in model.named_parameters()}


def test_tables_follow_a_pointer_change(cuda):
    model = _moved_linear_model(cuda)
    ewc = ElasticWeightConsolidation(model)
    anchor = _host(model)
    assert float(ewc(model).detach()) == 0.0 and ewc.table_rebuilds == 1
    before = [q.data_ptr() for q in model.parameters()]
    FusedSGD(model.parameters(), lr=0.1)                     # re-homes p.data into one flat buffer
    assert before != [q.data_ptr() for q in model.parameters()]
    _move(model, "ptr:")
    pen = ewc(model)
    assert ewc.table_rebuilds == 2
    want, _ = fp64_reference(_host(model), anchor, 2)
    assert want > 0 and abs(float(pen.detach()) - want) <= PEN_TOL * want
    assert torch.equal(ewc(model), pen) and ewc.table_rebuilds == 2


def test_consolidate_re_anchors(cuda):
    model = _moved_linear_model(cuda)
    ewc = ElasticWeightConsolidation(model)
    _move(model, "cons:")
    assert float(ewc(model).detach()) > 0
    ewc.consolidate(model)
    pen, grads = run(ewc, model)
    assert float(pen) == 0.0 and all(not g.any() for g in grads.values())
    for k, q in model.named_parameters():
        assert torch.equal(ewc.anchor_parameters[k], q), k
    assert ewc.table_rebuilds == 1                            # same addresses: the tables were kept
    _move(model, "cons2:")
    assert float(ewc(model).detach()) > 0


# ---- the fused trainer route against the autograd route ----------------------------------------------
WEIGHT = 0.3


class Tiny(torch.nn.Module):
    """Two parameter groups of a few Linears and a parameter the loss does not use."""

    def __init__(self, width=1, bias=True):
        super().__init__()
        self.enc = torch.nn.Sequential(*[torch.nn.Linear(6, 6, bias=bias) for _ in range(width)])
        self.head = torch.nn.Linear(6, 3, bias=bias)
        self.unused = torch.nn.Parameter(torch.zeros(7))
        self.in_loss = None          # route A: [penalty module]; a list, so it is not a submodule
        self.penalties = []

    def training_step(self, batch, batch_idx):
        x, y = batch["x"], batch["y"]
        loss = ((self.head(torch.relu(self.enc(x))) - y) ** 2).mean()
        if self.in_loss is not None:
            pen = self.in_loss[0](self)
            self.penalties.append(pen.detach().clone())
            loss = loss + (WEIGHT * pen).reshape(())
        return loss


def _tiny(cuda, optimizer, width=1, bias=True):
    torch.manual_seed(11)
    module = Tiny(width, bias).to(cuda).train()
    with torch.no_grad():
        module.unused.copy_(torch.from_numpy(C.draw("tiny:unused", (7,))))
    ewc = ElasticWeightConsolidation(module)
    _move(module, "tiny:")
    groups = create_param_groups(module, ["enc."], [{"lr": 0.02}])
    if optimizer == "sgd":
        opt = FusedSGD(groups, lr=0.05, momentum=0.9, weight_decay=1e-3)
    else:
        opt = FusedAdamW(groups, lr=1e-2, weight_decay=1e-2)
    return module, ewc, opt


def _batches(cuda, n):
    return [{"x": torch.from_numpy(C.draw(f"tiny:x{i}", (5, 6))).to(cuda),
             "y": torch.from_numpy(C.draw(f"tiny:y{i}", (5, 3))).to(cuda)} for i in range(n)]


@pytest.mark.parametrize("optimizer", ["sgd", "adamw"])
@pytest.mark.parametrize("mode", ["plain", "accumulate", "clip"])
def test_fused_route_agrees_with_the_autograd_route(cuda, optimizer, mode):
    kw = {"plain": {}, "accumulate": {"accumulate_grad_batches": 2}, "clip": {"gradient_clip_val": 0.05}}[mode]
    n = kw.get("accumulate_grad_batches", 1)
    batches = _batches(cuda, 2 * n)                       # two optimiser steps
    a, ewc_a, opt_a = _tiny(cuda, optimizer)
    a.in_loss = [ewc_a]
    run_a = StepRunner(a, opt_a, **kw)
    loss_a = [run_a.train_step(b).detach() for b in batches]
    b, ewc_b, opt_b = _tiny(cuda, optimizer)
    start = _host(b)
    run_b = StepRunner(b, opt_b, ewc=ewc_b, ewc_weight=WEIGHT, **kw)
    loss_b, pens_b = [], []
    for batch in batches:
        loss_b.append(run_b.train_step(batch).detach())
        pens_b.append(run_b.last_ewc_penalty)
    assert run_a.optimizer_steps == run_b.optimizer_steps == 2
    if mode == "clip":                                    # low enough to clip, on both routes
        assert float(run_a.last_grad_norm) > 0.05 and float(run_b.last_grad_norm) > 0.05
    pa, pb = _host(a), _host(b)
    for k in pa:
        top = np.abs(pa[k]).max()
        err = np.abs(pa[k].astype(np.float64) - pb[k]).max()
        print(f"{optimizer} {mode} {k}: err/max {err / top:.3e} (bound {2.0 ** -20:.3e})")
        assert err <= 2.0 ** -20 * top, k
    assert np.abs(pb["unused"] - start["unused"]).max() > 1e-4      # stepped by the penalty alone
    # ... and moved identically: its only gradient is the penalty's, WEIGHT * g on route A (2 WEIGHT g / 2
    # under accumulation, exact) and (WEIGHT / grad_scale) g grad_scale on route B, from its own norm
    # (clip: the coefficient comes from the norm over ALL tensors; without accumulation every gradient
    # here is one fp32 addition of the task and the penalty gradient on both routes -- the kernel rounds
    # g before it adds --, so the norm and the coefficient have the same bits as well)
    assert np.array_equal(pa["unused"], pb["unused"])
    # the first optimiser step starts from identical weights: the same penalty bit for bit
    first = n - 1
    assert pens_b[first].shape == (1,) and float(pens_b[first]) > 0
    assert torch.equal(pens_b[first], a.penalties[first])
    assert pens_b[0] is None or first == 0                # no penalty before the window's step
    # the returned loss includes the penalty (route A's loss is task + WEIGHT * penalty)
    assert abs(float(loss_b[first]) - float(loss_a[first])) <= 2.0 ** -22 * abs(float(loss_a[first]))
    assert float(loss_b[first]) > WEIGHT * float(pens_b[first]) > 0


def test_fused_route_launch_count_does_not_grow_with_the_model(cuda, monkeypatch):
    calls = []
    for name in ("ewc_partials", "ewc_finalize", "ewc_grad"):
        def counted(*args, _fn=getattr(ops, name), _name=name):
            calls.append(_name)
            return _fn(*args)
        monkeypatch.setattr(ops, name, counted)
    counts = {}
    for width in (1, 38):                                 # 3 and 40 parameter tensors
        module, ewc, opt = _tiny(cuda, "sgd", width, bias=False)
        assert len(list(module.parameters())) == width + 2
        runner = StepRunner(module, opt, ewc=ewc, ewc_weight=WEIGHT)
        runner.train_step(_batches(cuda, 1)[0])           # builds and uploads the tables
        del calls[:]
        runner.train_step(_batches(cuda, 1)[0])
        counts[width] = list(calls)
    assert counts[1] == counts[38]
    assert len(counts[1]) <= 2 + len(opt.param_groups)
    assert counts[1].count("ewc_grad") == len(opt.param_groups) == 2


def test_parameter_frozen_after_the_optimiser_was_built_is_value_only(cuda):
    module, ewc, opt = _tiny(cuda, "sgd")
    runner = StepRunner(module, opt, ewc=ewc, ewc_weight=WEIGHT)
    module.unused.requires_grad_(False)
    before = _host(module)
    anchor = {k: a.detach().cpu().numpy() for k, a in ewc.anchor_parameters.items()}
    runner.train_step(_batches(cuda, 1)[0])
    after = _host(module)
    assert np.array_equal(after["unused"], before["unused"]) and module.unused.grad is None
    assert not np.array_equal(after["head.weight"], before["head.weight"])
    want, _ = fp64_reference(before, anchor, 2)                 # the value still counts it
    assert abs(float(runner.last_ewc_penalty) - want) <= PEN_TOL * want
    module.unused.requires_grad_(True)                          # thawed: stepped by the penalty again
    runner.train_step(_batches(cuda, 1)[0])
    assert not np.array_equal(_host(module)["unused"], before["unused"])


def test_in_place_change_between_forward_and_backward_raises(cuda):
    model = _moved_linear_model(cuda)
    ewc = ElasticWeightConsolidation(model)
    _move(model, "ver:")
    pen = ewc(model)
    _move(model, "ver2:")
    with pytest.raises(RuntimeError, match="modified in place"):
        pen.sum().backward()


def test_step_runner_refuses_a_foreign_penalty(cuda):
    module, ewc, opt = _tiny(cuda, "sgd")
    other = ElasticWeightConsolidation(torch.nn.Linear(6, 6).to(cuda))
    with pytest.raises(ValueError, match="not the module's"):
        StepRunner(module, opt, ewc=other)
    with pytest.raises(TypeError, match="fused optimiser"):
        StepRunner(module, torch.optim.SGD(module.parameters(), lr=0.1), ewc=ewc)
