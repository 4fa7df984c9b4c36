"""Multiple-instance classification on the GPU: the kernels of csrc/mil.hip against the fp64
restatements (tests/mil_ref.py, pinned to the reference by tests/test_mil.py), every kernel result
computed twice and compared bit for bit; one training step and a following validation step of the six
fixture networks against the real reference (tests/golden/mil_step_*.npz).

Tolerances are the project's for the same kinds of quantity (tests/test_classification_gpu.py): bit
equality for copies (the slicing both ways, the token rows and their dx), ``SUM_BOUND`` = 5e-5 of the
largest reference magnitude for fixed-order sums; in the step tests loss 1e-4, gradients 5e-3 by
``cases.grad_rel_err``, parameters (2e-4, 2e-6) -- the fixtures' own fp32-against-fp64 error uses at
most a quarter of them (asserted by tools/make_mil_golden.py, recorded as ``fp32_vs_fp64``). ``db`` is
mathematically zero (softmax is shift-invariant): it is a sum of the dscore terms, so it is held to
``SUM_BOUND`` of the largest |dscore| of the reference."""
import numpy as np
import pytest
import torch

import mil_ref as MR
from cases import grad_rel_err
from mil_cases import CONFIGS, NETS, SHAPE, StepGold, fill, set_step_mode
from test_mil import build_pl

pytestmark = pytest.mark.gpu

SUM_BOUND = 5e-5
MODES = ("mean", "max", "vocabulary")


def rel(a, r):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a).double()
    r = r.detach().double().cpu() if isinstance(r, torch.Tensor) else torch.as_tensor(r).double()
    assert a.shape == r.shape, (a.shape, r.shape)
    return float((a - r).abs().max() / (r.abs().max() + 1e-300))


def twice(fn):
    """fn() run two times: the first result, after asserting that the second is bit-identical."""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            assert torch.equal(u, v), "two runs differ"
    return a


# ---- volume to slices ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (2, 3, 5, 7, 3), (1, 2, 5, 13, 8),
                                   (2, 1, 16, 16, 65)])
def test_volume_to_slices_is_torchs_copy(cuda, shape):
    from adell_mri_amd import functional as HF

    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(shape, generator=g).to(cuda)
    dy = torch.randn((shape[0] * shape[4],) + shape[1:4], generator=g).to(cuda)

    def run():
        xd = x.clone().requires_grad_(True)
        y = HF.volume_to_slices(xd)
        y.backward(dy)
        return y.detach(), xd.grad

    y, dx = twice(run)
    B, C, H, W, S = shape
    want = x.permute(0, 4, 1, 2, 3).contiguous().view(B * S, C, H, W)
    assert y.shape == want.shape and y.is_contiguous() and torch.equal(y, want)
    assert torch.equal(y[(B - 1) * S + S - 1], x[B - 1, ..., S - 1])
    want_dx = dy.view(B, S, C, H, W).permute(0, 2, 3, 4, 1).contiguous()
    assert dx.shape == x.shape and dx.is_contiguous() and torch.equal(dx, want_dx)
    assert np.array_equal(y.cpu().numpy(), MR.volume_to_slices(x.cpu().numpy()))


def test_volume_to_slices_refuses_a_non_dense_input(cuda):
    from adell_mri_amd import _lib
    from adell_mri_amd import functional as HF

    x = torch.randn((2, 3, 5, 7, 6), device=cuda)
    for view in (x[..., ::2], x.permute(0, 1, 3, 2, 4), x[:, :, :, 1:]):
        assert not view.is_contiguous()
        with pytest.raises(_lib.AdellHipError, match="non-dense"):
            HF.volume_to_slices(view)
    with pytest.raises(_lib.AdellHipError):
        HF.volume_to_slices(x.cpu())


# ---- attention and pooling -----------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1, 1), (3, 5, 33, 130), (2, 8, 32, 16), (1, 65, 7, 3)]
POOL_SEEDS = {(1, 1, 1, 1): 1, (3, 5, 33, 130): 2, (2, 8, 32, 16): 3, (1, 65, 7, 3): 4}


def pool_inputs(shape, seed=None):
    """fp32 inputs of one case (CPU tensors): feat, hv, hu, w, b and the incoming gradients."""
    B, S, N, F = shape
    g = torch.Generator().manual_seed(POOL_SEEDS[shape] if seed is None else seed)
    feat = torch.randn((B, S, F), generator=g)
    hv, hu = torch.randn((B, S, N), generator=g) * 1.5, torch.randn((B, S, N), generator=g) * 2.0
    w, b = torch.randn((N,), generator=g), torch.randn((1,), generator=g)
    gp = torch.randn((B, F), generator=g) * 0.7 + 0.3
    gA = torch.randn((B, S, 1), generator=g) * 1.3 - 0.2
    return feat, hv, hu, w, b, gp, gA


def run_pool(cuda, mode, feat, gate, gp, gA):
    """(pooled, A, dfeat, dhv, dhu, dw, db) of one forward and backward on the device."""
    from adell_mri_amd import functional as HF

    leaves = [t.to(cuda).requires_grad_(True) for t in (feat,) + tuple(gate)]
    pooled, A = HF.mil_gated_pool(*leaves, mode=mode)
    loss = (pooled * gp.to(cuda)).sum()
    if gA is not None:
        loss = loss + (A * gA.to(cuda)).sum()
    loss.backward()
    grads = [t.grad for t in leaves] + [None] * (5 - len(leaves))
    return (pooled.detach(), A.detach(), *grads)


@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", POOL_SHAPES)
def test_gated_pool_matches_the_restatement(cuda, shape, mode, gated):
    feat, hv, hu, w, b, gp, gA = pool_inputs(shape)
    gate = (hv, hu, w, b) if gated else ()
    gate_np = [t.numpy() for t in gate] if gated else [None] * 4
    want_pooled, want_A, want_arg = MR.gated_pool(feat.numpy(), *gate_np, mode=mode)
    if mode == "max" and shape[1] > 1:
        # the arg-max must be decided by more than rounding: the two largest fp64 products of
        # every (b, f) differ by more than 1e-4 of the larger (the seeds are chosen for it)
        top = np.sort(MR.products(feat.numpy(), want_A, mode), axis=1)
        assert np.all(top[:, -1] - top[:, -2] > 1e-4 * np.abs(top[:, -1])), "pick another seed"
    pooled, A, dfeat, dhv, dhu, dw, db = twice(
        lambda: run_pool(cuda, mode, feat, gate, gp, gA if gated else None))
    assert pooled.shape == (shape[0], shape[3]) and A.shape == (shape[0], shape[1], 1)
    assert rel(pooled, want_pooled) < SUM_BOUND and rel(A, want_A) < SUM_BOUND
    want = MR.gated_pool_bwd(feat.numpy(), *gate_np, mode, gp.numpy(), gA.numpy() if gated else None)
    assert rel(dfeat, want["dfeat"]) < SUM_BOUND
    if mode == "max":
        from adell_mri_amd import ops

        _, _, arg = twice(lambda: ops.mil_pool_fwd(mode, feat.to(cuda), *[t.to(cuda) for t in gate]))
        assert arg.dtype == torch.int32 and np.array_equal(arg.cpu().numpy(), want_arg)
    if not gated:
        assert torch.equal(A, torch.full_like(A, 1.0 / shape[1]))
        return
    assert rel(dhv, want["dhv"]) < SUM_BOUND and rel(dhu, want["dhu"]) < SUM_BOUND
    assert dw.shape == w.shape and rel(dw, want["dw"]) < SUM_BOUND
    # db: the fixed-order sum of dscore, zero but for rounding (see the module docstring)
    assert db.shape == (1,)
    assert abs(float(db) - float(want["db"][0])) <= SUM_BOUND * np.abs(want["dscore"]).max()


@pytest.mark.parametrize("mode", MODES)
def test_gradient_on_A_alone_reaches_the_gate(cuda, mode):
    """A gradient that arrives on A alone (``return_attention=True`` exposes it) reaches the gate."""
    from adell_mri_amd import functional as HF

    shape = (3, 5, 33, 130)
    feat, hv, hu, w, b, gp, gA = pool_inputs(shape)

    def run():
        leaves = [t.to(cuda).requires_grad_(True) for t in (feat, hv, hu, w, b)]
        _, A = HF.mil_gated_pool(*leaves, mode=mode)
        (A * gA.to(cuda)).sum().backward()
        return (A.detach(),) + tuple(t.grad for t in leaves)

    A, dfeat, dhv, dhu, dw, _ = twice(run)
    want = MR.gated_pool_bwd(feat.numpy(), hv.numpy(), hu.numpy(), w.numpy(), b.numpy(), mode,
                             np.zeros(gp.shape), gA.numpy())
    assert float(dfeat.abs().max()) == 0.0
    assert rel(dhv, want["dhv"]) < SUM_BOUND and rel(dhu, want["dhu"]) < SUM_BOUND
    assert rel(dw, want["dw"]) < SUM_BOUND
    # calculate_attention's entry point is the same kernel
    (A2,) = twice(lambda: (HF.mil_attention(*[t.to(cuda) for t in (hv, hu, w, b)]),))
    assert torch.equal(A2, A)


@pytest.mark.parametrize("mode", MODES)
def test_gated_pool_stays_finite_at_extreme_gate_inputs(cuda, mode):
    """Scores of +-200 (a softmax without max-subtraction overflows) and hv = +-50, hu = +-100 (a
    naive sigmoid or tanh overflows): every result is finite, and A is still a distribution."""
    shape = (3, 5, 33, 130)
    feat, hv, hu, w, b, gp, gA = pool_inputs(shape)
    hv[:, ::2], hv[:, 1::2] = 50.0, -50.0
    hu[0], hu[1], hu[2, :, ::2] = 100.0, -100.0, 100.0
    hu[1, 0] = 100.0
    _, gate = MR.attention(hv.numpy(), hu.numpy(), np.ones(shape[2]), np.zeros(1))
    w = torch.full((shape[2],), 1.0)
    score = gate @ w.double().numpy()
    w = w * float(200.0 / np.abs(score).max())
    score = gate @ w.double().numpy()
    assert score.max() > 199.0 and score.min() < -199.0
    out = twice(lambda: run_pool(cuda, mode, feat, (hv, hu, w, b), gp, gA))
    for t in out:
        assert bool(torch.isfinite(t).all())
    A = out[1]
    assert rel(A.sum(1), torch.ones((shape[0], 1))) < SUM_BOUND
    want_pooled, want_A, _ = MR.gated_pool(feat.numpy(), hv.numpy(), hu.numpy(), w.numpy(),
                                           b.numpy(), mode)
    assert rel(A, want_A) < 1e-3 and rel(out[0], want_pooled) < 1e-3   # scores of 200 carry 1e-5


@pytest.mark.parametrize("gated", [True, False])
def test_max_mode_exact_tie_takes_the_lowest_slice(cuda, gated):
    from adell_mri_amd import ops

    shape = (2, 8, 32, 16)
    feat, hv, hu, w, b, gp, gA = pool_inputs(shape)
    feat = -feat.abs() - 0.1        # every other product is negative (A > 0), the tied ones lead
    feat[:, 1] = feat[:, 1].abs() + 5.0
    for t in (feat, hv, hu):
        t[:, 5] = t[:, 1]           # two slices with identical rows: identical scores, A, products
    gate = [t.to(cuda) for t in (hv, hu, w, b)] if gated else []
    pooled, A, arg = twice(lambda: ops.mil_pool_fwd("max", feat.to(cuda), *gate))
    assert torch.equal(A[:, 1], A[:, 5])
    assert bool((arg == 1).all()), arg
    assert torch.equal(pooled, feat.to(cuda)[:, 1] * A[:, 1])
    out = twice(lambda: run_pool(cuda, "max", feat, (hv, hu, w, b) if gated else (), gp, None))
    assert float(out[2][:, 5].abs().max()) == 0.0 and float(out[2][:, 1].abs().min()) > 0.0
    # a NaN propagates as in torch.max
    feat[0, 3, 2] = float("nan")
    pooled, _, arg = ops.mil_pool_fwd("max", feat.to(cuda), *gate)
    again = ops.mil_pool_fwd("max", feat.to(cuda), *gate)
    assert torch.equal(arg, again[2]) and torch.equal(torch.isnan(pooled), torch.isnan(again[0]))
    assert torch.equal(torch.nan_to_num(pooled), torch.nan_to_num(again[0]))
    assert bool(torch.isnan(pooled[0, 2])) and int(arg[0, 2]) == 3
    assert int(torch.isnan(pooled).sum()) == 1


# ---- slice tokens --------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_class_token", [True, False])
@pytest.mark.parametrize("with_pos", [True, False])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 33), (2, 65, 130)])
def test_slice_tokens(cuda, shape, with_pos, with_class_token):
    from adell_mri_amd import functional as HF

    B, S, E = shape
    g = torch.Generator().manual_seed(B + S + E)
    x = torch.randn(shape, generator=g).to(cuda)
    pos = (torch.randn((1, S, 1), generator=g) * 0.5).to(cuda) if with_pos else None
    ct = torch.randn((1, 1, E), generator=g).to(cuda) if with_class_token else None
    dout = torch.randn((B, S + int(with_class_token), E), generator=g).to(cuda)

    def run():
        leaves = [None if t is None else t.clone().requires_grad_(True) for t in (x, pos, ct)]
        out = HF.slice_tokens(*leaves)
        out.backward(dout)
        return (out.detach(),) + tuple(None if t is None else t.grad for t in leaves)

    out, dx, dpos, dct = twice(run)
    want = x + pos if with_pos else x
    if with_class_token:
        want = torch.cat([ct.expand(B, 1, E), want], 1)
    assert out.shape == want.shape and out.is_contiguous() and torch.equal(out, want)
    assert np.array_equal(out.cpu().numpy(), MR.slice_tokens(
        x.cpu().numpy(), None if pos is None else pos.cpu().numpy(),
        None if ct is None else ct.cpu().numpy()))
    want_dx, want_dpos, want_dct = MR.slice_tokens_bwd(dout.cpu().numpy(), with_class_token)
    assert dx.is_contiguous() and torch.equal(dx, dout[:, int(with_class_token):])
    if with_pos:
        assert dpos.shape == (1, S, 1) and rel(dpos, want_dpos) < SUM_BOUND
    if with_class_token:
        assert dct.shape == (1, 1, E) and rel(dct, want_dct) < SUM_BOUND


# ---- one training step -----------------------------------------------------------------------------------
def build_step(name, cuda):
    """The wrapper of one fixture network with the fixture's weights on the device, in ``train()``
    mode (the 2-D module in ``eval()`` mode) with every dropout rate zeroed, and its batch."""
    g = StepGold(name)
    net, _ = build_pl(name)
    net.load_state_dict(fill(net.state_dict(), float(g["gain"])))
    net = set_step_mode(net.to(cuda))
    batch = {"image": torch.from_numpy(g["x"]).to(cuda), "label": torch.from_numpy(g["y"]).to(cuda)}
    return net, g, batch


@pytest.mark.parametrize("name", NETS)
def test_training_step_matches_reference(cuda, name):
    """``training_step`` through ``StepRunner``: logits, loss, every parameter gradient, one
    FusedAdamW step over the groups of ``configure_optimizers`` (the frozen module outside them and
    bit-unchanged), then ``validate_steps``; ``return_attention=True`` gives the recorded A /
    attention."""
    from adell_mri_amd.optim import FusedAdamW
    from adell_mri_amd.trainer import StepRunner, validate_steps

    net, g, batch = build_step(name, cuda)
    trains = CONFIGS[name][4]
    runner = StepRunner(net)
    assert isinstance(runner.optimizer, FusedAdamW)
    assert [len(gr["params"]) for gr in runner.optimizer.param_groups] == [
        len(g[f"groups:{i}:names"]) for i in range(int(g["groups:n"]))]
    in_optimizer = {id(p) for gr in runner.optimizer.param_groups for p in gr["params"]}
    module_params = list(net.module.named_parameters())
    assert all((id(p) in in_optimizer) == trains for _, p in module_params)
    before = {k: v.detach().clone() for k, v in net.module.state_dict().items()}

    with torch.no_grad():
        out, attention = net.predict_step(batch, 0, return_attention=True).values()
    assert attention.shape == g["attention"].shape and rel(attention, g["attention"]) < SUM_BOUND
    assert rel(torch.squeeze(out, 1), g["logits"]) < 1e-4

    runner.optimizer.zero_grad()
    loss = net.training_step(batch, 0)
    np.testing.assert_allclose(loss.item(), g["total"], rtol=1e-4)
    loss.backward()
    trainable = [(k, p) for k, p in net.named_parameters() if p.requires_grad]
    assert sum(k.startswith("grad:") for k in g.files) == len(trainable)
    worst = 0.0
    for k, p in trainable:
        assert p.grad is not None, k
        e = grad_rel_err(g, k, p.grad.cpu().numpy())
        worst = max(worst, e)
        assert e < 5e-3, (k, e)
    for k, p in module_params:
        assert (p.grad is not None) == trains, k
    print(f"{name}: loss {abs(loss.item() - g['total']) / g['total']:.2e}, worst gradient "
          f"{worst:.2e}")
    runner.optimizer.step()
    for k, v in net.state_dict().items():
        if v.is_floating_point():
            np.testing.assert_allclose(v.detach().cpu().numpy(), g["step1:" + k], rtol=2e-4,
                                       atol=2e-6, err_msg=k)
        else:
            assert np.array_equal(v.cpu().numpy(), g["step1:" + k]), k
    if not trains:
        for k, v in net.module.state_dict().items():
            assert torch.equal(v, before[k]), k
    else:
        assert any(not torch.equal(v, before[k]) for k, v in net.module.state_dict().items())
    out = validate_steps(net, [batch])
    np.testing.assert_allclose(out["val_loss"], g["val_total"], rtol=1e-4)
    assert net.training
    assert sorted(out) == sorted(["val_loss"] + list(net.val_metrics))
    assert all(np.isfinite(v) or np.isnan(v) for v in out.values())


# ---- modules -------------------------------------------------------------------------------------------
def test_mil_attention_module(cuda):
    """``calculate_attention`` and ``forward`` (``X * attention``) against the module's own weights in
    fp64, with gradients into V, U, W and X."""
    from adell_mri_amd.modules.classification import MILAttention

    torch.manual_seed(5)
    att = MILAttention(33).to(cuda)
    X = torch.randn((3, 5, 33), device=cuda, requires_grad=True)
    ref = MILAttention(33).double()
    ref.load_state_dict({k: v.detach().cpu().double() for k, v in att.state_dict().items()})
    Xr = X.detach().cpu().double().requires_grad_(True)
    Ar = torch.softmax(torch.nn.functional.linear(
        torch.tanh(torch.nn.functional.linear(Xr, ref.V.weight, ref.V.bias)) *
        torch.sigmoid(torch.nn.functional.linear(Xr, ref.U.weight, ref.U.bias)),
        ref.W.weight, ref.W.bias), -2)
    A = att.calculate_attention(X)
    assert A.shape == (3, 5, 1) and rel(A, Ar) < SUM_BOUND
    out = att(X)
    assert out.shape == X.shape and rel(out, Xr * Ar) < SUM_BOUND
    g = torch.linspace(-1.0, 2.0, X.numel()).reshape(X.shape)
    (out * g.to(cuda)).sum().backward()
    (Xr * Ar * g.double()).sum().backward()
    assert rel(X.grad, Xr.grad) < 1e-4
    for k, p in att.named_parameters():
        if k != "W.bias":           # mathematically zero
            assert rel(p.grad, dict(ref.named_parameters())[k].grad) < 1e-4, k


@pytest.mark.parametrize("reduce_fn", ["mean", "max"])
def test_extract_features_and_flat_module_output(cuda, reduce_fn):
    """[N, V, h, w] -> [N, V] by the mean or the maximum; a module that returns [B * S, V] is reduced
    over V itself as in the reference, and ``v_module`` then raises naming ``module``."""
    from adell_mri_amd.modules.classification import MultipleInstanceClassifier

    class Flat(torch.nn.Module):
        def forward(self, X):
            return X.flatten(1)[:, :6].contiguous()

    net = MultipleInstanceClassifier(Flat(), 6, 2, [], [4], n_slices=3, reduce_fn=reduce_fn).to(cuda)
    x = torch.randn((6, 5, 3, 4), device=cuda)
    want = x.flatten(2).mean(-1) if reduce_fn == "mean" else x.flatten(2).max(-1).values
    got = net.extract_features(x)
    assert got.shape == (6, 5) and rel(got, want) < SUM_BOUND
    flat = torch.randn((6, 7), device=cuda)
    want = flat.mean(-1) if reduce_fn == "mean" else flat.max(-1).values
    got = net.extract_features(flat)
    assert got.shape == (6,) and rel(got, want) < SUM_BOUND
    with pytest.raises(ValueError, match="module"):
        net(torch.randn((2, 1, 4, 4, 3), device=cuda))
