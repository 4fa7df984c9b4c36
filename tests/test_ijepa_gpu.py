"""I-JEPA on the GPU: the row kernels of csrc/ijepa.hip against the fp64 restatement
(tests/ijepa_ref.py), every result computed twice and compared bit for bit; one transformer block at
the sequence lengths the context and predictor passes produce; one training step and a following
validation step of both fixture networks against the real reference (tests/golden/ijepa_step*.npz)."""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ijepa_ref as JR
from cases import grad_rel_err
from ijepa_cases import NETS, StepGold, step_config
from oracle.weights import fill_state_dict

pytestmark = pytest.mark.gpu


def rel(a, r):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a).double()
    r = r.detach().double().cpu() if isinstance(r, torch.Tensor) else torch.as_tensor(r).double()
    return float((a - r).abs().max() / (r.abs().max() + 1e-300))


def uniform(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def twice(fn):
    """fn() run two times: the first result, after asserting that the second is bit-identical."""
    a, b = fn(), fn()
    a_, b_ = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    assert all(torch.equal(u, v) for u, v in zip(a_, b_)), "two runs differ"
    return a


# ---- gather ----------------------------------------------------------------------------------------
def _gather_rows(N, M, kind):
    if kind == "all":
        return np.arange(N)
    if kind == "offset":        # rows offset by 3 (class token + registers), the last row among them
        return np.unique(np.concatenate([3 + np.arange(M - 1) * 2, [N - 1]]))
    if kind == "tail":          # x[:, -M:]
        return np.arange(N - M, N)
    return np.unique(np.linspace(0, N - 1, M).astype(np.int64))


@pytest.mark.parametrize("B,N,E,M,kind", [(1, 1, 1, 1, "spread"), (3, 7, 5, 3, "spread"),
                                          (2, 67, 64, 67, "all"), (3, 19, 250, 6, "offset"),
                                          (2, 9, 770, 2, "spread"), (2, 18, 32, 6, "tail")])
def test_gather_tokens(cuda, B, N, E, M, kind):
    from adell_mri_amd import functional as HF

    rows = _gather_rows(N, M, kind)
    assert len(rows) == M and int(rows.max()) < N
    if kind in ("offset", "tail"):
        assert N - 1 in rows
    x = uniform((B, N, E), 1)
    r = uniform((B, M, E), 2)

    def run():
        xd = x.to(cuda).requires_grad_(True)
        y = HF.gather_tokens(xd, rows)
        y.backward(r.to(cuda))
        return y.detach(), xd.grad

    y, dx = twice(run)
    assert torch.equal(y.cpu(), x[:, rows])
    want = torch.zeros_like(x)
    want[:, rows] = r
    assert torch.equal(dx.cpu(), want)         # zeros included: the whole gradient is written


def test_gather_refuses_a_row_beyond_the_sequence_on_the_host(cuda, monkeypatch):
    from adell_mri_amd import functional as HF, ops

    launched = []
    real = ops.ijepa_gather_fwd
    monkeypatch.setattr(ops, "ijepa_gather_fwd", lambda *a: launched.append(1) or real(*a))
    x = torch.zeros((2, 9, 8), device=cuda)
    with pytest.raises(IndexError, match="index 9 is out of bounds for a sequence of 9 tokens"):
        HF.gather_tokens(x, [0, 4, 9])
    with pytest.raises(IndexError, match="index -1 is out of bounds"):
        HF.gather_tokens(x, [-1, 4])
    assert launched == []                      # raised on the host, before any launch
    assert HF.gather_tokens(x, [0, 4, 8]).shape == (2, 3, 8) and launched == [1]


# ---- predictor input ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B,nc,nt,T,P", [(1, 1, 1, 2, 1), (3, 4, 7, 96, 32), (2, 12, 6, 64, 30),
                                         (2, 10, 3, 64, 260)])
def test_predictor_tokens(cuda, B, nc, nt, T, P):
    from adell_mri_amd import functional as HF

    rng = np.random.default_rng(B * 1000 + T)
    both = np.sort(rng.choice(T, nc + nt, replace=False))
    ctx = both[np.sort(rng.choice(nc + nt, nc, replace=False))]
    tgt = np.setdiff1d(both, ctx)
    e, pos, mask = uniform((B, nc, P), 3), uniform((1, T, P), 4, 0, 1), uniform((1, 1, P), 5, 0, 1)
    r = uniform((B, nc + nt, P), 6)

    def run():
        leaves = [t.to(cuda).requires_grad_(True) for t in (e, pos, mask)]
        out = HF.predictor_tokens(*leaves, ctx, tgt)
        out.backward(r.to(cuda))
        return (out.detach(), *[t.grad for t in leaves])

    out, de, dpos, dmask = twice(run)
    ref = [t.double().requires_grad_(True) for t in (e, pos, mask)]
    want = JR.predictor_input(*ref, ctx, tgt)
    (want * r.double()).sum().backward()
    assert out.shape == want.shape
    assert torch.equal(out.cpu(), want.detach().float())       # one add per element: exact
    assert torch.equal(de.cpu(), ref[0].grad.float())
    assert dpos.shape == pos.shape and dmask.shape == mask.shape
    assert rel(dpos, ref[1].grad) < 5e-5 and rel(dmask, ref[2].grad) < 5e-5
    outside = np.setdiff1d(np.arange(T), both)
    assert float(dpos[:, outside].abs().max()) == 0.0 if len(outside) else True


# ---- block loss --------------------------------------------------------------------------------------
# (B, nt, N, E, first row, seed)
LOSS_CASES = [(1, 1, 1, 1, 0, 1), (3, 7, 99, 32, 3, 1), (2, 6, 64, 64, 0, 1), (2, 3, 20, 250, 0, 1),
              (2, 2, 9, 770, 0, 1)]


def loss_inputs(case):
    """h uniform in [-1, 1] times a per-row scale in [0.5, 4], pred uniform in [-2, 2]."""
    B, nt, N, E, first, seed = case
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    rows = first + np.sort(rng.choice(N - first, nt, replace=False))
    if nt > 1:
        rows[-1] = N - 1
    h = (torch.rand((B, N, E), generator=g) * 2 - 1) * (0.5 + 3.5 * torch.rand((B, N, 1), generator=g))
    pred = torch.rand((B, nt, E), generator=g) * 4 - 2
    return pred, h, rows


@functools.lru_cache(maxsize=None)
def loss_reference(case):
    """(fp64 loss, fp64 dpred, fraction of |d| < 1, the fp32 CPU composition's relative errors)."""
    pred, h, rows = loss_inputs(case)
    pd = pred.double().requires_grad_(True)
    loss = JR.block_loss(pd, h, rows)
    loss.backward()
    d = pd.detach() - JR.targets(h, [rows])[0]
    p32 = pred.clone().requires_grad_(True)
    l32 = torch.nn.SmoothL1Loss()(p32, F.layer_norm(h, (h.shape[-1],))[:, rows])
    l32.backward()
    e_loss = abs(l32.item() - loss.item()) / abs(loss.item())
    return loss.detach(), pd.grad, float((d.abs() < 1).double().mean()), (e_loss, rel(p32.grad, pd.grad))


@pytest.mark.parametrize("case", LOSS_CASES, ids=lambda c: "-".join(str(v) for v in c[:5]))
def test_block_loss(cuda, case):
    """Loss rtol 1e-5, dpred within 5e-5 of its largest entry (the DINO and iBOT loss bounds); a bound
    gives way to four times the error of the fp32 torch composition on the CPU where that exceeds a
    quarter of it. Measured composition errors (loss, dpred) at the five shapes: 1.8e-8 / 0 at
    (1, 1, 1, 1); 3.9e-8 / 1.9e-7 at (3, 7, 99, 32); 2.9e-8 / 2.3e-7 at (2, 6, 64, 64); 2.4e-8 /
    2.3e-7 at (2, 3, 20, 250); 3.9e-8 / 2.2e-7 at (2, 2, 9, 770) -- no bound is replaced. With seed
    1 the share of elements with |d| < 1 is 0.44 to 0.46 at the four shapes wider than one feature."""
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.self_supervised.pl import IJEPAPL

    B, nt, N, E, first, _ = case
    pred, h, rows = loss_inputs(case)
    want, want_d, inner, (e_loss, e_d) = loss_reference(case)
    if E > 1:       # both branches of the smooth-L1 carry at least 10 % of the elements
        assert 0.1 <= inner <= 0.9, inner
        assert int(rows.min()) >= first and int(rows.max()) == N - 1
    else:
        assert float(JR.targets(h, [rows])[0].abs().max()) == 0.0     # layer norm of one feature
    print(f"{case}: |d| < 1 on {inner:.3f}; fp32 CPU composition: loss {e_loss:.2e}, dpred {e_d:.2e}")
    bar_loss = 1e-5 if e_loss <= 0.25 * 1e-5 else 4 * e_loss
    bar_d = 5e-5 if e_d <= 0.25 * 5e-5 else 4 * e_d
    hd = h.to(cuda)

    def run():
        pd = pred.to(cuda).requires_grad_(True)
        loss = HF.ijepa_block_loss(pd, hd, rows)
        (loss * 1.5).backward()
        return loss.detach(), pd.grad

    loss, dpred = twice(run)
    assert loss.ndim == 0 and dpred.shape == pred.shape
    print(f"{case}: loss {abs(loss.item() - want.item()) / abs(want.item()):.2e}, "
          f"dpred {rel(dpred, 1.5 * want_d):.2e}")
    np.testing.assert_allclose(loss.item(), want.item(), rtol=bar_loss)
    assert rel(dpred, 1.5 * want_d) < bar_d
    # the composed path: normalise, gather, then the loss of two lists
    with torch.no_grad():
        target = HF.gather_tokens(HF.layer_norm(hd), rows)
        holder = types.SimpleNamespace(loss=torch.nn.SmoothL1Loss())
        composed = IJEPAPL.calculate_loss(holder, [pred.to(cuda)], [target])
    np.testing.assert_allclose(loss.item(), composed.item(), rtol=1e-5)


def test_block_loss_refuses_a_row_beyond_the_teacher_output(cuda):
    from adell_mri_amd import functional as HF

    pred, h = torch.zeros((2, 2, 8), device=cuda), torch.zeros((2, 9, 8), device=cuda)
    with pytest.raises(IndexError, match="index 9 is out of bounds"):
        HF.ijepa_block_loss(pred, h, [3, 9])


# ---- one transformer block at the new sequence lengths ---------------------------------------------
def _block_reference(sd, x, heads):
    """TransformerBlock (layers/vit.py) in fp64 from its state dict."""
    p = {k: v.double() for k, v in sd.items()}
    E = x.shape[-1]
    B, t = x.shape[:2]
    n1 = F.layer_norm(x, (E,), p["norm_op_1.weight"], p["norm_op_1.bias"])
    width = p["mha.qkv.weight"].shape[0] // heads
    a = p["mha.q_norm.weight"].shape[0]
    qkv = (n1 @ p["mha.qkv.weight"].T).reshape(B, t, heads, width).permute(0, 2, 1, 3)
    q = F.layer_norm(qkv[..., :a], (a,), p["mha.q_norm.weight"], p["mha.q_norm.bias"])
    k = F.layer_norm(qkv[..., a:2 * a], (a,), p["mha.k_norm.weight"], p["mha.k_norm.bias"])
    v = qkv[..., 2 * a:]
    o = torch.softmax(q @ k.transpose(-1, -2) * a ** -0.5, -1) @ v
    o = o.permute(0, 2, 1, 3).reshape(B, t, -1)
    x = x + o @ p["mha.output_layer.weight"].T + p["mha.output_layer.bias"]
    n2 = F.layer_norm(x, (E,), p["norm_op_2.weight"], p["norm_op_2.bias"])
    m = F.gelu(n2 @ p["mlp.op.0.weight"].T + p["mlp.op.0.bias"])
    return x + m @ p["mlp.op.2.weight"].T + p["mlp.op.2.bias"]


@pytest.mark.parametrize("tokens", [6, 11, 18])
def test_transformer_block_at_the_new_sequence_lengths(cuda, tokens):
    """Width 32, 4 heads, forward and backward against fp64 at the bounds of
    tests/test_attention_plans.py: output 1e-5, gradients 5e-5 of their largest entry."""
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.layers.vit import TransformerBlock

    block = TransformerBlock(32, 32, 32, n_heads=4, mlp_structure=[64],
                             adn_fn=get_adn_fn(1, "identity", "gelu", 0.0))
    sd = fill_state_dict(block.state_dict(), gain=1.5, norm_weight_offset=1.0)
    assert set(sd) == {"mha.qkv.weight", "mha.q_norm.weight", "mha.q_norm.bias", "mha.k_norm.weight",
                       "mha.k_norm.bias", "mha.output_layer.weight", "mha.output_layer.bias",
                       "norm_op_1.weight", "norm_op_1.bias", "norm_op_2.weight", "norm_op_2.bias",
                       "mlp.op.0.weight", "mlp.op.0.bias", "mlp.op.2.weight", "mlp.op.2.bias"}
    block.load_state_dict(sd)
    block = block.to(cuda).train()
    x, r = uniform((3, tokens, 32), tokens), uniform((3, tokens, 32), tokens + 1)
    xd = x.to(cuda).requires_grad_(True)
    y = block(xd)
    y.backward(r.to(cuda))
    ref = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    want = _block_reference(ref, xr, 4)
    want.backward(r.double())
    errs = {"out": rel(y, want), "dx": rel(xd.grad, xr.grad)}
    for k, p in block.named_parameters():
        errs[k] = rel(p.grad, ref[k].grad)
    # exactly zero in exact arithmetic (one bias on every key moves a whole row of scores, which the
    # softmax ignores): fp64 leaves 1e-17 of noise there, so the error is taken against the k-norm
    # weight's gradient, the tensor the same kernel writes beside it
    k = "mha.k_norm.bias"
    assert float(ref[k].grad.abs().max()) < 1e-12
    errs[k] = float((block.mha.k_norm.bias.grad.double().cpu() - ref[k].grad).abs().max() /
                    ref["mha.k_norm.weight"].grad.abs().max())
    print(tokens, {k: f"{e:.2e}" for k, e in errs.items()})
    assert errs.pop("out") < 1e-5
    bad = {k: e for k, e in errs.items() if not e < 5e-5}
    assert not bad, bad


# ---- one training step -------------------------------------------------------------------------------
def build_pl(name, cuda):
    """IJEPAPL of one fixture network: weights from fill_state_dict, then a fresh teacher made from
    those weights (as the constructor makes it from the initial ones)."""
    from adell_mri_amd.modules.self_supervised.pl import IJEPAPL
    from adell_mri_amd.utils import ExponentialMovingAverage

    g = StepGold(name)
    net = IJEPAPL(ema=ExponentialMovingAverage(0.99), **step_config(name))
    own = {k: v for k, v in net.state_dict().items() if not k.startswith("ema.")}
    assert list(own) == [str(k) for k in g["state_keys"]]
    net.load_state_dict(fill_state_dict(own, gain=float(g["gain"])), strict=False)
    net = net.to(cuda).train()
    net.ema = ExponentialMovingAverage(float(g.top["ema_decay"]))
    net.ema.update(net)
    return net, g, {"image": torch.from_numpy(g["x"]).to(cuda)}


def own_parameters(net):
    return [(k, p) for k, p in net.named_parameters() if not k.startswith("ema.")]


@pytest.mark.parametrize("name", NETS)
def test_training_step_matches_reference(cuda, name):
    """``IJEPAPL.training_step`` (context and target draws, the student on the context tokens, one
    predictor pass per kept target block, the teacher on the whole image, the fused block losses),
    every parameter gradient, one FusedAdamW step and the EMA update; then a validation step with
    the second draw. As in the DINO step test the fixture's EMA is reached by one more
    ``ema.update`` after the optimiser step (the one inside the step sees teacher == student)."""
    from adell_mri_amd.trainer import StepRunner

    net, g, batch = build_pl(name, cuda)
    _, want_tgts = g.draw(0)
    with torch.no_grad():       # the outputs with the step's first draw, then the draw again
        predictions, targets = net.forward_training(batch["image"], net.ema)
        assert len(predictions) == len(targets) == len(want_tgts)
        for i, (p, t) in enumerate(zip(predictions, targets)):
            assert p.shape == t.shape == g[f"pred{i}"].shape
            assert rel(p, g[f"pred{i}"]) < 1e-4 and rel(t, g[f"target{i}"]) < 1e-4, i
        composed = net.calculate_loss(predictions, targets)
        np.testing.assert_allclose(composed.item(), g["loss"], rtol=1e-4)
    net.patch_masker_.rng = np.random.default_rng(net.seed)
    runner = StepRunner(net)
    runner.optimizer.zero_grad()
    loss = net.training_step(batch, 0)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-4)
    loss.backward()
    seen = 0
    for k, p in own_parameters(net):
        if "grad:" + k in g.files:
            assert grad_rel_err(g, k, p.grad.cpu().numpy()) < 5e-3, k
            seen += 1
        else:       # what the student never touches: class token, registers
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    assert seen == sum(k.startswith("grad:") for k in g.files)
    runner.optimizer.step()
    net.ema.update(net)
    for k, p in own_parameters(net):
        np.testing.assert_allclose(p.detach().cpu().numpy(), g["step1:" + k], rtol=2e-4, atol=2e-6,
                                   err_msg=k)
    shadow = dict(net.ema.shadow.named_parameters())
    for k, _ in own_parameters(net):
        np.testing.assert_allclose(shadow[k].detach().cpu().numpy(), g["ema1:" + k], rtol=1e-5,
                                   atol=1e-7, err_msg=k)
    # a validation step: the second draw, no EMA update, no gradient
    before = {k: p.detach().clone() for k, p in net.ema.shadow.named_parameters()}
    grads = {k: None if p.grad is None else p.grad.clone() for k, p in own_parameters(net)}
    ema_steps = net.ema.step
    with torch.no_grad():
        val = net.validation_step(batch, 0)
    np.testing.assert_allclose(val.item(), g["val_loss"], rtol=1e-4)
    assert not val.requires_grad and net.ema.step == ema_steps
    for k, p in net.ema.shadow.named_parameters():
        assert torch.equal(p, before[k]), k
    for k, p in own_parameters(net):
        assert (p.grad is None) if grads[k] is None else torch.equal(p.grad, grads[k]), k
