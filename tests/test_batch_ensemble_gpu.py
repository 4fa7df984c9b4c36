"""Batch ensembles on the GPU: the kernels of csrc/batch_ensemble.hip against the fp64 restatements
(tests/batch_ensemble_ref.py), every kernel result computed twice and compared bit for bit; the
layers in all their modes and the two fixture networks against the real reference
(tests/golden/batch_ensemble_*.npz, tools/make_batch_ensemble_golden.py).

Bounds (tests/golden/batch_ensemble_bounds.json, from the reference's own fp32-against-fp64 error):
kernel and layer quantities 5e-5 of the largest reference magnitude; in the step tests loss and
logits 1e-4, gradients 5e-3 by ``cases.grad_rel_err``, parameters (2e-4, 2e-6)."""
import numpy as np
import pytest
import torch

import batch_ensemble_cases as C
import batch_ensemble_ref as R
from cases import grad_rel_err
from classification_cases import zero_dropout

pytestmark = pytest.mark.gpu

SUM_BOUND = C.SUM_BOUND


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


def on_device(a, cuda):
    """fp32 on the device: rows as they are, activations in channels-last memory."""
    t = torch.as_tensor(a, dtype=torch.float32).to(cuda)
    if t.dim() == 5:
        return t.contiguous(memory_format=torch.channels_last_3d)
    if t.dim() == 4:
        return t.contiguous(memory_format=torch.channels_last)
    return t


def uniform(seed, shape, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=shape).astype(np.float32)


# ---- be_scale ------------------------------------------------------------------------------------------
SCALE_SHAPES = [(5, 6), (5, 6, 7, 5, 3), (3, 32, 9, 9), (2, 16, 24, 24, 8)]


@pytest.mark.parametrize("shape", SCALE_SHAPES)
@pytest.mark.parametrize("case", ["drawn", "row0", "single", "x_only", "table_only"])
def test_be_scale(cuda, shape, case):
    """``drawn``: members [2, 0, 2, 2, 0] of 3 -- member 1 is never drawn, member 2 sums three items;
    ``row0``: no indices, row 0 of a table of 3; ``single``: a table of one row; the last two: one
    input without a gradient."""
    from adell_mri_amd import functional as HF

    B, Cc = shape[:2]
    n = 1 if case == "single" else 3
    idx = None if case in ("row0", "single") else [2, 0, 2, 2, 0][:B]
    x, dy = uniform(1, shape), uniform(2, shape)
    table = uniform(3, (n, Cc), 0.5, 1.5)
    need_x, need_t = case != "table_only", case != "x_only"

    def run():
        xd = on_device(x, cuda).requires_grad_(need_x)
        td = on_device(table, cuda).requires_grad_(need_t)
        idxd = None if idx is None else HF.be_indices(idx, n, B, cuda)
        y = HF.be_scale(xd, td, idxd)
        y.backward(on_device(dy, cuda))
        return y.detach(), xd.grad, td.grad

    y, dx, dt = twice(run)
    want_dx, want_dt = R.be_scale_backward(x, table, idx, dy)
    errs = [rel(y, R.be_scale(x, table, idx))]
    assert y.shape == shape and (dx is None) == (not need_x) and (dt is None) == (not need_t)
    if need_x:
        assert dx.shape == shape
        errs.append(rel(dx, want_dx))
    if need_t:
        assert dt.shape == (n, Cc)
        errs.append(rel(dt, want_dt))
        drawn = {0} if idx is None else set(idx)
        for m in set(range(n)) - drawn:
            assert not bool(dt[m].any()), f"member {m} was never drawn: its row must be exactly 0"
    print(f"be_scale {shape} {case}: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < SUM_BOUND


def test_be_scale_refuses_and_poisons(cuda):
    from adell_mri_amd import functional as HF
    from adell_mri_amd.ops import AdellHipError

    x = on_device(uniform(1, (2, 8, 4, 4, 4)), cuda)
    table = on_device(uniform(2, (3, 8), 0.5, 1.5), cuda)
    with pytest.raises(AdellHipError, match="non-dense"):
        HF.be_scale(x[:, :, :, ::2], table)                               # a view with gaps
    with pytest.raises(AdellHipError):
        HF.be_scale(x, table[:1].expand(3, 8))                            # an expanded row
    with pytest.raises(ValueError, match="table"):
        HF.be_scale(x, on_device(uniform(2, (3, 4)), cuda))
    with pytest.raises(ValueError, match="int32"):
        HF.be_scale(x, table, torch.zeros(2, dtype=torch.int64, device=cuda))
    with pytest.raises(AdellHipError, match="fp32"):
        HF.be_scale(x.double(), table)
    with pytest.raises(IndexError):
        HF.be_indices([0, 3], 3, 2, cuda)
    assert HF.be_indices([-1, -3], 3, 2, cuda).tolist() == [2, 0]
    # a hand-made index outside the table is never read through: that item is NaN, the other exact
    y = HF.be_scale(x, table, torch.tensor([7, 1], dtype=torch.int32, device=cuda))
    assert bool(torch.isnan(y[0]).all())
    assert torch.equal(y[1], x[1] * table[1].reshape(1, 8, 1, 1, 1)[0])


# ---- expand and mean -----------------------------------------------------------------------------------
CHUNKINGS = ([0, 3], [0, 2, 3], [0, 1, 2, 3])


@pytest.mark.parametrize("shape", [(2, 6), (2, 6, 5, 4, 3), (2, 8, 9, 9), (2, 16, 24, 24, 8)])
def test_members_expand_and_mean(cuda, shape):
    """n = 3, B = 2: the mean of post[m] * (pre[m] * x) over the members in one piece, in two chunks
    and one member at a time -- the three results bit-identical; results and gradients (the tables'
    included) against the restatement."""
    from adell_mri_amd import functional as HF

    n, Cc = 3, shape[1]
    x, dout = uniform(1, shape), uniform(2, shape)
    pre, post = uniform(3, (n, Cc), 0.5, 1.5), uniform(4, (n, Cc), 0.5, 1.5)

    def run(cuts):
        xd = on_device(x, cuda).requires_grad_(True)
        pd = on_device(pre, cuda).requires_grad_(True)
        qd = on_device(post, cuda).requires_grad_(True)
        acc = None
        for m0, m1 in zip(cuts[:-1], cuts[1:]):
            e = HF.be_members_expand(xd, pd, m0, m1)
            assert e.shape == ((m1 - m0) * shape[0],) + shape[1:]
            acc = HF.be_members_mean(e, qd, m0, m1, n, acc)
        acc.backward(on_device(dout, cuda))
        return acc.detach(), xd.grad, pd.grad, qd.grad

    results = [twice(lambda c=cuts: run(c)) for cuts in CHUNKINGS]
    for other in results[1:]:
        assert torch.equal(results[0][0], other[0]), "the mean depends on the chunking"
    e = R.members_expand(x, pre, 0, n)
    want = R.members_mean(e, post, 0, n, n)
    dy, want_dpost, _ = R.members_mean_backward(e, post, 0, n, n, dout)
    want_dx, want_dpre = R.members_expand_backward(x, pre, 0, n, dy)
    for cuts, (out, dx, dpre, dpost) in zip(CHUNKINGS, results):
        errs = [rel(out, want), rel(dx, want_dx), rel(dpre, want_dpre), rel(dpost, want_dpost)]
        print(f"members {shape} {cuts}: " + " ".join(f"{v:.2e}" for v in errs))
        assert max(errs) < SUM_BOUND


@pytest.mark.parametrize("shape", [(2, 6), (2, 6, 5, 4, 3), (2, 16, 24, 24, 8)])
def test_members_pieces_against_the_restatement(cuda, shape):
    """Each piece alone: the expand of a middle chunk, a closing mean with a running sum that takes
    a gradient, and a mean that does not close."""
    from adell_mri_amd import functional as HF

    n, Cc, B = 4, shape[1], shape[0]
    x = uniform(1, shape)
    pre, post = uniform(3, (n, Cc), 0.5, 1.5), uniform(4, (n, Cc), 0.5, 1.5)
    y = uniform(5, (2 * B,) + shape[1:])
    acc, dout, de = uniform(6, shape), uniform(7, shape), uniform(8, (2 * B,) + shape[1:])

    def expand():
        xd = on_device(x, cuda).requires_grad_(True)
        pd = on_device(pre, cuda).requires_grad_(True)
        e = HF.be_members_expand(xd, pd, 1, 3)
        e.backward(on_device(de, cuda))
        return e.detach(), xd.grad, pd.grad

    e, dx, dpre = twice(expand)
    want_dx, want_dpre = R.members_expand_backward(x, pre, 1, 3, de)
    assert max(rel(e, R.members_expand(x, pre, 1, 3)), rel(dx, want_dx),
               rel(dpre, want_dpre)) < SUM_BOUND
    assert not bool(dpre[0].any()) and not bool(dpre[3].any())        # members outside the chunk

    for m0, m1 in ((2, 4), (1, 3)):                                    # closing, not closing

        def mean():
            yd = on_device(y, cuda).requires_grad_(True)
            qd = on_device(post, cuda).requires_grad_(True)
            ad = on_device(acc, cuda).requires_grad_(True)
            out = HF.be_members_mean(yd, qd, m0, m1, n, ad)
            out.backward(on_device(dout, cuda))
            return out.detach(), yd.grad, qd.grad, ad.grad

        out, dy, dpost, dacc = twice(mean)
        want_dy, want_dpost, want_dacc = R.members_mean_backward(y, post, m0, m1, n, dout, acc)
        errs = [rel(out, R.members_mean(y, post, m0, m1, n, acc)), rel(dy, want_dy),
                rel(dpost, want_dpost), rel(dacc, want_dacc)]
        print(f"mean {shape} [{m0}, {m1}): " + " ".join(f"{v:.2e}" for v in errs))
        assert max(errs) < SUM_BOUND
        outside = sorted(set(range(n)) - set(range(m0, m1)))
        assert not bool(dpost[outside].any())


# ---- the layers against the reference ------------------------------------------------------------------
def build_layer(layer, n, cuda):
    from adell_mri_amd.modules.layers import BatchEnsemble, BatchEnsembleWrapper
    from adell_mri_amd.modules.layers.linear_blocks import Linear

    cls, dim, cin, cout, _ = C.LAYERS[layer]
    if cls == "BatchEnsemble":
        net = BatchEnsemble(dim, n, cin, cout)
    else:
        net = BatchEnsembleWrapper(Linear(cin, cout), n, cin, cout)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in C.layer_state(layer, n).items()})
    return net.to(cuda)


@pytest.mark.parametrize("layer,mode", C.layer_cases())
def test_layers_match_the_reference(cuda, layer, mode):
    g, bounds = C.layer_gold(), C.bounds()["layers"]
    n, training, idx = C.MODES[mode]
    tag = f"{layer}:{mode}:"
    for route in (("batched", "loop") if mode == "mean" else (None,)):
        net = build_layer(layer, n, cuda).train(training)
        x = on_device(C.layer_input(layer), cuda).requires_grad_(True)
        np.random.seed(C.DRAW_SEED)
        y = net(x, route=route) if idx is None else net(x, idx)
        if tag + "idxs" in g.files:          # the same draw: nothing else was drawn before it
            np.random.seed(C.DRAW_SEED)
            assert np.array_equal(np.random.randint(n, size=x.shape[0]), g[tag + "idxs"])
            after = np.random.get_state()[1].copy()
            np.random.seed(C.DRAW_SEED)
            net(x.detach())
            assert np.array_equal(np.random.get_state()[1], after)
        errs = {"y": rel(y, g[tag + "y"])}
        if tag + "dx" in g.files:
            y.backward(on_device(C.layer_dy(layer, tuple(y.shape)), cuda))
            errs["dx"] = rel(x.grad, g[tag + "dx"])
            for k, p in net.named_parameters():
                errs["d" + k] = rel(p.grad, g[tag + "d" + k])
        else:
            assert not y.requires_grad                    # the wrapper's mean runs under no_grad
        print(f"{layer} {mode} {route}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v < bounds[k]["bound"], (k, v)


def test_route_with_batch_statistics_is_the_loop(cuda):
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.layers import BatchEnsembleWrapper
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.layers.res_blocks import ResidualBlock3d

    free = lambda c: torch.nn.BatchNorm3d(c, track_running_stats=False)     # noqa: E731
    body = torch.nn.Sequential(torch.nn.Identity(), free(4)).to(cuda).eval()
    assert HF.be_route(3, 2, 4096, body) == "loop"
    block = ResidualBlock3d(4, 3, 4, 4, get_adn_fn(3, "batch", "swish", 0.0)).to(cuda).eval()
    assert HF.be_route(3, 2, 4096, block) == "batched"
    with pytest.raises(ValueError, match="route"):
        BatchEnsembleWrapper(block, 3, 4, 4).to(cuda).eval()(
            on_device(uniform(1, (2, 4, 4, 4, 4)), cuda), route="stacked")


def test_routes_agree_around_a_residual_stage(cuda):
    """The eval mean around a residual block with batch norm on running statistics: the batched
    route (in one chunk and, under a small budget, in two) and the loop give the same mean within
    the bound of a sum; the batched chunkings are not compared bit for bit (the convolution may plan
    differently for another batch size)."""
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.layers import BatchEnsembleWrapper
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.layers.res_blocks import ResidualBlock3d

    adn = get_adn_fn(3, "batch", "swish", 0.0)
    torch.manual_seed(0)
    np.random.seed(0)
    block = ResidualBlock3d(8, 3, 8, 8, adn, skip_activation=True)
    layer = BatchEnsembleWrapper(block, 3, 8, 8, adn).to(cuda).eval()
    x = on_device(uniform(1, (2, 8, 6, 6, 4)), cuda)
    loop = layer(x, route="loop")
    batched = layer(x, route="batched")
    budget = HF.BE_BATCH_BUDGET_BYTES
    HF.BE_BATCH_BUDGET_BYTES = 2 * 2 * x[0].numel() * 4                  # two members per chunk
    try:
        assert HF.be_chunk(3, 2, x[0].numel() * 4) == 2
        chunked = layer(x, route="batched")
    finally:
        HF.BE_BATCH_BUDGET_BYTES = budget
    assert layer(x).shape == x.shape
    assert rel(batched, loop) < SUM_BOUND and rel(chunked, loop) < SUM_BOUND


# ---- the networks against the reference ----------------------------------------------------------------
def build_pl(name):
    from adell_mri_amd.modules.classification.losses import configure_loss_fn
    from adell_mri_amd.modules.classification.pl import ClassNetPL, OrdNetPL
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn

    cls, _, _, _, weight_decay = C.NETS[name]
    kw = C.net_kwargs(name)
    cfg = {}
    configure_loss_fn(cfg, "ord" if cls == "OrdNet" else "cat", kw["n_classes"], None)
    wrapper = OrdNetPL if cls == "OrdNet" else ClassNetPL
    net = wrapper(adn_fn=get_adn_fn(3, "batch", "swish", 0.0), loss_fn=cfg["loss_fn"],
                  learning_rate=C.STEP_LR, optimizer_eps=C.STEP_EPS, weight_decay=weight_decay, **kw)
    zero_dropout(net)
    return net


def build_step(name, cuda):
    g = C.StepGold(name)
    net = build_pl(name)
    net.network.load_state_dict(C.fill(net.network.state_dict(), float(g["gain"])))
    if name == "ord":            # the constructor's zero, which the fill must not undo
        with torch.no_grad():
            net.network.classification_layer.op[-1].bias.zero_()
    net = net.to(cuda).train()
    batch = {"image": torch.from_numpy(g["x"]).to(cuda),
             "label": torch.tensor(C.NETS[name][3]).to(cuda)}
    return net, g, batch


@pytest.mark.parametrize("name", list(C.NETS))
def test_training_step_matches_reference(cuda, monkeypatch, name):
    """``training_step`` through ``StepRunner`` under the fixture's seed: the members every stage
    drew, logits, loss, every parameter gradient, one FusedAdamW step; then ``validate_steps`` (the
    mean over the members) and, for ``CatNet``, the forward with ``batch_idx=1``."""
    from adell_mri_amd.trainer import StepRunner, validate_steps

    net, g, batch = build_step(name, cuda)
    runner = StepRunner(net)
    assert [len(gr["params"]) for gr in runner.optimizer.param_groups] == [
        len(g[f"groups:{i}:names"]) for i in range(int(g["groups:n"]))]
    seen, forward = [], net.forward

    def record(*args, **kwargs):
        seen.append(forward(*args, **kwargs))
        return seen[-1]

    net.forward = record
    draws, randint = [], np.random.randint

    def recorder(*args, **kwargs):
        draws.append(np.array(randint(*args, **kwargs)))
        return draws[-1]

    monkeypatch.setattr(np.random, "randint", recorder)
    runner.optimizer.zero_grad()
    np.random.seed(C.STEP_SEED)
    loss = net.training_step(batch, 0)
    assert np.array_equal(np.stack(draws), g["idxs"])
    logits = torch.squeeze(seen[0][0] if name == "ord" else seen[0], 1)
    print(f"{name}: logits {rel(logits, g['logits']):.2e}, loss "
          f"{abs(loss.item() - g['total']) / g['total']:.2e}")
    assert rel(logits, g["logits"]) < C.TOL["loss"]
    np.testing.assert_allclose(loss.item(), g["total"], rtol=C.TOL["loss"])
    loss.backward()
    params = list(net.network.named_parameters())
    worst = 0.0
    for k, p in params:
        if "grad:" + k not in g.files:   # the norm of a stage's last block: its activation is skipped
            assert p.grad is None and ".adn_op." in k, k
            continue
        e = grad_rel_err(g, k, p.grad.cpu().numpy())
        worst = max(worst, e)
        assert e < C.TOL["grad"], (k, e)
    print(f"{name}: worst gradient {worst:.2e}")
    runner.optimizer.step()
    for k, v in net.network.state_dict().items():
        if k.startswith("feature_extraction."):
            continue                                   # the same tensors as ``res_net.*``
        if v.is_floating_point():
            np.testing.assert_allclose(v.detach().cpu().numpy(), g["step1:" + k],
                                       rtol=C.TOL["param"][0], atol=C.TOL["param"][1], err_msg=k)
        else:
            assert np.array_equal(v.cpu().numpy(), g["step1:" + k]), k
    del seen[:], draws[:]
    out = validate_steps(net, [batch])
    np.testing.assert_allclose(out["val_loss"], g["val_total"], rtol=C.TOL["loss"])
    vlogits = torch.squeeze(seen[0][0] if name == "ord" else seen[0], 1)
    print(f"{name}: validation logits {rel(vlogits, g['val_logits']):.2e}")
    assert rel(vlogits, g["val_logits"]) < C.TOL["loss"] and not draws
    if name == "cat":
        net.eval()
        with torch.no_grad():
            one = torch.squeeze(net.network(batch["image"], batch_idx=C.BATCH_IDX), 1)
        assert rel(one, g["idx_logits"]) < C.TOL["loss"] and not draws


def test_fit_and_validate_through_the_wrapper(cuda):
    from adell_mri_amd.trainer import fit_steps, test_steps, validate_steps

    net, g, batch = build_step("cat", cuda)
    other = {"image": batch["image"].flip(0).contiguous(), "label": 1 - batch["label"].flip(0)}
    np.random.seed(1)
    before = {k: v.detach().clone() for k, v in net.network.named_parameters()}
    losses = fit_steps(net, [batch, other])
    assert len(losses) == 2 and all(bool(torch.isfinite(v)) for v in losses)
    moved = [k for k, v in net.network.named_parameters() if not torch.equal(v, before[k])]
    assert "res_net.be_operations.0.all_weights.pre" in moved
    assert "res_net.be_operations.1.all_weights.post" in moved
    out = validate_steps(net, [batch, other])
    assert np.isfinite(out["val_loss"]) and "V_AUC" in out
    assert np.isfinite(test_steps(net, [batch])["test_loss"])


def test_wrapper_training_runs_without_a_host_synchronisation(cuda):
    """The wrapper's training forward and backward from given tensors (draw, one upload, the two
    scales around a Linear) under torch's synchronisation check."""
    from adell_mri_amd.modules.layers import BatchEnsembleWrapper
    from adell_mri_amd.modules.layers.linear_blocks import Linear

    np.random.seed(3)
    layer = BatchEnsembleWrapper(Linear(16, 12), 4, 16, 12).to(cuda).train()
    x = on_device(uniform(1, (6, 16)), cuda)
    dy = on_device(uniform(2, (6, 12)), cuda)

    def run():
        layer.zero_grad()
        xd = x.clone().requires_grad_(True)
        y = layer(xd)
        y.backward(dy)
        listed = layer(x, idx=[0, 3, -1, 2, 1, 0])
        return y.detach(), xd.grad, layer.all_weights["pre"].grad.clone(), listed.detach()

    run()                                   # allocator warm-up
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(t).all()) for t in second)
