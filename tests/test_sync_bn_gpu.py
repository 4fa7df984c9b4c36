"""Synchronised batch norm at the ops level, one process: the split reductions of a batch-norm site
(ops.bn_stats_sums / bn_stats_from_sums / norm_act_bwd_sums / norm_act_bwd_apply_sums).

A batch of 4 is cut in two halves, as two ranks would hold it. Adding the halves' records is what
the all-reduce does; each half's apply must then give its rows of the unsplit site
(functional.norm_drop_act(norm="batch") on the whole batch): output, running buffers, dx, dgamma
summed over the halves, dbeta. A record of the whole batch (a world of one) reproduces the unsplit
path bit for bit. Dropout masks depend on an element's place in the batch, so dropout is checked on
the whole batch (split path == fused path) rather than across halves."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

ACTS = [("identity", 0.0), ("swish", 0.0), ("leaky_relu", 0.1), ("prelu", 0.0)]


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def _operands(cuda, C, shape, act, seed=0):
    g = torch.Generator().manual_seed(seed + C)
    x = (torch.randn((4, C) + shape, generator=g) * 1.7 + 0.4).to(cuda)
    dout = torch.randn((4, C) + shape, generator=g).to(cuda)
    gamma = (torch.rand(C, generator=g) + 0.5).to(cuda)
    beta = (torch.randn(C, generator=g) * 0.2).to(cuda)
    act_w = (torch.rand(C, generator=g) * 0.3).to(cuda) if act == "prelu" else None
    return x, dout, gamma, beta, act_w


def _running(C, cuda):
    return (torch.full((C,), 0.1, device=cuda), torch.full((C,), 0.9, device=cuda),
            torch.zeros((), dtype=torch.int64, device=cuda))


def _whole(x, dout, gamma, beta, act, act_p, act_w, drop_p=0.0, part=None):
    """The unsplit site through the functional layer (autograd)."""
    from adell_mri_amd import functional as HF
    from adell_mri_amd import ops

    C = x.shape[1]
    running = _running(C, x.device)
    xl = ops.ndhwc(x.detach().clone()).requires_grad_(True)
    if part is not None:
        xl._adell_partials = part
    g = gamma.clone().requires_grad_(True)
    b = beta.clone().requires_grad_(True)
    w = None if act_w is None else act_w.clone().requires_grad_(True)
    out = HF.norm_drop_act(xl, norm="batch", eps=1e-5, gamma=g, beta=b, running=running,
                           momentum=0.1, act=act, act_p=act_p, act_w=w, drop_p=drop_p,
                           training=True)
    out.backward(ops.ndhwc(dout))
    return dict(out=out.detach(), dx=xl.grad, dgamma=g.grad, dbeta=b.grad,
                dact_w=None if w is None else w.grad, running=running)


def _halves(x, dout, gamma, beta, act, act_p, act_w, part=None, split_exp=None):
    """Two 'ranks' of 2 items: records summed, then each half's apply."""
    from adell_mri_amd import ops

    C = x.shape[1]
    V = x[0, 0].numel()
    xs = [ops.ndhwc(x[0:2].contiguous()), ops.ndhwc(x[2:4].contiguous())]
    ds = [ops.ndhwc(dout[0:2].contiguous()), ops.ndhwc(dout[2:4].contiguous())]
    parts = ([ops.channel_partials(h) for h in xs] if part is None
             else [part[0:2].contiguous(), part[2:4].contiguous()])
    rec = sum(ops.bn_stats_sums(p, V) for p in parts)
    running = _running(C, x.device)
    mean, rstd = ops.bn_stats_from_sums(rec, 1e-5, running, 0.1)
    kw = dict(gamma=gamma, beta=beta, act_w=act_w, act_p=act_p)
    outs = [ops.norm_act_fwd(h, mean, rstd, act, stats_per_item=0, split_exp=split_exp, **kw)
            for h in xs]
    recs = [ops.norm_act_bwd_sums(h, d, mean, rstd, act, want_affine_grads=True, **kw)
            for h, d in zip(xs, ds)]
    brec = recs[0][0] + recs[1][0]
    dxs = [ops.norm_act_bwd_apply_sums(h, d, mean, rstd, brec, act, **kw) for h, d in zip(xs, ds)]
    dact_w = None
    if act_w is not None:
        dact_w = sum(ops.prelu_wgrad(h, d, mean, rstd, act_w, gamma=gamma, beta=beta,
                                     stats_per_item=0) for h, d in zip(xs, ds))
    return dict(out=torch.cat(outs), dx=torch.cat(dxs), dgamma=recs[0][1] + recs[1][1],
                dbeta=recs[0][2] + recs[1][2], dact_w=dact_w, running=running, rec=rec, brec=brec,
                outs=outs)


def _check(h, w, tol=2e-6):
    for k in ("out", "dx", "dgamma", "dbeta", "dact_w"):
        if w[k] is None:
            assert h[k] is None, k
            continue
        assert _rel(h[k], w[k]) < tol, (k, _rel(h[k], w[k]))
    for a, b in zip(h["running"][:2], w["running"][:2]):
        assert _rel(a, b) < tol
    assert int(h["running"][2]) == int(w["running"][2]) == 1


@pytest.mark.parametrize("act,act_p", ACTS)
@pytest.mark.parametrize("C,shape", [(3, (6, 5, 7)), (16, (8, 8, 8)), (64, (4, 6, 8)), (512, (2, 3, 4))])
def test_half_batch_records_merge_to_the_whole_batch(cuda, C, shape, act, act_p):
    x, dout, gamma, beta, act_w = _operands(cuda, C, shape, act)
    w = _whole(x, dout, gamma, beta, act, act_p, act_w)
    h = _halves(x, dout, gamma, beta, act, act_p, act_w)
    _check(h, w)
    assert float(h["rec"][-1]) == 4 * x[0, 0].numel() == float(h["brec"][-1])


@pytest.mark.parametrize("C", [4, 32])
def test_feature_vectors(cuda, C):
    """[B, C] inputs (a projection head's batch norm) as [B, C, 1, 1, 1] volumes."""
    x, dout, gamma, beta, _ = _operands(cuda, C, (1, 1, 1), "swish", seed=5)
    _check(_halves(x, dout, gamma, beta, "swish", 0.0, None),
           _whole(x, dout, gamma, beta, "swish", 0.0, None))


def test_conv_epilogue_partials(cuda):
    """A site fed by the partials a conv epilogue left in y._adell_partials."""
    from adell_mri_amd import functional as HF
    from adell_mri_amd import ops

    g = torch.Generator().manual_seed(3)
    x0 = torch.randn((4, 8, 12, 12, 12), generator=g).to(cuda)
    wt = (torch.randn((32, 8, 3, 3, 3), generator=g) * 0.1).to(cuda)
    with torch.no_grad():
        y = HF.conv3d(ops.ndhwc(x0), wt, None, 1, 1)
    part = y._adell_partials
    assert part.shape[0] == 4 and part.shape[2] == 32
    dout = torch.randn(y.shape, generator=g).to(cuda)
    gamma = torch.linspace(0.5, 1.5, 32, device=cuda)
    beta = torch.linspace(-0.2, 0.2, 32, device=cuda)
    _check(_halves(y, dout, gamma, beta, "swish", 0.0, None, part=part),
           _whole(y, dout, gamma, beta, "swish", 0.0, None, part=part))


@pytest.mark.parametrize("C", [16, 64])
def test_split_rows_output(cuda, C):
    from adell_mri_amd import ops

    x, dout, gamma, beta, _ = _operands(cuda, C, (8, 8, 8), "swish", seed=7)
    xw = ops.ndhwc(x)
    mean, rstd = ops.stats_finalize(ops.channel_partials(xw), 512, 1e-5, per_item=False)
    ref = ops.norm_act_fwd(xw, mean, rstd, "swish", gamma=gamma, beta=beta, stats_per_item=0,
                           split_exp=9)
    h = _halves(x, dout, gamma, beta, "swish", 0.0, None, split_exp=9)
    sr = ops.SplitRows(9, ops.split_exponents(4, C, 9, x.device))
    sr2 = ops.SplitRows(9, ops.split_exponents(2, C, 9, x.device))
    got = torch.cat([ops.rows_to_f32(o, sr2) for o in h["outs"]])
    assert _rel(got, ops.rows_to_f32(ref, sr)) < 2e-6


@pytest.mark.parametrize("shape", [(6, 5, 7), (84, 80, 80)])
def test_world_of_one_statistics_are_bit_identical(cuda, shape):
    """One rank's record gives stats_finalize's mean / rstd bit for bit (also through the two-level
    fold of more than 512 tiles), and bn_running_update's buffers."""
    from adell_mri_amd import ops

    g = torch.Generator().manual_seed(11)
    x = ops.ndhwc((torch.randn((2, 3) + shape, generator=g) * 2 + 1).to(cuda))
    part = ops.channel_partials(x)
    V = x[0, 0].numel()
    m0, r0 = ops.stats_finalize(part, V, 1e-5, per_item=False)
    ref = _running(3, cuda)
    ops.bn_running_update(m0, r0, ref[0], ref[1], ref[2], 2 * V, 1e-5, 0.1)
    run = _running(3, cuda)
    m1, r1 = ops.bn_stats_from_sums(ops.bn_stats_sums(part, V), 1e-5, run, 0.1)
    assert torch.equal(m0, m1) and torch.equal(r0, r1)
    for a, b in zip(run, ref):
        assert torch.allclose(a.float(), b.float(), rtol=1e-6, atol=0)
    # momentum None: the cumulative average of num_batches_tracked
    run = _running(3, cuda)
    ops.bn_stats_from_sums(ops.bn_stats_sums(part, V), 1e-5, run, None)
    assert int(run[2]) == 1 and torch.allclose(run[0], m0)


@pytest.mark.parametrize("act,act_p", [("swish", 0.0), ("prelu", 0.0)])
@pytest.mark.parametrize("C", [3, 32])
def test_split_backward_with_dropout_is_the_fused_backward(cuda, C, act, act_p):
    """Whole batch, dropout on: reduce -> apply with the batch's own record == adell_norm_act_bwd."""
    from adell_mri_amd import ops

    x, dout, gamma, beta, act_w = _operands(cuda, C, (6, 8, 10), act, seed=13)
    x, dout = ops.ndhwc(x), ops.ndhwc(dout)
    V = x[0, 0].numel()
    mean, rstd = ops.stats_finalize(ops.channel_partials(x), V, 1e-5, per_item=False)
    kw = dict(gamma=gamma, beta=beta, act_w=act_w, act_p=act_p, drop_p=0.3, seed=1234,
              rng_offset=5)
    dx0, dg0, db0 = ops.norm_act_bwd(x, dout, mean, rstd, act, stats_per_item=0,
                                     want_affine_grads=True, **kw)
    rec, dg1, db1 = ops.norm_act_bwd_sums(x, dout, mean, rstd, act, want_affine_grads=True, **kw)
    dx1 = ops.norm_act_bwd_apply_sums(x, dout, mean, rstd, rec, act, **kw)
    assert torch.equal(dx0, dx1) and torch.equal(dg0, dg1) and torch.equal(db0, db1)
    assert float(rec[-1]) == 4 * V
    assert torch.allclose(rec[C:2 * C].float(), dg0, rtol=1e-6, atol=1e-6)


def _modules(cuda):
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.layers.res_net import _NormLeaf

    torch.manual_seed(0)
    adn = get_adn_fn(3, "batch", "prelu", 0.0)(16)
    leaf = _NormLeaf(torch.nn.BatchNorm1d, 16)
    with torch.no_grad():
        for m in (adn, leaf):
            for p in m.parameters():
                p.add_(torch.rand(p.shape) * 0.5)
    return adn.to(cuda).train(), leaf.to(cuda).train()


def test_world_of_one_converted_modules_are_bit_identical(cuda):
    from adell_mri_amd import parallel

    g = torch.Generator().manual_seed(21)
    inputs = [torch.randn((3, 16, 6, 7, 8), generator=g).to(cuda),
              torch.randn((5, 16), generator=g).to(cuda)]
    plain = _modules(cuda)
    conv = [parallel.convert_sync_batchnorm(copy.deepcopy(m)) for m in plain]
    assert all(any(isinstance(s, torch.nn.SyncBatchNorm) for s in m.modules()) for m in conv)
    for a, b, x in zip(plain, conv, inputs):
        outs, grads = [], []
        for m in (a, b):
            xi = x.clone().requires_grad_(True)
            y = m(xi)
            (y * torch.linspace(-1, 1, y.numel(), device=cuda).reshape(y.shape)).sum().backward()
            outs.append(y.detach())
            grads.append([xi.grad] + [p.grad for p in m.parameters()])
        assert torch.equal(outs[0], outs[1])
        for ga, gb in zip(*grads):
            assert torch.equal(ga, gb)
        for ba, bb in zip(a.buffers(), b.buffers()):
            assert torch.equal(ba, bb)
