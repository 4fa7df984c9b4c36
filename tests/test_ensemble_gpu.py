"""Ensemble classification and the Gaussian-process head on the GPU: the kernels of csrc/ensemble.hip
against the fp64 restatements (tests/ensemble_ref.py, pinned to the reference by
tests/test_ensemble.py), every kernel result computed twice and compared bit for bit; one training
step and a following validation step of the five fixture networks against the real reference
(tests/golden/ensemble_step_*.npz), and for the two Gaussian-process ensembles the fit of the
precision matrix over three batches and ``predict_step_gp`` with given draws.

Bounds are the project's: ``SUM_BOUND`` = 5e-5 of the largest reference magnitude for kernel outputs
and gradients; in the step tests loss 1e-4, gradients 5e-3 by ``cases.grad_rel_err``, parameters
(2e-4, 2e-6). tools/make_ensemble_golden.py asserts that the reference's own fp32 step uses at most
a quarter of the step tolerances against its fp64 step (``fp32_vs_fp64``) and records, for every
kernel and fitted quantity, the reference's fp32-against-fp64 error in
tests/golden/ensemble_bounds.json: all of them are inside a quarter of ``SUM_BOUND`` (the worst is
phi at 2.8e-6; the covariance behind the inverse 3.8e-7), so every ``bound`` read from that file IS
``SUM_BOUND``; had one been outside, its bound there would be four times the recorded error."""
import numpy as np
import pytest
import torch

import ensemble_cases as C
import ensemble_ref as ER
from cases import grad_rel_err
from test_ensemble import build_pl

pytestmark = pytest.mark.gpu

SUM_BOUND = 5e-5


def bound(group, quantity):
    b = C.bounds()[group][quantity]["bound"]
    assert b >= SUM_BOUND
    return b


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
            assert torch.equal(torch.nan_to_num(u, nan=12345.0), torch.nan_to_num(v, nan=12345.0)), \
                "two runs differ"
    return a


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- the Gaussian-process layer ----------------------------------------------------------------------------
def run_gp(cuda, shape, case, normalize, route=None):
    from adell_mri_amd import functional as HF

    t = {k: dev(v, cuda) for k, v in case.items()}
    for k in ("x", "weights") + (("gamma", "beta") if normalize else ()):
        t[k].requires_grad_(True)
    logits, phi = HF.gp_phi(t["x"], t["gamma"] if normalize else None, t["beta"] if normalize else None,
                            t["W"], t["b"], t["weights"], C.gp_scale(shape[2]), C.GP_EPS, route=route)
    ((logits * t["dlogits"]).sum() + (phi * t["dphi"]).sum()).backward()
    return (logits.detach(), phi.detach(), t["x"].grad, t["weights"].grad,
            t["gamma"].grad if normalize else None, t["beta"].grad if normalize else None)


def check_gp(cuda, shape, normalize, route, want_route):
    from adell_mri_amd import functional as HF

    case = C.gp_case(shape)
    assert HF.gp_route(*shape[:3]) == want_route
    logits, phi, dx, dw, dg, db = twice(lambda: run_gp(cuda, shape, case, normalize, route))
    norm = dict(gamma=case["gamma"], beta=case["beta"], eps=C.GP_EPS) if normalize else {}
    scale = C.gp_scale(shape[2])
    want_phi, want_logits = ER.gp_phi(case["x"], case["W"], case["b"], case["weights"], scale, **norm)
    want = ER.gp_phi_bwd(case["x"], case["W"], case["b"], case["weights"], scale, case["dlogits"],
                         case["dphi"], **norm)
    figures = {"phi": rel(phi, want_phi), "logits": rel(logits, want_logits), "dx": rel(dx, want["dx"]),
               "dweights": rel(dw, want["dweights"])}
    if normalize:
        figures.update(dgamma=rel(dg, want["dgamma"]), dbeta=rel(db, want["dbeta"]))
    print(shape, normalize, route, figures)
    assert figures["phi"] < bound("kernels", "phi") and figures["logits"] < bound("kernels", "logits")
    assert all(v < SUM_BOUND for v in figures.values()), figures


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("shape", C.GP_SHAPES)
def test_gp_fused_route_matches_the_restatement(cuda, shape, normalize):
    check_gp(cuda, shape, normalize, None, "fused")


@pytest.mark.parametrize("normalize", [True, False])
def test_gp_composed_route_matches_the_restatement(cuda, normalize):
    """A shape ``gp_route`` sends to the composed route, and the composed route forced on a shape
    the fused one takes."""
    check_gp(cuda, C.GP_COMPOSED_SHAPE, normalize, None, "composed")
    check_gp(cuda, C.GP_SHAPES[1], normalize, "composed", "fused")


def test_gp_gradient_of_one_output_alone(cuda):
    """Only the logits, or only phi, carry a gradient: the other is not materialised."""
    from adell_mri_amd import functional as HF

    shape = C.GP_SHAPES[3]
    case = C.gp_case(shape)
    scale = C.gp_scale(shape[2])
    for which in ("logits", "phi"):
        def run():
            t = {k: dev(v, cuda) for k, v in case.items()}
            for k in ("x", "weights", "gamma", "beta"):
                t[k].requires_grad_(True)
            logits, phi = HF.gp_phi(t["x"], t["gamma"], t["beta"], t["W"], t["b"], t["weights"], scale,
                                    C.GP_EPS)
            ((logits * t["dlogits"]).sum() if which == "logits" else (phi * t["dphi"]).sum()).backward()
            return t["x"].grad, t["weights"].grad, t["gamma"].grad
        dx, dw, dg = twice(run)
        want = ER.gp_phi_bwd(case["x"], case["W"], case["b"], case["weights"], scale,
                             case["dlogits"] if which == "logits" else None,
                             case["dphi"] if which == "phi" else None, gamma=case["gamma"],
                             beta=case["beta"], eps=C.GP_EPS)
        assert rel(dx, want["dx"]) < SUM_BOUND and rel(dg, want["dgamma"]) < SUM_BOUND
        if which == "logits":
            assert rel(dw, want["dweights"]) < SUM_BOUND
        else:
            assert dw is None


def test_gp_refuses_cpu_non_dense_and_rank_3_inputs(cuda):
    from adell_mri_amd import _lib, ops
    from adell_mri_amd import functional as HF

    shape = C.GP_SHAPES[1]
    t = {k: dev(v, cuda) for k, v in C.gp_case(shape).items()}
    args = lambda x: (x, t["gamma"], t["beta"], t["W"], t["b"], t["weights"], C.gp_scale(shape[2]))  # noqa: E731
    with pytest.raises(_lib.AdellHipError):
        ops.gp_phi_fwd(*args(t["x"].cpu()))
    wide = torch.randn((shape[0], 2 * shape[1]), device=cuda)
    with pytest.raises(_lib.AdellHipError, match="non-dense"):
        ops.gp_phi_fwd(*args(wide[:, ::2]))
    with pytest.raises(NotImplementedError, match="rank above 2"):
        HF.gp_phi(*args(t["x"][:, None]))
    with pytest.raises(_lib.AdellHipError, match="fused route"):
        big = C.gp_case(C.GP_COMPOSED_SHAPE)
        b = {k: dev(v, cuda) for k, v in big.items()}
        ops.gp_phi_fwd(b["x"], None, None, b["W"], b["b"], b["weights"], 1.0)


# ---- the precision matrix ----------------------------------------------------------------------------------
def phi_batches(shape):
    """Three fp32 phi batches [N, r] of one shape (the restatement's, rounded)."""
    case = C.gp_case(shape)
    return [ER.gp_phi(C.gp_case(shape, seed=200 + k)["x"], case["W"], case["b"], None,
                      C.gp_scale(shape[2]), case["gamma"], case["beta"], C.GP_EPS)[0].astype(np.float32)
            for k in range(3)]


@pytest.mark.parametrize("momentum", [False, True])
@pytest.mark.parametrize("kind", list(C.PRECISION_KINDS))
def test_precision_update_three_batches(cuda, kind, momentum):
    from adell_mri_amd.modules.layers.gaussian_process import GaussianProcessLayer

    n_classes, ordinal, _ = C.PRECISION_KINDS[kind]
    N, i, r, o = C.PRECISION_SHAPE
    phis, probs = phi_batches(C.PRECISION_SHAPE), C.precision_batches(kind)
    layer = GaussianProcessLayer(i, r, n_classes, n_outputs=o, m=C.PRECISION_M, ordinal=ordinal).to(cuda)

    def run():
        layer.reset_inv_cov()
        for phi, p in zip(phis, probs):
            layer.update_inv_cov_from_phi(dev(phi, cuda), dev(p, cuda), use_momentum=momentum)
        return (layer.inv_conv.clone(),)

    (P,) = twice(run)
    want = np.eye(r)
    for phi, p in zip(phis, probs):
        want = ER.precision_update(want, phi, p, momentum, C.PRECISION_M)
    assert P.shape == (1, r, r) and torch.equal(P[0], P[0].T)
    e = rel(P[0], want)
    print(kind, momentum, "precision", e)
    assert e < bound("kernels", "precision")
    # the fixture's fp64 matrix is the same thing from the real reference
    assert rel(P[0], C.kernel_gold()[f"prec:{kind}:{int(momentum)}:P"]) < bound("kernels", "precision")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (5, 24, 130, 3), (3, 65, 257, 2)])
def test_precision_variance_and_samples(cuda, shape):
    """Tile edges of the precision update (r = 1, 130, 257), then the variance and the samples."""
    from adell_mri_amd import ops

    N, i, r, o = shape
    phis = phi_batches(shape)
    g = np.random.default_rng(r)
    probs = [(1.0 / (1.0 + np.exp(-g.normal(size=(N, 1))))).astype(np.float32) for _ in phis]

    def update():
        P = torch.eye(r, device=cuda)[None].contiguous()
        for phi, p in zip(phis, probs):
            ops.gp_precision_update(P, dev(phi, cuda), dev(p, cuda))
        return (P,)

    (P,) = twice(update)
    want = np.eye(r)
    for phi, p in zip(phis, probs):
        want = ER.precision_update(want, phi, p)
    assert torch.equal(P[0], P[0].T) and rel(P[0], want) < bound("kernels", "precision")
    cov = ER.covariance(want).astype(np.float32)
    (var,) = twice(lambda: (ops.gp_variance(dev(phis[0], cuda), dev(cov, cuda)[None].contiguous()),))
    want_var = ER.variance(phis[0], cov)
    assert var.shape == (N,) and rel(var, want_var) < bound("kernels", "variance")
    mean = g.normal(size=(N, o)).astype(np.float32)
    var32 = var.cpu().numpy().copy()
    var32[0] = -1e-7                # a variance that rounding made negative is used as 0
    for S in C.SAMPLE_S:
        eps = C.sample_eps(S, N, o)
        samples, smean, sstd = twice(lambda: ops.gp_sample(dev(mean, cuda), dev(var32, cuda),
                                                           dev(eps, cuda)))
        ws, wm, wsd = ER.sample(mean, var32, eps)
        assert samples.shape == (S, N, o) and rel(samples, ws) < SUM_BOUND and rel(smean, wm) < SUM_BOUND
        assert torch.equal(samples[:, 0], dev(mean, cuda)[0].expand(S, o))
        if S == 1:
            assert bool(torch.isnan(sstd).all())
            assert bool(torch.isnan(samples.std(0)).all())     # as torch's
        else:
            assert rel(sstd, wsd) < SUM_BOUND and rel(sstd, samples.std(0)) < SUM_BOUND


# ---- ensemble_pool -----------------------------------------------------------------------------------------
def member(a, cuda):
    t = dev(a, cuda)
    if t.dim() == 4:
        return t.contiguous(memory_format=torch.channels_last)
    if t.dim() == 5:
        return t.contiguous(memory_format=torch.channels_last_3d)
    return t


def run_pool(cuda, arrays, g):
    from adell_mri_amd import functional as HF

    leaves = [member(a, cuda).requires_grad_(True) for a in arrays]
    out = HF.ensemble_pool(leaves)
    out.backward(dev(g, cuda))
    return (out.detach(),) + tuple(t.grad for t in leaves)


@pytest.mark.parametrize("case", ["one", "three", "nine"])
def test_ensemble_pool(cuda, case):
    from adell_mri_amd import ops

    if case == "one":
        arrays = [np.full((1, 1, 1, 1), -2.5, dtype=np.float32)]
    elif case == "three":
        arrays = [C.pool_member(s) for s in C.POOL_MEMBERS]
    else:       # more than ops.ENSEMBLE_MAX members: channel_max and the concat copy
        arrays = [C.pool_member(s, seed=k) for k in range(3) for s in C.POOL_MEMBERS]
        assert len(arrays) > ops.ENSEMBLE_MAX
    want, want_arg = ER.pool(arrays)
    g = np.random.default_rng(3).normal(size=want.shape).astype(np.float32)
    out, *grads = twice(lambda: run_pool(cuda, arrays, g))
    assert out.shape == want.shape and np.array_equal(out.cpu().numpy(), want)
    for got, w, a in zip(grads, ER.pool_bwd(arrays, g), arrays):
        assert got.shape == a.shape and np.array_equal(got.cpu().numpy(), w)
    if case != "nine":
        out2, arg = twice(lambda: ops.ensemble_pool_fwd([member(a, cuda) for a in arrays]))
        assert torch.equal(out2, out) and arg.dtype == torch.int32
        assert np.array_equal(arg.cpu().numpy(), want_arg)


def test_ensemble_pool_tie_takes_the_lowest_index(cuda):
    from adell_mri_amd import ops

    a = C.pool_member(C.POOL_MEMBERS[0])
    a[:, :, 1, 2] = a[:, :, 2, 5] = 10.0
    b = C.pool_member(C.POOL_MEMBERS[2])
    out, arg = twice(lambda: ops.ensemble_pool_fwd([member(a, cuda), member(b, cuda)]))
    assert bool((arg[:, :5] == 1 * 7 + 2).all()) and bool((out[:, :5] == 10.0).all())
    assert bool((arg[:, 5:] == 0).all())
    g = np.ones(out.shape, dtype=np.float32)
    _, da, db = twice(lambda: run_pool(cuda, [a, b], g))
    assert float(da[:, :, 1, 2].min()) == 1.0 and float(da.sum()) == a.shape[0] * a.shape[1]
    assert torch.equal(db, torch.ones_like(db))
    a[0, 3, 0, 4] = np.nan         # a NaN wins, as in torch.max
    out, arg = ops.ensemble_pool_fwd([member(a, cuda)])
    assert bool(torch.isnan(out[0, 3])) and int(arg[0, 3]) == 4 and int(torch.isnan(out).sum()) == 1


def test_ensemble_pool_refuses_cpu_and_non_dense_inputs(cuda):
    from adell_mri_amd import _lib, ops

    x = member(C.pool_member(C.POOL_MEMBERS[1]), cuda)
    v = dev(C.pool_member(C.POOL_MEMBERS[2]), cuda)
    for bad in (x[..., ::2], x.contiguous(), v[:, ::2]):
        with pytest.raises(_lib.AdellHipError, match="non-dense"):
            ops.ensemble_pool_fwd([bad])
    with pytest.raises(_lib.AdellHipError):
        ops.ensemble_pool_fwd([x.cpu()])
    with pytest.raises(ValueError, match="members"):
        ops.ensemble_pool_fwd([v] * (ops.ENSEMBLE_MAX + 1))
    with pytest.raises(ValueError, match="batch sizes"):
        ops.ensemble_pool_fwd([v, v[:1].contiguous()])


# ---- ensemble_average --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Cc,B", C.AVERAGE_CASES)
def test_ensemble_average(cuda, K, Cc, B):
    from adell_mri_amd import functional as HF

    logits, dy = C.average_case(K, Cc, B)

    def run():
        leaves = [dev(x, cuda).requires_grad_(True) for x in logits]
        y = HF.ensemble_average(leaves)
        y.backward(dev(dy, cuda))
        return (y.detach(),) + tuple(t.grad for t in leaves)

    y, *grads = twice(run)
    assert y.shape == (B, Cc) and rel(y, ER.average(logits)) < SUM_BOUND
    want = ER.average_bwd(logits, dy)
    for got in grads:
        assert rel(got, want) < SUM_BOUND and torch.equal(got, grads[0])


# ---- networks ----------------------------------------------------------------------------------------------
def build_step(name, cuda):
    """The wrapper of one fixture network with the fixture's weights on the device, in ``train()``
    mode with every dropout rate zeroed, and its batch."""
    g = C.StepGold(name)
    net, _ = build_pl(name)
    net.load_state_dict(C.fill(net.state_dict(), float(g["gain"])))
    net = net.to(cuda).train()
    batch = {"image": torch.from_numpy(g["x"]).to(cuda), "label": torch.from_numpy(g["y"]).to(cuda)}
    return net, g, batch


def check_gaussian_process(net, g, batch, name, cuda):
    """``fit_gaussian_process`` over the fixture's three batches, then ``predict_step_gp`` with the
    fixture's draws, against the reference's fp64 records. The fit (``fit:*``), ``prediction``,
    ``gp_mean`` and ``epistemic_uncertainty`` come from the real reference's methods. The sampled
    keys are tools/make_ensemble_golden.py's restatement of ``predict_step_gp`` on the reference's
    mean and variance -- given draws instead of ``MultivariateNormal``'s stream and, for
    ``predictive_std_pred`` and ``epistemic_uncertainty_pred``, the softmax over the class axis where
    the reference names axis 1 -- so those pin this project's reading (README, deviations), not
    reference parity."""
    x = g["x"]
    batches = [{"image": dev(C.fit_inputs(x, k), cuda)} for k in range(C.FIT_BATCHES)]
    net.train()
    net.fit_gaussian_process(batches)
    assert net.training
    head = net.gaussian_process_head
    P = head.inv_conv
    figures = {"fit:inv_conv": rel(P, g["fit:inv_conv"]), "fit:cov": rel(head.cov, g["fit:cov"])}
    assert torch.equal(P[0], P[0].T)
    net.eval()
    eps = dev(C.predict_eps(*g["gp:gp_mean"].shape), cuda)
    out = net.predict_step_gp(batch, 0, n_samples=C.PREDICT_SAMPLES, eps=eps)
    again = net.predict_step(batch, 0, n_samples=C.PREDICT_SAMPLES, eps=eps)
    assert sorted(out) == sorted(["prediction", "gp_mean", "gp_samples", "predictive_mean",
                                  "predictive_std", "epistemic_uncertainty", "predictive_std_pred",
                                  "epistemic_uncertainty_pred"])
    for k, v in out.items():
        assert torch.equal(v, again[k]), k
        figures["gp:" + k] = rel(v, g["gp:" + k])
    print(name, figures)
    for k, e in figures.items():
        assert e < bound(name, k), (k, e)
    net.train()


@pytest.mark.parametrize("name", C.NETS)
def test_training_step_matches_reference(cuda, name):
    """``training_step`` through ``StepRunner``: logits, loss, every parameter gradient, one
    FusedAdamW step over the groups of ``configure_optimizers``, then ``validate_steps``,
    ``test_steps`` (two classes) and ``test_step``; for the Gaussian-process ensembles the fit and the prediction behind it."""
    from adell_mri_amd.optim import FusedAdamW
    from adell_mri_amd.trainer import StepRunner, test_steps, validate_steps

    net, g, batch = build_step(name, cuda)
    runner = StepRunner(net)
    assert isinstance(runner.optimizer, FusedAdamW)
    assert [len(gr["params"]) for gr in runner.optimizer.param_groups] == [
        len(g[f"groups:{i}:names"]) for i in range(int(g["groups:n"]))]
    if name != "avg3":
        with torch.no_grad():
            features = net.forward_features([batch["image"]])
        assert rel(features, g["features"]) < bound(name, "features")
    runner.optimizer.zero_grad()
    loss = net.training_step(batch, 0)
    np.testing.assert_allclose(loss.item(), g["total"], rtol=1e-4)
    loss.backward()
    params = list(net.named_parameters())
    assert sum(k.startswith("grad:") for k in g.files) == len(params)
    worst = 0.0
    for k, p in params:
        assert p.grad is not None, k
        e = grad_rel_err(g, k, p.grad.cpu().numpy())
        worst = max(worst, e)
        assert e < 5e-3, (k, e)
    print(f"{name}: loss {abs(loss.item() - g['total']) / g['total']:.2e}, worst gradient "
          f"{worst:.2e}")
    runner.optimizer.step()
    for k, v in net.state_dict().items():
        if v.is_floating_point():
            np.testing.assert_allclose(v.detach().cpu().numpy(), g["step1:" + k], rtol=2e-4,
                                       atol=2e-6, err_msg=k)
        else:
            assert np.array_equal(v.cpu().numpy(), g["step1:" + k]), k
    out = validate_steps(net, [batch])
    np.testing.assert_allclose(out["val_loss"], g["val_total"], rtol=1e-4)
    assert net.training
    assert sorted(out) == sorted(["val_loss"] + list(net.val_metrics))
    if C.CONFIGS[name][1] == 2:     # (a multi-class ``average="none"`` test metric is a vector and
        out = test_steps(net, [batch])          # goes through ``log_metrics_end_epoch`` instead)
        np.testing.assert_allclose(out["test_loss"], g["val_total"], rtol=1e-4)
    with torch.no_grad():
        loss, prediction = net.eval().test_step(batch, 0)
    assert rel(prediction, g["val_logits"]) < 1e-4
    net.train()
    if name in C.GP_NETS:
        check_gaussian_process(net, g, batch, name, cuda)


def test_steps_read_nothing_on_the_host(cuda):
    """``training_step`` (and its backward), the precision update and ``predict_step_gp`` after the
    fit under torch's synchronisation check."""
    name = "gen2d_gp32"
    net, g, batch = build_step(name, cuda)
    net.fit_gaussian_process([{"image": batch["image"]}])
    head = net.gaussian_process_head
    eps = dev(C.predict_eps(*g["gp:gp_mean"].shape), cuda)
    phi = dev(phi_batches((4, 10, 32, 3))[0], cuda)
    prob = torch.softmax(torch.randn((4, 3), device=cuda), 1)

    def run():
        net.train()
        net.zero_grad()
        loss = net.training_step(batch, 0)
        loss.backward()
        head.update_inv_cov_from_phi(phi, prob)
        head.update_inv_cov_from_phi(phi, prob, use_momentum=True)
        net.eval()
        out = net.predict_step_gp(batch, 0, n_samples=C.PREDICT_SAMPLES, eps=eps)
        return loss.detach(), head.weights.grad.clone(), out["predictive_std"], out["gp_samples"]

    run()                                   # allocator warm-up, running statistics
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(bool(torch.isfinite(t).all()) for t in second)
