"""Deconfounded classification on the GPU: the three kernels of csrc/deconfound.hip against the fp64
restatements of tests/deconfounded_ref.py (bound: ``SUM_BOUND`` = 5e-5 of the largest reference
magnitude; tools/make_deconfounded_golden.py measured the reference's own fp32 error at these shapes
below 5e-7 and tests/test_deconfounded.py pins the restatements to the reference's recorded results),
every kernel result computed twice and compared bit for bit; then the two fixture networks against
the reference's recorded step at the step tolerances of the classification tests."""
import numpy as np
import pytest
import torch

import deconfounded_cases as C
import deconfounded_ref as R
from cases import grad_rel_err
from classification_cases import zero_dropout
from test_deconfounded import build_pl

pytestmark = pytest.mark.gpu

BOUND = C.bounds()["kernels"]


def rel(got, ref):
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else got
    return R.rel(got, ref)


def twice(fn):
    """fn() two times; every tensor of the results must be bit-identical. Returns the first."""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert (u is None and v is None) or torch.equal(u, v) or (
            torch.isnan(u).any() and torch.equal(torch.isnan(u), torch.isnan(v))
            and torch.equal(torch.nan_to_num(u), torch.nan_to_num(v)))
    return a


# ---- correlation loss --------------------------------------------------------------------------------------
def corr_run(cuda, x, n):
    from adell_mri_amd import functional as HF

    def run():
        t = torch.from_numpy(x).to(cuda).requires_grad_(True)
        loss = HF.deconf_correlation_loss(t, n)
        loss.backward()
        return loss.detach(), t.grad

    return twice(run)


@pytest.mark.parametrize("case", C.CORR_CASES)
def test_correlation_loss_and_gradient(cuda, case):
    B, F, n = case
    x = C.corr_input(B, F, n)
    want_loss, want_grad = R.correlation_loss_and_grad(x, n)
    loss, grad = corr_run(cuda, x, n)
    assert loss.shape == () and grad.shape == (B, F)
    e_loss, e_grad = abs(loss.item() - want_loss) / want_loss, rel(grad, want_grad)
    print(f"corr {case}: loss {e_loss:.2e}, gradient {e_grad:.2e}")
    assert e_loss < BOUND["corr_loss"]["bound"] and e_grad < BOUND["corr_grad"]["bound"]
    assert bool(torch.isfinite(grad).all())
    zero = C.corr_zero_columns(B, F, n)
    assert (F >= 24) == bool(zero)
    assert bool((grad[:, zero] == 0).all())              # exactly 0, not small


def test_correlation_loss_on_the_clamps_edge(cuda):
    """Two items: every r is +-1. The loss is 1; the gradient is finite (its values are
    ill-conditioned in any precision and are not compared)."""
    B, F, n = C.CORR_EDGE
    loss, grad = corr_run(cuda, C.corr_input(B, F, n), n)
    assert abs(loss.item() - 1.0) < BOUND["corr_loss"]["bound"]
    assert bool(torch.isfinite(grad).all())


def test_correlation_loss_of_a_duplicated_column(cuda):
    from adell_mri_amd import functional as HF

    B, F, n = C.CORR_DUP
    x = C.dup_input()
    want = R.correlation_loss_and_grad(x, n)[0]
    t = torch.from_numpy(x).to(cuda)
    a, b = HF.deconf_correlation_loss(t, n), HF.deconf_correlation_loss(t, n)
    assert torch.equal(a, b) and abs(a.item() - want) / want < BOUND["corr_loss"]["bound"]


def test_correlation_loss_gradient_routing(cuda):
    """Only ``features`` requires a gradient (scaled by the upstream gradient); with none, no
    graph."""
    from adell_mri_amd import functional as HF

    B, F, n = 5, 24, 8
    x = C.corr_input(B, F, n)
    _, want = R.correlation_loss_and_grad(x, n)
    t = torch.from_numpy(x).to(cuda).requires_grad_(True)
    (HF.deconf_correlation_loss(t, n) * 3.0).backward()
    assert rel(t.grad, 3.0 * want) < BOUND["corr_grad"]["bound"]
    plain = HF.deconf_correlation_loss(torch.from_numpy(x).to(cuda), n)
    assert not plain.requires_grad and plain.grad_fn is None
    # a strided view is made dense, never read through its strides
    wide = torch.from_numpy(np.concatenate([x, x], 1)).to(cuda)
    assert torch.equal(HF.deconf_correlation_loss(wide[:, :F], n), plain)


# ---- heads loss ------------------------------------------------------------------------------------------
def heads_run(cuda, case, n, conf_mult, labels=None):
    from adell_mri_amd import functional as HF

    x, cat, lab, cont, target = case
    lab = lab if labels is None else labels

    def run():
        leaf = lambda a: torch.from_numpy(a).to(cuda).requires_grad_(True)  # noqa: E731
        xt = leaf(x)
        heads = [(leaf(W), leaf(b)) for W, b in cat]
        chead = None if cont is None else (leaf(cont[0]), leaf(cont[1]))
        table = torch.from_numpy(lab).to(cuda) if cat else None
        tgt = None if target is None else torch.from_numpy(target).to(cuda)
        cl, rl = HF.deconf_heads_loss(xt, n, heads, table, chead, tgt, conf_mult)
        sum(v for v in (cl, rl) if v is not None).backward()
        grads = [xt.grad] + [t.grad for pair in heads for t in pair] + \
            ([t.grad for t in chead] if chead else [])
        return [None if cl is None else cl.detach(), None if rl is None else rl.detach()] + grads

    return twice(run)


def check_heads(out, want, n_cat, has_cont, bound_loss, bound_grad):
    cat_loss, cont_loss, grads = want
    for got, ref in ((out[0], cat_loss), (out[1], cont_loss)):
        assert (got is None) == (ref is None)
        if ref is not None:
            assert got.shape == () and abs(got.item() - ref) / abs(ref) < bound_loss
    keys = ["x"] + [f"{k}{h}" for h in range(n_cat) for k in ("W", "b")] + (["Wc", "bc"] if has_cont else [])
    worst = 0.0
    for got, k in zip(out[2:], keys):
        assert got is not None and tuple(got.shape) == grads[k].shape, k
        worst = max(worst, rel(got, grads[k]))
        assert rel(got, grads[k]) < bound_grad, k
    return worst


@pytest.mark.parametrize("heads", list(C.HEADS))
@pytest.mark.parametrize("n", C.HEAD_NCONF)
@pytest.mark.parametrize("B", C.HEAD_B)
def test_heads_loss(cuda, B, n, heads):
    from adell_mri_amd import functional as HF

    classes, n_cont = C.HEADS[heads]
    assert HF.deconf_route(n, classes, n_cont) == "fused"
    for conf_mult in (1.0, 0.5):
        case = C.heads_case(B, n + 3, n, classes, n_cont)
        want = R.heads_losses(case[0], n, case[1], case[2], case[3], case[4], conf_mult)
        out = heads_run(cuda, case, n, conf_mult)
        worst = check_heads(out, want, len(classes), n_cont > 0, BOUND["heads_loss"]["bound"],
                            BOUND["heads_grad"]["bound"])
        assert bool((out[2][:, n:] == 0).all())          # the other columns take no gradient
    print(f"heads {heads} B {B} n {n}: worst gradient {worst:.2e}")


def test_heads_loss_with_a_label_out_of_range(cuda):
    """The item is NaN and the label is never used as an index: everything else stays what it was."""
    B, n = 5, 8
    classes, n_cont = C.HEADS["both"]
    case = C.heads_case(B, n + 3, n, classes, n_cont)
    for bad in (5, -1, 2 ** 40):
        labels = case[2].copy()
        labels[1, 3] = bad
        out = heads_run(cuda, case, n, 1.0, labels)
        want = R.heads_losses(case[0], n, case[1], labels, case[3], case[4])
        assert bool(torch.isnan(out[0])) and np.isnan(want[0])
        assert abs(out[1].item() - want[1]) / want[1] < BOUND["heads_loss"]["bound"]
        dx, dW0, dW1 = out[2], out[3], out[5]
        assert bool(torch.isnan(dx[3, :n]).all()) and bool(torch.isfinite(dx[[0, 1, 2, 4]]).all())
        assert bool(torch.isnan(dW1).all()) and rel(dW0, want[2]["W0"]) < BOUND["heads_grad"]["bound"]
        for got, k in zip(out[7:], ("Wc", "bc")):
            assert rel(got, want[2][k]) < BOUND["heads_grad"]["bound"]


@pytest.mark.parametrize("which", list(C.HEADS_BEYOND))
def test_heads_loss_beyond_the_fused_limits(cuda, which):
    """Just beyond each limit the composed route (split_columns, linear, cross_entropy, mse_loss)
    gives the same values, at the same bound: the f16x3 GEMM of ``linear`` drops terms of 2^-22
    relative, a tenth of SUM_BOUND."""
    from adell_mri_amd import functional as HF

    n, classes, n_cont = C.HEADS_BEYOND[which]
    assert HF.deconf_route(n, classes, n_cont) == "composed"
    B = 5
    case = C.heads_case(B, n + 3, n, classes, n_cont, tag="beyond")
    want = R.heads_losses(case[0], n, case[1], case[2], case[3], case[4], 0.5)
    out = heads_run(cuda, case, n, 0.5)
    worst = check_heads(out, want, len(classes), n_cont > 0, C.SUM_BOUND, C.SUM_BOUND)
    print(f"beyond {which}: worst gradient {worst:.2e}")


def test_heads_loss_gradient_routing(cuda):
    """Only ``features`` requires a gradient; only one of the two losses is used."""
    from adell_mri_amd import functional as HF

    B, n = 5, 8
    classes, n_cont = C.HEADS["both"]
    x, cat, lab, cont, target = C.heads_case(B, n + 3, n, classes, n_cont)
    dev = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    heads, chead = [(dev(W), dev(b)) for W, b in cat], (dev(cont[0]), dev(cont[1]))
    xt = dev(x).requires_grad_(True)
    cl, rl = HF.deconf_heads_loss(xt, n, heads, dev(lab), chead, dev(target))
    cl.backward()                                        # the regression loss is not used
    want = R.heads_losses(x, n, cat, lab, None, None)
    assert rel(xt.grad, want[2]["x"]) < BOUND["heads_grad"]["bound"]
    with torch.no_grad():
        cl2, rl2 = HF.deconf_heads_loss(xt, n, heads, dev(lab), chead, dev(target))
    assert torch.equal(cl2, cl.detach()) and torch.equal(rl2, rl.detach()) and not cl2.requires_grad


# ---- split_columns -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.SPLIT_CASES)
def test_split_columns(cuda, case):
    from adell_mri_amd import functional as HF

    B, F, n = case
    x = torch.from_numpy(C.uniform(f"split:{case}", (B, F))).to(cuda)
    da = torch.from_numpy(C.uniform(f"split:da:{case}", (B, n))).to(cuda)
    db = torch.from_numpy(C.uniform(f"split:db:{case}", (B, F - n))).to(cuda)
    for use_a, use_b in ((True, True), (True, False), (False, True)):
        t = x.clone().requires_grad_(True)
        a, b = HF.split_columns(t, n)
        assert a.is_contiguous() and b.is_contiguous()
        assert torch.equal(a, x[:, :n]) and torch.equal(b, x[:, n:])
        ref = x.clone().requires_grad_(True)
        ra, rb = ref[:, :n].contiguous(), ref[:, n:].contiguous()
        total = sum(((o * g).sum() for o, g, use in ((a, da, use_a), (b, db, use_b)) if use))
        rtotal = sum(((o * g).sum() for o, g, use in ((ra, da, use_a), (rb, db, use_b)) if use))
        total.backward()
        rtotal.backward()
        assert torch.equal(t.grad, ref.grad)
    assert not HF.split_columns(x, n)[0].requires_grad


# ---- networks --------------------------------------------------------------------------------------------
def build_step(name, cuda, **extra):
    g = C.StepGold(name)
    net = build_pl(name, **extra)
    assert zero_dropout(net) == list(g["dropout_rates"])
    net.load_state_dict(C.fill(net.state_dict(), float(g["gain"])))
    net = net.to(cuda).train()
    batch = {"image": torch.from_numpy(g["x"]).to(cuda), "label": torch.tensor(C.NETS[name][2]).to(cuda),
             "cat": [list(item) for item in C.NETS[name][3]]}
    if C.NETS[name][4] is not None:
        batch["cont"] = torch.tensor(C.NETS[name][4])
    return net, g, batch


@pytest.mark.parametrize("name", list(C.NETS))
def test_training_step_matches_reference(cuda, name):
    """``step`` and ``training_step`` in ``train()`` mode: the four loss terms, the logits, every
    parameter gradient, one FusedAdam step over the two groups (a non-zero weight decay: AdamW
    would miss), the buffers; then ``validation_step`` in ``eval()`` mode with its metric counts,
    and ``predict_step``."""
    from adell_mri_amd.optim import FusedAdam
    from adell_mri_amd.trainer import StepRunner, validate_steps

    net, g, batch = build_step(name, cuda)
    assert net.heads_route() == ("fused" if name == "a" else "composed")
    runner = StepRunner(net)
    assert type(runner.optimizer) is FusedAdam
    runner.optimizer.zero_grad()
    out = net.step(batch, with_loss_params=True)
    assert len(out) == 6 and out[5] is batch["label"]
    terms = dict(zip(net.loss_str, out[:4]))
    for k, v in terms.items():
        assert (v is None) == (k not in g.files), k
        if v is not None:
            np.testing.assert_allclose(v.item(), g[k], rtol=C.TOL["loss"], err_msg=k)
    logits = torch.squeeze(out[4], 1)
    assert logits.shape == g["logits"].shape and rel(logits, g["logits"]) < C.TOL["loss"]
    loss = sum(v for v in out[:4] if v is not None)
    np.testing.assert_allclose(loss.item(), g["total"], rtol=C.TOL["loss"])
    loss.backward()
    params = dict(net.named_parameters())
    want = [k[5:] for k in g.files if k.startswith("grad:")]
    worst = 0.0
    for k, p in params.items():
        assert (p.grad is not None) == (k in want), k     # the extractor's own head takes no part
        if p.grad is not None:
            e = grad_rel_err(g, k, p.grad.cpu().numpy())
            worst = max(worst, e)
            assert e < C.TOL["grad"], (k, e)
    print(f"{name}: worst gradient {worst:.2e}")
    runner.optimizer.step()
    for k, v in net.state_dict().items():
        if ".feature_extraction." in k:
            continue                                       # CatNet: the same tensors as ``res_net.*``
        if v.is_floating_point():
            np.testing.assert_allclose(v.detach().cpu().numpy(), g["step1:" + k],
                                       rtol=C.TOL["param"][0], atol=C.TOL["param"][1], err_msg=k)
        else:
            assert np.array_equal(v.cpu().numpy(), g["step1:" + k]), k
    # validation: eval mode, the running statistics the step left
    net.eval()
    with torch.no_grad():
        vout = net.step(batch, with_loss_params=False)
        for k, v in zip(net.loss_str, vout[:4]):
            if v is not None:
                np.testing.assert_allclose(v.item(), g["val_" + k], rtol=C.TOL["loss"], err_msg=k)
        vlogits = torch.squeeze(vout[4], 1)
        assert rel(vlogits, g["val_logits"]) < C.TOL["loss"]
        feats = net.predict_step(batch, 0, return_features=True)["features"]
        assert rel(feats, g["features"]) < C.TOL["loss"]
        pred = net.predict_step(batch, 0)["prediction"]
        assert torch.equal(pred, vlogits)
    net.train()
    res = validate_steps(net, [batch])
    np.testing.assert_allclose(res["val_loss"], g["val_total"], rtol=C.TOL["loss"])
    assert net.training
    # the metric counts: the confusion matrix of the wrapper's own predictions
    labels = np.array(C.NETS[name][2])
    if name == "a":
        hard = (torch.sigmoid(vlogits.double()) > 0.5).long().cpu().numpy()
    else:
        hard = vlogits.argmax(1).cpu().numpy()
    recall = np.mean([np.mean(hard[labels == c] == c) for c in np.unique(labels)]) if name == "b" \
        else np.mean(hard[labels == 1] == 1)
    assert set(res) > {"val_loss", "V_Rec"}
    np.testing.assert_allclose(res["V_Rec"], recall, rtol=2e-7, atol=1e-9)


def test_fit_and_validate_steps(cuda):
    from adell_mri_amd.trainer import fit_steps, test_steps, validate_steps

    net, g, batch = build_step("a", cuda)
    losses = fit_steps(net, [batch, batch])
    assert len(losses) == 2 and all(bool(torch.isfinite(v)) for v in losses)
    np.testing.assert_allclose(losses[0].item(), g["total"], rtol=C.TOL["loss"])
    assert losses[1].item() != losses[0].item()
    for res, key in ((validate_steps(net, [batch]), "val_loss"), (test_steps(net, [batch]), "test_loss")):
        assert all(np.isfinite(v) or k.endswith("AUC") for k, v in res.items()) and np.isfinite(res[key])


def test_tensor_tables_and_routes_agree(cuda):
    """A categorical entry that is already the int64 [n_heads, B] device table gives the same bits as
    the embedder's; the composed route (a CPU-free check: ``heads_route`` forced) the same values."""
    net, g, batch = build_step("a", cuda)
    with torch.no_grad():
        a = net.step(batch, False)
        table = dict(batch, cat=torch.from_numpy(C.cat_table("a")).to(cuda), cont=batch["cont"].to(cuda))
        b = net.step(table, False)
        net.heads_route = lambda device=None: "composed"
        c = net.step(batch, False)
    for u, v, w in zip(a[:5], b[:5], c[:5]):
        assert torch.equal(u, v)
        np.testing.assert_allclose(w.cpu().numpy(), u.cpu().numpy(), rtol=C.TOL["loss"])


def test_cosine_loss_as_written(cuda):
    net, g, batch = build_step("a", cuda)
    feats = torch.from_numpy(C.uniform("cosine", (4, 16))).to(cuda)
    n = net.n_features_deconfounder
    want = torch.nn.functional.cosine_similarity(feats.double()[:, :n, None],
                                                 feats.double()[:, None, n:]).mean()
    assert abs(net.cosine_loss(feats).item() - want.item()) < 1e-6


def test_deconfounded_step_has_no_host_read(cuda):
    """The loss part of a fused-route training step (both confounder losses and the correlation
    loss, forward and backward) with the confounder tables already on the device, under torch's
    synchronisation check."""
    net, g, batch = build_step("a", cuda)
    assert net.heads_route() == "fused"
    batch = dict(batch, cat=torch.from_numpy(C.cat_table("a")).to(cuda), cont=batch["cont"].to(cuda))
    with torch.no_grad():
        feats = net(batch["image"], return_features=True).detach()

    def run():
        net.zero_grad()
        leaf = feats.clone().requires_grad_(True)
        cat, cont = net.fused_confounder_losses(batch, leaf)
        total = cat + cont + net.loss_features(leaf)
        total.backward()
        return total.detach(), leaf.grad, net.confound_regressions.op[-1].weight.grad.clone()

    first = run()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for u, v in zip(first, second):
        assert torch.equal(u, v)
    np.testing.assert_allclose(first[0].item(), float(g["cat_loss"]) + float(g["cont_loss"])
                               + float(g["feat_loss"]), rtol=C.TOL["loss"])
