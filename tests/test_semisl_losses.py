"""Semi-supervised losses beyond LocalContrastiveLoss, without a GPU: the helpers, the signatures, the
three modules on CPU tensors (the composite route) and the queue script against the fixtures of the
real reference (tools/make_semisl_losses_golden.py), the raiser, the routes, and the fp64 restatements
of tests/semisl_losses_ref.py against the same fixtures and against torch's cosine."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import semisl_losses_cases as C
import semisl_losses_ref as R
from adell_mri_amd import functional as HF
from adell_mri_amd.modules import semi_supervised_segmentation as SS
from adell_mri_amd.modules.semi_supervised_segmentation import losses as L

GOLD = C.GOLD


@pytest.fixture(scope="module")
def surface():
    with open(os.path.join(GOLD, "semisl_losses_surface.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def bounds():
    return C.bounds()


def _params(fn):
    return [[p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
            for p in inspect.signature(fn).parameters.values()]


# ---- helpers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(2, 10))
def test_derangement_matches_the_recorded_permutation(surface, n):
    perm = L.derangement(n, seed=0)
    assert perm == surface["derangement_seed0"][str(n)]
    assert sorted(perm) == list(range(n)) and all(p != i for i, p in enumerate(perm))


@pytest.mark.parametrize("n", [1, 0, -3])
def test_derangement_needs_two_elements(n):
    with pytest.raises(ValueError, match="at least 2"):
        L.derangement(n)


def test_derangement_draws_choice_of_range_in_order():
    rng, probe = np.random.default_rng(5), np.random.default_rng(5)
    xs = list(range(6))
    for a in range(1, 6):
        L.swap(xs, a, probe.choice(range(a)))
    assert L.derangement(6, rng=rng) == xs
    assert rng.random() == probe.random()       # the same number of draws


def test_anchors_from_derangement_is_the_loop_and_stack():
    X = torch.randn(5, 3, 4, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    got = L.anchors_from_derangement(X, np.random.default_rng(3))
    perm = L.derangement(5, rng=np.random.default_rng(3))
    want = torch.stack([X[i] for i in perm])
    assert torch.equal(got, want)
    w = torch.arange(60.0).reshape(5, 3, 4)
    g1, = torch.autograd.grad((got * w).sum(), X)
    g2, = torch.autograd.grad((want * w).sum(), X)
    assert torch.equal(g1, g2)


# ---- surface ----------------------------------------------------------------------------------------------
def test_signatures_equal_the_reference(surface):
    for name, want in surface["functions"].items():
        assert _params(getattr(L, name)) == want, name
    for cls, methods in surface["classes"].items():
        assert hasattr(SS, cls), cls
        if cls == "AnatomicalContrastiveLoss":
            continue                                # a raiser: see its test
        for name, want in methods.items():
            assert _params(getattr(getattr(L, cls), name)) == want, (cls, name)


def test_attributes_follow_the_reference():
    m = L.LocalContrastiveLossWithAnchors(0.2, seed=3)
    assert m.temperature == 0.2 and m.seed == 3 and float(m.eps) == pytest.approx(1e-8)
    assert isinstance(m.rng, np.random.Generator)
    n = L.NearestNeighbourLoss(**C.NN_ARGS)
    assert len(n.q) == 3 and all(q.maxsize == 16 for q in n.q) and len(n) == 0
    p = L.PseudoLabelCrossEntropy(0.5, weight=torch.ones(3), label_smoothing=0.1)
    assert isinstance(p.ce, torch.nn.CrossEntropyLoss) and p.threshold == 0.5
    assert list(p.state_dict()) == ["ce.weight"] and p.ce.label_smoothing == 0.1


def test_anatomical_contrastive_loss_raises_with_its_reason():
    with pytest.raises(NotImplementedError, match="backward of the second"):
        L.AnatomicalContrastiveLoss(n_classes=3, n_features=8, batch_size=2)


# ---- the modules on CPU tensors: the composite route ------------------------------------------------------
def _anchor_module_run(tag, device="cpu"):
    case = C.ANCHOR_CASES[tag]
    x, a1, a2, r = (torch.from_numpy(v).to(device) for v in C.anchor_inputs(tag))
    x.requires_grad_(True)
    mod = L.LocalContrastiveLossWithAnchors(case["temperature"], seed=case.get("seed", 42))
    if case["anchors"] == "given":
        a1.requires_grad_(True)
        a2.requires_grad_(True)
        loss = mod(x, a1, a2)
    elif case["anchors"] == "drawn":
        loss = mod(x)
    else:
        a1.requires_grad_(True)
        loss = mod(x, a1)
    (loss * r).sum().backward()
    return loss, {"x": x.grad, "a1": a1.grad, "a2": a2.grad}


def check_anchor_against_fixture(tag, loss, grads, table):
    g = np.load(os.path.join(GOLD, "semisl_losses_anchor.npz"))
    ref = g[f"{tag}:value"]
    got = loss.detach().cpu().numpy()
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    print(tag, "value err", err.max())
    assert (err <= C.value_tol(f"anchor:{tag}:value", ref, table)).all(), (tag, err)
    for k in ("x", "a1", "a2"):
        key = f"{tag}:grad_{k}"
        if key not in g.files:
            assert grads[k] is None, (tag, k)
            continue
        got = C.grad_sample(grads[k].detach().cpu().numpy())
        e = float(np.abs(got - g[key]).max())
        print(tag, k, "grad err", e, "of", float(np.abs(g[key]).max()))
        assert e <= C.grad_tol(f"anchor:{tag}:grad_{k}", g[key], table), (tag, k, e)


@pytest.mark.parametrize("tag", list(C.ANCHOR_CASES))
def test_anchor_loss_on_cpu_matches_fixture(tag, bounds):
    loss, grads = _anchor_module_run(tag)
    check_anchor_against_fixture(tag, loss, grads, bounds)


@pytest.mark.parametrize("tag", ["e", "f"])
def test_anchor_derangement_cases_draw_the_recorded_permutations(tag):
    g = np.load(os.path.join(GOLD, "semisl_losses_anchor.npz"))
    case = C.ANCHOR_CASES[tag]
    rng = np.random.default_rng(case["seed"])
    perms = [L.derangement(case["shape"][0], rng=rng) for _ in range(len(g[f"{tag}:perms"]))]
    assert np.array_equal(np.asarray(perms), g[f"{tag}:perms"])


def _queue_rows(mod):
    return [[e for e in q.queue] for q in mod.q]


def check_queue(mod, g, key, device="cpu"):
    assert len(mod) == int(g[f"{key}:len"]), key
    for cl, entries in enumerate(_queue_rows(mod)):
        assert len(entries) == int(g[f"{key}:q{cl}:n"]), (key, cl)
        for k, e in enumerate(entries):
            assert not e.requires_grad and e.device.type == device
            assert np.array_equal(e.cpu().numpy(), g[f"{key}:q{cl}:{k}"]), (key, cl, k)


def run_nn_script(device, table):
    """The recorded put / forward script on ``device``; returns (loss, dX)."""
    g = np.load(os.path.join(GOLD, "semisl_losses_nn.npz"))
    mod = L.NearestNeighbourLoss(**C.NN_ARGS)
    for i in range(C.NN_PUTS):
        X, y = (torch.from_numpy(v).to(device) for v in C.nn_put_inputs(i))
        mod.put(X.requires_grad_(True), y)
        check_queue(mod, g, f"put{i}", torch.device(device).type)
    X, y = (torch.from_numpy(v).to(device) for v in C.nn_forward_inputs())
    X.requires_grad_(True)
    loss = mod(X, y)
    assert loss.dim() == 0
    loss.backward()
    check_queue(mod, g, "fwd", torch.device(device).type)
    err = abs(float(loss.detach()) - float(g["fwd:value"]))
    gerr = float(np.abs(X.grad.cpu().numpy() - g["fwd:grad"]).max())
    print("nn value err", err, "grad err", gerr, "of", float(np.abs(g["fwd:grad"]).max()))
    assert err <= C.value_tol("nn:value", g["fwd:value"], table)
    assert gerr <= C.grad_tol("nn:grad", g["fwd:grad"], table)
    return loss, X.grad


def test_nearest_neighbour_script_on_cpu(bounds):
    run_nn_script("cpu", bounds)


def test_nearest_neighbour_empty_queue_returns_zero():
    g = np.load(os.path.join(GOLD, "semisl_losses_nn.npz"))
    mod = L.NearestNeighbourLoss(**C.NN_ARGS)
    X, y = (torch.from_numpy(v) for v in C.nn_forward_inputs())
    out = mod(X, y)
    assert out.dim() == 0 and float(out) == float(g["empty:value"]) == 0.0
    samples, labels = mod.get_past_samples("cpu")
    assert samples.shape == (0,) and labels.shape == (0, 3)


def test_nearest_neighbour_past_samples_are_the_reference_pair():
    mod = L.NearestNeighbourLoss(**C.NN_ARGS)
    for i in range(2):
        X, y = (torch.from_numpy(v) for v in C.nn_put_inputs(i))
        mod.put(X, y)
    samples, labels = mod.get_past_samples("cpu")
    assert samples.shape == (6 + 6 + 4 + 4, 8) and labels.dtype == torch.int64
    assert labels.shape == (20, 3) and labels.sum(0).tolist() == [12, 8, 0]
    assert len(mod) == 0


def pl_module_run(name, device="cpu"):
    kw = dict(C.PL_CASES[name])
    if "weight" in kw:
        kw["weight"] = torch.tensor(kw["weight"])
    mod = L.PseudoLabelCrossEntropy(C.PL_THRESHOLD, **kw).to(device)
    pred, proba = (torch.from_numpy(v).to(device) for v in C.pl_inputs())
    pred.requires_grad_(True)
    loss = mod(pred, proba)
    loss.backward()
    return loss, pred.grad


def check_pl_against_fixture(name, loss, grad, table):
    g = np.load(os.path.join(GOLD, "semisl_losses_pl.npz"))
    assert np.array_equal(g["pred"], C.pl_inputs()[0]) and np.array_equal(g["proba"], C.pl_inputs()[1])
    err = abs(float(loss.detach()) - float(g[f"{name}:value"]))
    gerr = float(np.abs(grad.detach().cpu().numpy() - g[f"{name}:grad"]).max())
    print(name, "value err", err, "grad err", gerr, "of", float(np.abs(g[f"{name}:grad"]).max()))
    assert err <= C.value_tol(f"pl:{name}:value", g[f"{name}:value"], table)
    assert gerr <= C.grad_tol(f"pl:{name}:grad", g[f"{name}:grad"], table)


@pytest.mark.parametrize("name", list(C.PL_CASES))
def test_pseudo_label_ce_on_cpu_matches_fixture(name, bounds):
    loss, grad = pl_module_run(name)
    assert loss.dim() == 0
    check_pl_against_fixture(name, loss, grad, bounds)


# ---- routes -----------------------------------------------------------------------------------------------
def test_semisl_route_at_and_past_each_limit():
    assert HF.semisl_route("anchor", C=4) == "fused"
    assert HF.semisl_route("anchor", C=1024) == "fused"
    assert HF.semisl_route("anchor", C=1028) == "composed"
    assert HF.semisl_route("anchor", C=6) == "composed"
    assert HF.semisl_route("nn", C=64, K=64) == "fused"
    assert HF.semisl_route("nn", C=68, K=2) == "composed"
    assert HF.semisl_route("nn", C=10, K=2) == "composed"
    assert HF.semisl_route("nn", C=8, K=65) == "composed"
    assert HF.semisl_route("pseudo_label", K=64) == "fused"
    assert HF.semisl_route("pseudo_label", K=65) == "composed"
    assert HF.semisl_route("pseudo_label", K=3, reduction="sum") == "fused"
    assert HF.semisl_route("pseudo_label", K=3, reduction="none") == "composed"
    assert HF.semisl_route("pseudo_label", K=3, ignore_index=0) == "composed"
    with pytest.raises(ValueError, match="kind"):
        HF.semisl_route("anatomical")


# ---- the restatements -------------------------------------------------------------------------------------
def test_cosine_restatement_equals_torch_with_a_zero_vector():
    g = torch.Generator().manual_seed(2)
    a = torch.randn(3, 6, 11, generator=g, dtype=torch.float64)
    b = torch.randn(3, 6, 11, generator=g, dtype=torch.float64)
    a[0, :, 3] = 0.0
    b[1, :, 5] = 0.0
    a[2, :, 7] = 0.0
    b[2, :, 7] = 0.0
    w = torch.randn(3, 11, generator=g, dtype=torch.float64)
    outs = []
    for fn in (lambda u, v: R.cosine(u, v, 1),
               lambda u, v: torch.nn.functional.cosine_similarity(u, v, dim=1, eps=1e-8)):
        u, v = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        c = fn(u, v)
        (c * w).sum().backward()
        outs.append((c.detach(), u.grad, v.grad))
    for got, want in zip(*outs):
        assert torch.isfinite(want).all()
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert float(outs[0][0][0, 3]) == 0.0


@pytest.mark.parametrize("tag", [t for t, c in C.ANCHOR_CASES.items() if c["anchors"] == "given"])
def test_anchor_restatement_matches_fixture(tag):
    g = np.load(os.path.join(GOLD, "semisl_losses_anchor.npz"))
    x, a1, a2, r = (torch.from_numpy(v) for v in C.anchor_inputs(tag))
    loss, dx, da1, da2 = R.anchor_loss_and_grads(x, a1, a2, r, C.ANCHOR_CASES[tag]["temperature"])
    np.testing.assert_allclose(loss.numpy(), g[f"{tag}:value"], rtol=1e-11, atol=1e-12)
    for k, d in (("x", dx), ("a1", da1), ("a2", da2)):
        ref = g[f"{tag}:grad_{k}"]
        assert np.abs(C.grad_sample(d.numpy()) - ref).max() <= 1e-10 * np.abs(ref).max()


def test_nn_restatement_matches_fixture():
    g = np.load(os.path.join(GOLD, "semisl_losses_nn.npz"))
    mod = L.NearestNeighbourLoss(**C.NN_ARGS)
    for i in range(C.NN_PUTS):
        X, y = (torch.from_numpy(v) for v in C.nn_put_inputs(i))
        mod.put(X, y)
    past, classes = mod._past_samples()
    X, y = (torch.from_numpy(v) for v in C.nn_forward_inputs())
    loss, dx = R.nn_loss_and_grad(X, y, past, torch.from_numpy(classes), C.NN_ARGS["temperature"])
    np.testing.assert_allclose(float(loss), float(g["fwd:value"]), rtol=1e-11)
    assert np.abs(dx.numpy() - g["fwd:grad"]).max() <= 1e-10 * np.abs(g["fwd:grad"]).max()


@pytest.mark.parametrize("name", list(C.PL_CASES))
def test_pseudo_label_restatement_matches_fixture(name):
    g = np.load(os.path.join(GOLD, "semisl_losses_pl.npz"))
    pred, proba = (torch.from_numpy(v) for v in C.pl_inputs())
    loss, d = R.pseudo_label_ce_and_grad(pred, proba, C.PL_THRESHOLD, **C.PL_CASES[name])
    np.testing.assert_allclose(float(loss), float(g[f"{name}:value"]), rtol=1e-12)
    assert np.abs(d.numpy() - g[f"{name}:grad"]).max() <= 1e-11 * np.abs(g[f"{name}:grad"]).max()
