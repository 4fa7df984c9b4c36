"""Classification on the GPU: the kernels of csrc/classify.hip against the fp64 restatements
(tests/classification_ref.py), every kernel result computed twice and compared bit for bit; the
metrics; one training step and a following validation step of the five fixture networks against the
real reference (tests/golden/classification_step_*.npz), and the test loop on a wrapper whose
``test_step`` returns a tuple.

Tolerances are the project's for the same kinds of quantity (tests/test_mae_gpu.py): bit equality
for copies (mixup: torch's own three-operation expression), 5e-5 of the largest reference magnitude
for fixed-order sums and losses; in the step tests loss 1e-4, gradients 5e-3 by
``cases.grad_rel_err``, parameters (2e-4, 2e-6) -- the fixture's own fp32-against-fp64 error uses at
most a quarter of them (recorded as ``<net>:fp32_vs_fp64``); integer counts and the AUROC pair
counts exact. Metric values are fp64 results rounded to fp32: 2e-7 relative."""
import numpy as np
import pytest
import torch

import classification_ref as CR
from cases import grad_rel_err
from classification_cases import CONFIGS, NETS, StepGold, fill
from test_classification import build_pl, inner

pytestmark = pytest.mark.gpu

SUM_BOUND = 5e-5


def rel(a, r):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a).double()
    r = r.detach().double().cpu() if isinstance(r, torch.Tensor) else torch.as_tensor(r).double()
    return float((a - r).abs().max() / (r.abs().max() + 1e-300))


def twice(fn):
    """fn() run two times: the first result, after asserting that the second is bit-identical
    (NaNs at the same places)."""
    a, b = fn(), fn()
    a_, b_ = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    for u, v in zip(a_, b_):
        assert torch.equal(torch.nan_to_num(u, nan=12345.0), torch.nan_to_num(v, nan=12345.0)), \
            "two runs differ"
        assert torch.equal(torch.isnan(u), torch.isnan(v))
    return a


def logits_for(B, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, W), generator=g) * 8 - 4
    x[0, 0], x[-1, -1] = 90.0, -90.0
    if B > 2:
        x[1, W // 2] = -90.0 if W > 1 else 90.0
    return x


# ---- losses ------------------------------------------------------------------------------------------
def _check_loss(cuda, kind, x, y, w, K):
    """Forward and both backwards of one case against the restatement."""
    from adell_mri_amd import functional as HF

    B = x.shape[0]
    fn = {"bce": lambda xd, red: HF.bce_with_logits(xd[:, 0], y.to(cuda), wd, reduction=red),
          "ce": lambda xd, red: HF.cross_entropy(xd, y.to(cuda), wd, reduction=red),
          "ordinal": lambda xd, red: (HF.ordinal_sigmoidal_loss(xd, y.to(cuda), K, wd).mean()
                                      if red == "mean" else
                                      HF.ordinal_sigmoidal_loss(xd, y.to(cuda), K, wd))}[kind]
    wd = None if w is None else w.to(cuda)
    gi = torch.linspace(-1.0, 2.0, B)

    def run():
        xd = x.to(cuda).requires_grad_(True)
        red = fn(xd, "mean")
        (red * 0.37).backward()                    # an incoming gradient other than 1
        xi = x.to(cuda).requires_grad_(True)
        item = fn(xi, "none")
        item.backward(gi.to(cuda))
        return red.detach(), xd.grad, item.detach(), xi.grad

    red, dx, item, dxi = twice(run)
    xr = x[:, 0] if kind == "bce" else x
    want_item, want_red, want_dx = CR.loss(kind, xr.numpy(), y.numpy(),
                                           None if w is None else w.numpy(), K)
    _, _, want_dxi = CR.loss(kind, xr.numpy(), y.numpy(), None if w is None else w.numpy(), K,
                             g=gi.numpy())
    if kind == "ordinal":       # the wrapper's mean: what the reduced output of the kernel is
        want_red = want_item.mean()
    assert item.shape == (B,) and red.dim() == 0
    assert rel(item, want_item) < SUM_BOUND and abs(red.item() - want_red) < SUM_BOUND * abs(want_red)
    assert rel(dx.reshape(-1), 0.37 * want_dx.reshape(-1)) < SUM_BOUND
    assert rel(dxi.reshape(-1), want_dxi.reshape(-1)) < SUM_BOUND


@pytest.mark.parametrize("B", [1, 3, 64, 65, 130])
def test_bce_with_logits(cuda, B):
    g = torch.Generator().manual_seed(B)
    x = logits_for(B, 1, 10 + B)
    soft = torch.rand((B,), generator=g)                       # soft targets
    hard = (torch.rand((B,), generator=g) > 0.5).float()
    for y in (soft, hard):
        for w in (None, torch.tensor([0.7]), torch.rand((B,), generator=g) + 0.25):
            _check_loss(cuda, "bce", x, y, w, 1)


@pytest.mark.parametrize("kind", ["ce", "ordinal"])
@pytest.mark.parametrize("B", [1, 3, 64, 65, 130])
def test_losses_on_labels(cuda, kind, B):
    for K in (2, 3, 5, 33):
        g = torch.Generator().manual_seed(100 * B + K)
        W = K if kind == "ce" else K - 1
        x = logits_for(B, W, 7 * B + K)
        y = torch.randint(0, K, (B,), generator=g)
        y[0] = K - 1                                           # a class of non-zero weight below
        w = torch.rand((K,), generator=g) + 0.25
        w[0] = 0.0                                             # a class weight of zero
        for weights in (None, w):
            _check_loss(cuda, kind, x, y, weights, K)


def test_loss_modules_and_configure_loss_fn(cuda):
    from adell_mri_amd.modules.classification.losses import (BCEWithLogitsLoss, CrossEntropyLoss,
                                                             OrdinalSigmoidalLoss,
                                                             configure_loss_fn)

    cfg = {}
    configure_loss_fn(cfg, "cat", 2)
    assert isinstance(cfg["loss_fn"], BCEWithLogitsLoss) and cfg["loss_fn"].weight is None
    configure_loss_fn(cfg, "cat", 3, torch.tensor([1.0, 2.0, 0.5]))
    assert isinstance(cfg["loss_fn"], CrossEntropyLoss)
    x = logits_for(5, 3, 1)
    y = torch.tensor([0, 2, 1, 1, 2])
    got = cfg["loss_fn"](x.to(cuda), y.to(cuda))
    assert abs(got.item() - CR.loss("ce", x.numpy(), y.numpy(), [1.0, 2.0, 0.5])[1]) < SUM_BOUND * 90
    configure_loss_fn(cfg, "ord", 4, torch.tensor([1.0, 2.0, 0.5, 1.5]))
    assert isinstance(cfg["loss_fn"], OrdinalSigmoidalLoss)
    y4 = torch.tensor([0, 3, 1, 1, 2])
    pre = x[:, :1].contiguous()
    loss, roc = cfg["loss_fn"](x.to(cuda), y4.to(cuda), pre_bias=pre.to(cuda))
    assert rel(loss, CR.loss("ordinal", x.numpy(), y4.numpy(), [1.0, 2.0, 0.5, 1.5], 4)[0]) < SUM_BOUND
    assert abs(roc.item() - CR.roc(pre.numpy(), y4.numpy())[0]) < SUM_BOUND * abs(roc.item())
    assert cfg["loss_fn"](x.to(cuda), y4.to(cuda)).shape == (5,)


# ---- relative order consistency --------------------------------------------------------------------------
def _check_roc(cuda, p, y):
    from adell_mri_amd import functional as HF

    def run():
        pd = p.to(cuda).requires_grad_(True)
        loss = HF.relative_order_consistency(pd, y.to(cuda))
        (loss * 1.7).backward()
        return loss.detach(), pd.grad

    loss, dp = twice(run)
    want, want_dp, M = CR.roc(p.numpy(), y.numpy())
    assert loss.dim() == 0 and dp.shape == p.shape
    return loss, dp, want, 1.7 * want_dp, M


@pytest.mark.parametrize("B", [2, 5, 64, 65, 129])
def test_relative_order_consistency(cuda, B):
    g = torch.Generator().manual_seed(B)
    p = torch.rand((B, 1), generator=g) * 6 - 3
    p[0, 0] = 40.0
    y = torch.randint(0, 4, (B,), generator=g)
    y[0], y[-1] = 0, 3
    loss, dp, want, want_dp, M = _check_roc(cuda, p, y)
    assert M > 0 and abs(loss.item() - want) < SUM_BOUND * abs(want)
    assert rel(dp.reshape(-1), want_dp) < SUM_BOUND
    # exactly one label differs: 2 (B - 1) ordered pairs
    one = torch.zeros(B, dtype=torch.int64)
    one[B // 2] = 2
    loss, dp, want, want_dp, M = _check_roc(cuda, p, one)
    assert M == 2 * (B - 1) and abs(loss.item() - want) < SUM_BOUND * abs(want)
    assert rel(dp.reshape(-1), want_dp) < SUM_BOUND


def test_relative_order_consistency_without_pairs_is_nan(cuda):
    p = torch.tensor([[0.5], [-1.0], [2.0]])
    loss, dp, want, _, M = _check_roc(cuda, p, torch.full((3,), 2, dtype=torch.int64))
    assert M == 0 and np.isnan(want) and bool(torch.isnan(loss))
    assert bool((torch.isnan(dp) | (dp == 0)).all())           # NaN accepted


# ---- mixup ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("V", [1, 3, 4, 1023, 4100])
def test_mixup_rows_bit_equal(cuda, B, V):
    from adell_mri_amd import functional as HF

    g = torch.Generator().manual_seed(100 * B + V)
    x = torch.rand((B, V), generator=g) * 4 - 2
    factor = torch.rand((B,), generator=g)
    partner = np.roll(np.arange(B), 1)
    partner[B - 1] = B - 1                       # a row that is its own partner ...
    x[B - 1, V // 2] = float("inf")              # ... and holds an Inf
    for offset in (0, 1):                        # a view at an element offset of 1: misaligned rows
        store = torch.zeros(B * V + offset, device=cuda)
        xd = store[offset:].view(B, V)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4 * offset and xd.is_contiguous()
        out = twice(lambda: HF.mixup_rows(xd, factor, partner))
        want = CR.mixup_rows(x, factor, partner)
        assert torch.equal(out.cpu(), want)
        assert torch.equal(out[B - 1].cpu(), x[B - 1])
        if B > 1:
            direct = x[0] * factor[0] + x[partner[0]] * (1.0 - factor[0])
            assert torch.equal(out[0].cpu(), direct)
        assert torch.equal(xd.cpu(), x)          # the input is not written


def test_mixup_5d_and_bad_partner(cuda):
    from adell_mri_amd import functional as HF

    x = torch.rand((3, 2, 4, 5, 3), generator=torch.Generator().manual_seed(0))
    factor, partner = torch.tensor([0.25, 0.5, 0.9]), [2, 0, 1]
    out = HF.mixup_rows(x.to(cuda), factor, partner)
    assert out.shape == x.shape and torch.equal(out.cpu(), CR.mixup_rows(x, factor, partner))
    with pytest.raises(IndexError, match="partner outside"):
        HF.mixup_rows(x.to(cuda), factor, [0, 1, 3])


@pytest.mark.parametrize("fraction,n_selected", [(0.0, 0), (1.0, 5)])
def test_partial_mixup_none_and_all(cuda, fraction, n_selected):
    from adell_mri_amd.utils.batch_preprocessing import BatchPreprocessing, partial_mixup

    x = torch.rand((5, 3, 7), generator=torch.Generator().manual_seed(1))
    y = torch.tensor([0.0, 1.0, 1.0, 0.0, 1.0])
    rng = np.random.default_rng(3)
    selected = rng.binomial(1, fraction, 5).astype(bool)
    factor = np.ones(5)
    factor[selected] = rng.beta(0.4, 0.4, selected.sum())
    perm = rng.permutation(5)
    assert selected.sum() == n_selected
    xd, yd = x.to(cuda), y.to(cuda)
    X, Y = partial_mixup(xd, yd, 0.4, fraction, np.random.default_rng(3))
    partner = np.where(selected, perm, np.arange(5))
    assert torch.equal(X.cpu(), CR.mixup_rows(x, factor, partner))
    f32 = torch.as_tensor(factor, dtype=torch.float32)
    want_y = torch.where(torch.as_tensor(selected), y * f32 + y[perm] * (1.0 - f32), y)
    assert torch.equal(Y.cpu(), want_y)
    assert torch.equal(xd.cpu(), x) and torch.equal(yd.cpu(), y)     # new tensors
    if n_selected == 0:
        assert torch.equal(X.cpu(), x) and X.data_ptr() != xd.data_ptr()
    bp = BatchPreprocessing(None, 0.4, fraction, seed=3)
    X2, _ = bp(xd, yd)
    assert torch.equal(X2, X)


# ---- metrics ---------------------------------------------------------------------------------------------
def _close(value, want):
    np.testing.assert_allclose(value.double().cpu().numpy(), want, rtol=2e-7, atol=1e-9,
                               equal_nan=True)


@pytest.mark.parametrize("N", [1, 64, 65, 1000])
@pytest.mark.parametrize("C", [2, 3, 7])
def test_classification_metrics(cuda, N, C):
    from adell_mri_amd import classification_metrics as CM
    from adell_mri_amd import ops

    rng = np.random.default_rng(10 * N + C)
    top = C if C == 2 else C - 1                               # C > 2: the last class is absent
    labels = rng.integers(0, top, N)
    scores = (np.round(rng.random((N, C)) * 8) / 8).astype(np.float32)      # many ties
    preds = scores[:, 1].copy() if C == 2 else scores
    M, bad = CR.confusion(preds, labels, C)
    assert bad == 0
    pd, ld = torch.from_numpy(preds).to(cuda), torch.from_numpy(labels).to(cuda)
    counts = torch.zeros(C * C + 1, dtype=torch.int64, device=cuda)
    ops.cls_confusion_update(pd, ld, counts)
    assert np.array_equal(counts.cpu().numpy(), np.append(M.reshape(-1), 0))
    for average in ("macro", "none"):
        metrics = CM.get_metric_dict(C, None, prefix="V_", average=average).to(cuda)
        assert list(metrics) == ["V_Rec", "V_Spe", "V_Pr", "V_F1", "V_AUC"]
        half = N // 2
        CM.update_many(metrics.values(), pd[:half], ld[:half])             # two updates ...
        CM.update_many(metrics.values(), pd[half:], ld[half:])
        whole = CM.get_metric_dict(C, None, average=average).to(cuda)
        for m in whole.values():
            m.update(pd, ld)                                               # ... against one
        for key, kind in (("Rec", "recall"), ("Spe", "specificity"), ("Pr", "precision"),
                          ("F1", "fbeta")):
            if C == 2:
                want = CR.per_class(M, kind)[1]
            else:
                want = CR.macro(M, kind) if average == "macro" else CR.per_class(M, kind)
            got = metrics["V_" + key].compute()
            _close(got, want)
            assert torch.equal(got, whole[key].compute())
            assert torch.equal(metrics["V_" + key].state[:-1].cpu(),
                               torch.from_numpy(M.reshape(-1)))
        want_auc = CR.auroc(preds, labels) if C == 2 else CR.multiclass_auroc(scores, labels, C)
        _close(metrics["V_AUC"].compute(), want_auc)
        assert torch.equal(torch.nan_to_num(metrics["V_AUC"].compute()),
                           torch.nan_to_num(whole["AUC"].compute()))
        for m in metrics.values():
            m.reset()
        assert int(metrics["V_Rec"].state.sum()) == 0 and metrics["V_AUC"].scores == []
    column = scores[:, 1]
    pairs = twice(lambda: ops.cls_auroc_pairs(torch.from_numpy(column).to(cuda),
                                              torch.from_numpy((labels == 1).astype(np.int64)).to(cuda)))
    assert tuple(pairs.cpu().tolist()) == CR.auroc_pairs(column, (labels == 1).astype(np.int64))


@pytest.mark.parametrize("N", [1, 64, 65, 1000])
@pytest.mark.parametrize("C", [2, 3, 7])
def test_ordinal_metrics(cuda, N, C):
    from adell_mri_amd import classification_metrics as CM

    rng = np.random.default_rng(N + C)
    labels = rng.integers(0, C if C == 2 else C - 1, N)
    pred = np.clip(labels + rng.integers(-2, 3, N), 0, C - 1)
    M, _ = CR.confusion(pred, labels, C)
    metrics = CM.get_ordinal_metric_dict(C, prefix="T_").to(cuda)
    assert list(metrics) == ["T_Pearson", "T_Spearman", "T_MSE", "T_Kappa"]
    pd, ld = torch.from_numpy(pred).to(cuda), torch.from_numpy(labels).to(cuda)
    half = N // 2
    CM.update_many(metrics.values(), pd[:half].float(), ld[:half].float())     # what OrdNetPL feeds
    CM.update_many(metrics.values(), pd[half:], ld[half:])
    for key, fn in (("Pearson", CR.pearson), ("Spearman", CR.spearman), ("MSE", CR.mse),
                    ("Kappa", CR.kappa_quadratic)):
        assert torch.equal(metrics["T_" + key].state[:-1].cpu(), torch.from_numpy(M.reshape(-1)))
        _close(metrics["T_" + key].compute(), fn(M))


def test_a_bad_target_raises_at_compute(cuda):
    from adell_mri_amd import classification_metrics as CM

    m = CM.MulticlassRecall(3).to(cuda)
    m.update(torch.rand((4, 3), device=cuda), torch.tensor([0, 1, 3, 2], device=cuda))
    assert int(m.state[-1]) == 1 and int(m.state[:-1].sum()) == 3
    with pytest.raises(RuntimeError, match=r"outside \[0, 3\)"):
        m.compute()
    m.reset()
    m.update(torch.rand((4, 3), device=cuda), torch.tensor([0, 1, 2, 2], device=cuda))
    assert m.compute().dim() == 0
    auc = CM.BinaryAUROC().to(cuda)
    auc.update(torch.rand(4, device=cuda), torch.tensor([0, 1, 2, 0], device=cuda))
    with pytest.raises(RuntimeError, match=r"outside \[0, 2\)"):
        auc.compute()
    nan_wins = torch.tensor([[1.0, float("nan"), float("nan")], [2.0, 2.0, 1.0]], device=cuda)
    rec = CM.MulticlassRecall(3, average="none").to(cuda)
    rec.update(nan_wins, torch.tensor([1, 0], device=cuda))
    assert rec.compute().tolist() == [1.0, 1.0, 0.0]


# ---- pooling, feature extractors ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 4, 5, 2), (2, 5, 7), (3, 4, 6, 5), (2, 6)])
def test_global_pooling(cuda, shape):
    from adell_mri_amd.modules.classification import GlobalPooling

    x = torch.rand(shape, generator=torch.Generator().manual_seed(len(shape))) * 2 - 1
    r = torch.rand(shape[:2], generator=torch.Generator().manual_seed(7))
    for mode in ("max", "average"):
        xd = x.to(cuda).requires_grad_(True)
        y = GlobalPooling(mode)(xd)
        y.backward(r.to(cuda))
        xc = x.double().requires_grad_(True)
        if len(shape) == 2:
            want = xc * 1.0
        elif mode == "max":
            want = xc.flatten(start_dim=2).max(-1).values
        else:
            want = xc.flatten(start_dim=2).mean(-1)
        want.backward(r.double())
        assert y.shape == shape[:2]
        if mode == "max" or len(shape) == 2:
            assert torch.equal(y.detach().cpu(), want.detach().float())        # a selection
            assert torch.equal(xd.grad.cpu(), xc.grad.float())
        else:
            assert rel(y, want) < SUM_BOUND and rel(xd.grad, xc.grad) < SUM_BOUND
    with pytest.raises(ValueError, match="average,max"):
        GlobalPooling("median")


def test_catnet_probes_a_feature_extractor_on_its_own_device(cuda):
    """A feature extractor without ``output_features``: the reference's probe tensor, on the
    module's device, under ``no_grad``."""
    from adell_mri_amd.modules.classification import CatNet
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.layers.res_net import ResNetBackbone

    backbone = ResNetBackbone(3, 2, [(8, 16, 3, 2), (16, 32, 3, 2)], [(2, 2, 2), (2, 2, 2)],
                              adn_fn=get_adn_fn(3, "batch", "swish", 0.0))
    wrapped = torch.nn.Sequential(backbone).to(cuda)
    assert not hasattr(wrapped, "output_features")
    net = CatNet(in_channels=2, n_classes=3, feature_extraction=wrapped).to(cuda)
    assert net.last_size == net.output_features == 16
    assert all(p.grad is None for p in wrapped.parameters())
    assert "res_net.input_layer.0.weight" not in net.state_dict()
    out = net.eval()(torch.rand((2, 2, 16, 16, 8), device=cuda))
    assert out.shape == (2, 3) and bool(torch.isfinite(out).all())


# ---- one training step -------------------------------------------------------------------------------------
def build_step(name, cuda, **extra):
    """The wrapper of one fixture network with the fixture's weights on the device, in ``train()``
    mode with every dropout rate zeroed, and its batch."""
    g = StepGold(name)
    net, _ = build_pl(name, **extra)
    net_ = inner(net)
    net_.load_state_dict(fill(net_.state_dict(), float(g["gain"])))
    if name == "ord4":           # the constructor's zero, which the fill must not undo
        with torch.no_grad():
            net_.classification_layer.op[-1].bias.zero_()
    net = net.to(cuda).train()
    batch = {"image": torch.from_numpy(g["x"]).to(cuda),
             "label": torch.tensor(CONFIGS[name][3]).to(cuda)}
    return net, g, batch


def recording_forward(net):
    """Every output of ``net.forward`` from here on (the wrappers call ``self.forward``)."""
    seen, forward = [], net.forward

    def record(*args, **kwargs):
        out = forward(*args, **kwargs)
        seen.append(out)
        return out

    net.forward = record
    return seen


def expected_metrics(name, logits, labels, prefix, average="macro"):
    """The wrapper's metric dict from its own logits, by the restatement."""
    K = CONFIGS[name][1]["n_classes"]
    logits = logits.detach().double().cpu()
    if name == "ord4":
        pred = (torch.sigmoid(logits) > 0.5).sum(1).numpy()
        M, _ = CR.confusion(pred, labels, K)
        return {prefix + "Pearson": CR.pearson(M), prefix + "Spearman": CR.spearman(M),
                prefix + "MSE": CR.mse(M), prefix + "Kappa": CR.kappa_quadratic(M)}
    if K == 2:
        prob = torch.sigmoid(logits.float()).numpy()
        M, _ = CR.confusion(prob, labels, 2)
        values = {k: CR.per_class(M, kind)[1] for k, kind in (
            ("Rec", "recall"), ("Spe", "specificity"), ("Pr", "precision"), ("F1", "fbeta"))}
        values["AUC"] = CR.auroc(prob, labels)
    else:
        prob = torch.softmax(logits.float(), 1).numpy()
        M, _ = CR.confusion(prob, labels, K)
        values = {k: CR.macro(M, kind) for k, kind in (
            ("Rec", "recall"), ("Spe", "specificity"), ("Pr", "precision"), ("F1", "fbeta"))}
        values["AUC"] = CR.multiclass_auroc(prob, labels, K)
    return {prefix + k: v for k, v in values.items()}


@pytest.mark.parametrize("name", NETS)
def test_training_step_matches_reference(cuda, name):
    """``training_step`` through ``StepRunner`` in ``train()`` mode (batch statistics, running
    buffers updated): logits, loss (``loss + roc_loss`` for the ordinal network), every parameter
    gradient, one FusedAdamW step over the groups of ``configure_optimizers``, the buffers; then
    ``validate_steps`` (``eval()`` mode: the running statistics the step left)."""
    from adell_mri_amd.optim import FusedAdamW
    from adell_mri_amd.trainer import StepRunner, validate_steps

    net, g, batch = build_step(name, cuda)
    labels = np.array(CONFIGS[name][3])
    runner = StepRunner(net)
    assert isinstance(runner.optimizer, FusedAdamW)
    assert [len(gr["params"]) for gr in runner.optimizer.param_groups] == [
        len(g[f"groups:{i}:names"]) for i in range(int(g["groups:n"]))]
    assert [gr["weight_decay"] for gr in runner.optimizer.param_groups] == [
        float(g[f"groups:{i}:wd"]) for i in range(int(g["groups:n"]))]
    seen = recording_forward(net)
    runner.optimizer.zero_grad()
    loss = net.training_step(batch, 0)
    logits = seen[0][0] if name == "ord4" else seen[0]
    logits = torch.squeeze(logits, 1)
    assert logits.shape == g["logits"].shape and rel(logits, g["logits"]) < 1e-4
    if name == "ord4":
        assert rel(seen[0][1], g["pre_bias"]) < 1e-4
        parts = net.calculate_loss(logits.detach(), batch["label"],
                                   additional_params={"pre_bias": seen[0][1].detach()})
        np.testing.assert_allclose(parts[0].item(), g["loss"], rtol=1e-4)
        np.testing.assert_allclose(parts[1].item(), g["roc_loss"], rtol=1e-4)
    np.testing.assert_allclose(loss.item(), g["total"], rtol=1e-4)
    loss.backward()
    params = list(inner(net).named_parameters())
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
    for k, v in inner(net).state_dict().items():
        if k.startswith("feature_extraction."):
            continue                                   # the same tensors as ``res_net.*``
        if v.is_floating_point():
            np.testing.assert_allclose(v.detach().cpu().numpy(), g["step1:" + k], rtol=2e-4,
                                       atol=2e-6, err_msg=k)
        else:
            assert np.array_equal(v.cpu().numpy(), g["step1:" + k]), k
    # validation: eval mode, no gradient, the metrics of the wrapper's own logits
    del seen[:]
    grads = {k: None if p.grad is None else p.grad.clone() for k, p in params}
    out = validate_steps(net, [batch])
    np.testing.assert_allclose(out["val_loss"], g["val_total"], rtol=1e-4)
    assert net.training and len(seen) == 1
    vlogits = torch.squeeze(seen[0][0] if name == "ord4" else seen[0], 1)
    print(f"{name}: validation logits {rel(vlogits, g['val_logits']):.2e}")
    want = expected_metrics(name, vlogits, labels, "V_")
    assert sorted(out) == sorted(["val_loss"] + list(want))
    for k, v in want.items():
        np.testing.assert_allclose(out[k], v, rtol=2e-7, atol=1e-9, equal_nan=True, err_msg=k)
    for k, p in params:
        assert (p.grad is None) if grads[k] is None else torch.equal(p.grad, grads[k]), k


def test_test_steps_take_the_tuple_of_test_step(cuda):
    """``ClassNetPL.test_step`` returns ``(loss, prediction)``: the loop takes the loss; two batches,
    the metrics over both, reset afterwards."""
    from adell_mri_amd.trainer import test_steps

    net, g, batch = build_step("cat2", cuda)
    net.eval()
    with torch.no_grad():
        loss, prediction = net.test_step(batch, 0)
    assert loss.dim() == 0 and prediction.shape == (4,)
    for m in net.test_metrics.values():
        m.reset()
    other = {"image": batch["image"].flip(0).contiguous(), "label": 1 - batch["label"].flip(0)}
    seen = recording_forward(net)
    out = test_steps(net, [batch, other])
    logits = torch.cat([torch.squeeze(s, 1) for s in seen])
    labels = torch.cat([batch["label"], other["label"]]).cpu().numpy()
    want = expected_metrics("cat2", logits, labels, "T_")
    assert sorted(out) == sorted(["test_loss"] + list(want))
    for k, v in want.items():
        np.testing.assert_allclose(out[k], v, rtol=2e-7, atol=1e-9, equal_nan=True, err_msg=k)
    item = CR.loss("bce", logits.double().cpu().numpy(), labels.astype(np.float64))[0]
    np.testing.assert_allclose(out["test_loss"], item.mean(), rtol=1e-4)
    assert int(net.test_metrics["T_Rec"].state.sum()) == 0 and net.test_metrics["T_AUC"].scores == []


def test_training_step_with_mixup(cuda):
    """``training_batch_preproc``: the images through the mixup kernel, the labels mixed, the loss
    on soft targets; finite gradients everywhere."""
    from adell_mri_amd.utils.batch_preprocessing import BatchPreprocessing

    net, g, batch = build_step("vit_mean", cuda,
                               training_batch_preproc=BatchPreprocessing(0.05, 0.4, None, seed=5))
    rng = np.random.default_rng(5)
    factor, perm = rng.beta(0.4, 0.4, 4), rng.permutation(4)
    seen = recording_forward(net)
    loss = net.training_step({"image": batch["image"], "label": batch["label"].float()}, 0)
    loss.backward()
    y = torch.tensor(CONFIGS["vit_mean"][3]).float()
    y = torch.where(y < 0.5, y + 0.05, y - 0.05)
    f32 = torch.as_tensor(factor, dtype=torch.float32)
    y = y * f32 + y[perm] * (1.0 - f32)
    want = CR.loss("bce", seen[0].detach().double().cpu().numpy()[:, 0], y.double().numpy())[1]
    np.testing.assert_allclose(loss.item(), want, rtol=1e-4)
    for k, p in net.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
