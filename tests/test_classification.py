"""Classification without a GPU: the fp64 restatements (tests/classification_ref.py) against the
recorded results of the real reference and against scikit-learn / scipy, the draw order of
``BatchPreprocessing``, the module trees and optimiser groups of the fixture networks
(tests/golden/classification_step_*.npz, tools/make_classification_golden.py), the factory's errors
and the ordinal label tables."""
import numpy as np
import pytest
import torch

import classification_ref as CR
from classification_cases import (CONFIGS, NETS, STEP_EPS, STEP_LR, StepGold, case_gold, net_kwargs,
                                  step_groups, zero_dropout)


def build_pl(name, **extra):
    """The wrapper of one fixture network, dropout rates zeroed (returned too)."""
    from adell_mri_amd.modules.classification.losses import configure_loss_fn
    from adell_mri_amd.modules.classification.pl import ClassNetPL, OrdNetPL, ViTClassifierPL
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn

    cls, _, _, _, weights, weight_decay = CONFIGS[name]
    kw = net_kwargs(name)
    cfg = {}
    configure_loss_fn(cfg, "ord" if cls == "OrdNet" else "cat", kw["n_classes"],
                      None if weights is None else torch.tensor(weights))
    common = dict(loss_fn=cfg["loss_fn"], learning_rate=STEP_LR, optimizer_eps=STEP_EPS,
                  weight_decay=weight_decay, **extra)
    if cls == "ViTClassifier":
        net = ViTClassifierPL(**common, **kw)
    else:
        wrapper = OrdNetPL if cls == "OrdNet" else ClassNetPL
        net = wrapper(adn_fn=get_adn_fn(3, "batch", "swish", 0.0), **common, **kw)
    return net, zero_dropout(net)


def inner(net):
    return getattr(net, "network", net)


# ---- the restatements against the reference ---------------------------------------------------------
@pytest.mark.parametrize("name", [str(n) for n in case_gold()["loss_cases"]])
def test_loss_restatements_equal_the_reference(name):
    g = case_gold()
    kind, K = str(g[f"{name}:kind"]), int(g[f"{name}:K"])
    w = g[f"{name}:w"] if f"{name}:w" in g.files else None
    x = g[f"{name}:x"][:, 0] if kind == "bce" else g[f"{name}:x"]
    item, red, dx = CR.loss(kind, x, g[f"{name}:y"], w, K)
    np.testing.assert_allclose(item, g[f"{name}:item"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(red, g[f"{name}:loss"], rtol=1e-12)
    np.testing.assert_allclose(dx.reshape(g[f"{name}:dx"].shape), g[f"{name}:dx"], rtol=1e-11,
                               atol=1e-14)
    assert np.abs(g[f"{name}:x"]).max() == 90.0
    if kind == "ordinal":
        value, dp, M = CR.roc(g[f"{name}:x"][:, 0], g[f"{name}:y"])
        assert M > 0
        np.testing.assert_allclose(value, g[f"{name}:roc"], rtol=1e-12)
        np.testing.assert_allclose(dp, g[f"{name}:dpre"][:, 0], rtol=1e-11, atol=1e-14)
    # a per-item incoming gradient: the chain rule on the items
    gi = np.linspace(-1.0, 2.0, item.shape[0])
    _, _, dxi = CR.loss(kind, x, g[f"{name}:y"], w, K, g=gi)
    eps, flat = 1e-6, np.asarray(x, dtype=np.float64)
    probe = flat.copy()
    idx = tuple(np.unravel_index(np.argmin(np.abs(flat)), flat.shape))
    probe[idx] += eps
    up = (CR.loss(kind, probe, g[f"{name}:y"], w, K)[0] * gi).sum()
    probe[idx] -= 2 * eps
    down = (CR.loss(kind, probe, g[f"{name}:y"], w, K)[0] * gi).sum()
    np.testing.assert_allclose(dxi[idx], (up - down) / (2 * eps), rtol=1e-5, atol=1e-8)


def test_roc_restatement_without_pairs_is_nan():
    value, dp, M = CR.roc([0.1, 0.2, 0.3], [2, 2, 2])
    assert M == 0 and np.isnan(value) and np.isnan(dp).all()
    assert np.isnan(float(torch.nn.functional.binary_cross_entropy_with_logits(
        torch.zeros(0), torch.zeros(0))))        # the reference's mean over no pairs


def _metric_data(seed, N, C):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, N)
    scores = np.round(rng.random((N, C)) * 8) / 8          # many ties
    return scores, labels


def test_metric_restatements_equal_sklearn():
    skm = pytest.importorskip("sklearn.metrics")
    for seed, N, C in [(1, 200, 2), (2, 300, 3), (3, 500, 7)]:
        scores, labels = _metric_data(seed, N, C)
        M, bad = CR.confusion(scores, labels, C)
        pred = CR.classes_of(scores, C)
        assert bad == 0 and M.sum() == N
        kw = dict(labels=list(range(C)), average=None, zero_division=0)
        np.testing.assert_allclose(CR.per_class(M, "recall"), skm.recall_score(labels, pred, **kw))
        np.testing.assert_allclose(CR.per_class(M, "precision"),
                                   skm.precision_score(labels, pred, **kw))
        np.testing.assert_allclose(CR.per_class(M, "fbeta"), skm.f1_score(labels, pred, **kw))
        np.testing.assert_allclose(CR.macro(M, "recall"),
                                   skm.recall_score(labels, pred, average="macro", zero_division=0))
        np.testing.assert_allclose(CR.kappa_quadratic(M),
                                   skm.cohen_kappa_score(labels, pred, weights="quadratic"))
        for c in range(C):
            one = (labels == c).astype(int)
            np.testing.assert_allclose(CR.auroc(scores[:, c], one),
                                       skm.roc_auc_score(one, scores[:, c]), rtol=1e-12)
        # specificity of class c is the recall of "not c"
        for c in range(C):
            np.testing.assert_allclose(CR.per_class(M, "specificity")[c],
                                       skm.recall_score(labels != c, pred != c, zero_division=0))
    prob = np.round(np.random.default_rng(5).random(100) * 8) / 8
    y = np.random.default_rng(6).integers(0, 2, 100)
    M, _ = CR.confusion(prob.astype(np.float32), y, 2)
    np.testing.assert_allclose(CR.per_class(M, "recall")[1], skm.recall_score(y, prob > 0.5))


def test_ordinal_metric_restatements_equal_scipy():
    stats = pytest.importorskip("scipy.stats")
    for seed, N, C in [(1, 200, 2), (2, 300, 4), (3, 500, 7)]:
        rng = np.random.default_rng(seed)
        labels = rng.integers(0, C, N)
        pred = np.clip(labels + rng.integers(-2, 3, N), 0, C - 1)
        M, bad = CR.confusion(pred, labels, C)
        assert bad == 0
        np.testing.assert_allclose(CR.pearson(M), stats.pearsonr(pred, labels)[0], rtol=1e-10)
        np.testing.assert_allclose(CR.spearman(M), stats.spearmanr(pred, labels)[0], rtol=1e-10)
        np.testing.assert_allclose(CR.mse(M), np.mean((pred - labels) ** 2.0))
    assert np.isnan(CR.pearson(np.diag([0, 5, 0]))) and np.isnan(CR.spearman(np.diag([0, 5, 0])))


def test_metric_conventions():
    M = np.array([[3, 1, 0], [2, 4, 0], [0, 0, 0]])       # class 2 absent from labels and predictions
    assert CR.per_class(M, "recall")[2] == 0.0
    np.testing.assert_allclose(CR.macro(M, "recall"), (3 / 4 + 4 / 6) / 2)
    assert CR.macro(np.zeros((3, 3)), "precision") == 0.0
    assert np.isnan(CR.auroc([0.1, 0.2], [1, 1])) and np.isnan(CR.multiclass_auroc(
        np.zeros((2, 3)), [1, 1], 1))
    assert list(CR.argmax_nan_wins([[1.0, np.nan, np.nan], [2.0, 2.0, 1.0]])) == [1, 0]
    assert CR.auroc_pairs([0.5, 0.5, 0.25, 1.0], [1, 0, 0, 1]) == (2 * 3 + 1, 2, 2)


# ---- batch preprocessing ------------------------------------------------------------------------------
class _Recorder:
    """``functional.mixup_rows`` replaced: records (factor, partner), mixes on the CPU."""

    def __init__(self):
        self.calls = []

    def __call__(self, x, factor, partner):
        self.calls.append((factor.double().numpy().copy(), np.asarray(partner).copy()))
        return CR.mixup_rows(x, factor, partner)


@pytest.mark.parametrize("name", ["mixup", "partial"])
def test_batch_preprocessing_draws_in_the_reference_order(monkeypatch, name):
    from adell_mri_amd import functional as HF
    from adell_mri_amd.utils.batch_preprocessing import BatchPreprocessing

    g = case_gold()
    alpha, partial, seed = g[f"draws:{name}:args"]
    rec = _Recorder()
    monkeypatch.setattr(HF, "mixup_rows", rec)
    bp = BatchPreprocessing(None, float(alpha), None if partial < 0 else float(partial), int(seed))
    for call in range(2):
        factor, perm = g[f"draws:{name}:{call}:factor"], g[f"draws:{name}:{call}:perm"]
        selected = g[f"draws:{name}:{call}:selected"]
        x = torch.arange(18, dtype=torch.float32).reshape(6, 3)
        y = torch.tensor([0, 1, 1, 0, 1, 0])
        x0, y0 = x.clone(), y.clone()
        X, Y = bp(x, y)
        got_factor, got_partner = rec.calls[call]
        np.testing.assert_array_equal(got_factor, factor.astype(np.float32).astype(np.float64))
        np.testing.assert_array_equal(got_partner, np.where(selected, perm, np.arange(6)))
        assert torch.equal(x, x0) and torch.equal(y, y0)          # the inputs are not written
        f32 = torch.as_tensor(factor, dtype=torch.float32)
        mixed = y0.float() * f32 + y0.float()[perm] * (1.0 - f32)
        want = torch.where(torch.as_tensor(selected), mixed, y0.float()).to(torch.int64)
        assert Y.dtype == torch.int64 and torch.equal(Y, want)     # cast back: integers truncate
        assert X.shape == x.shape


def test_label_smoothing():
    from adell_mri_amd.utils.batch_preprocessing import BatchPreprocessing, label_smoothing

    y = torch.tensor([0.0, 1.0, 0.4, 0.5])
    assert torch.equal(label_smoothing(y, 0.1), torch.tensor([0.1, 0.9, 0.5, 0.4]))
    X, Y = BatchPreprocessing(label_smoothing=0.1)(torch.zeros(4, 2), y)
    assert torch.equal(Y, torch.tensor([0.1, 0.9, 0.5, 0.4])) and torch.equal(X, torch.zeros(4, 2))


# ---- module trees, optimiser groups ----------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_state_dict_keys_equal_the_reference(name):
    g = StepGold(name)
    net, rates = build_pl(name)
    assert list(inner(net).state_dict()) == [str(k) for k in g["state_keys"]]
    assert [k for k, _ in inner(net).named_parameters()] == [str(k) for k in g["param_keys"]]
    assert sorted(rates) == sorted(float(r) for r in g["dropout_rates"])
    if name.startswith("cat"):
        assert inner(net).feature_extraction is inner(net).res_net and 0.1 in rates
    if name == "ord4":
        head = inner(net).classification_layer.op[-1]
        assert float(head.bias.detach().abs().max()) == 0.0 and head.bias.requires_grad
        assert inner(net).ordinal_bias.tolist() == [1.0, 0.0, -1.0]
        np.testing.assert_allclose(float(inner(net).ordinal_bias_scale.detach()), 1 / 3)


@pytest.mark.parametrize("name", NETS)
@pytest.mark.parametrize("tag", ["groups", "groups_other"])
def test_optimizer_groups_equal_the_reference(name, tag):
    from adell_mri_amd.optim import FusedAdamW

    g = StepGold(name)
    weight_decay = CONFIGS[name][5]
    if tag == "groups_other":
        weight_decay = (0.05, 0.1) if not isinstance(weight_decay, tuple) else 0.05
    net, _ = build_pl(name)
    net.weight_decay = weight_decay
    prefix = "network." if hasattr(net, "network") else ""
    opt = net.configure_optimizers()["optimizer"]
    assert isinstance(opt, FusedAdamW) and opt.defaults["weight_decay"] == float(g[f"{tag}:base_wd"])
    assert opt.defaults["lr"] == STEP_LR and opt.defaults["eps"] == STEP_EPS
    names = {id(p): k for k, p in net.named_parameters()}
    assert len(opt.param_groups) == int(g[f"{tag}:n"]) == (4 if isinstance(weight_decay, tuple) else 3)
    for i, group in enumerate(opt.param_groups):
        want = [prefix + str(k) for k in g[f"{tag}:{i}:names"]]
        assert [names[id(p)] for p in group["params"]] == want, i
        assert group["weight_decay"] == float(g[f"{tag}:{i}:wd"])
    assert opt.param_groups[0]["params"] == []                 # the empty group is accepted
    restated, base = step_groups(list(inner(net).named_parameters()), weight_decay)
    assert [len(m) for m, _ in restated] == [len(gr["params"]) for gr in opt.param_groups]
    if name == "ord4":
        assert [names[id(p)] for p in opt.param_groups[1]["params"]] == [
            "network.ordinal_bias", "network.ordinal_bias_scale"]


# ---- factory -------------------------------------------------------------------------------------------
def _factory(net_type, network_config, n_classes=2, clinical=(), **kw):
    from adell_mri_amd.utils.network_factories import get_classification_network

    return get_classification_network(
        net_type=net_type, network_config=network_config, dropout_param=0.0, seed=42,
        n_classes=n_classes, keys=["a", "b"], clinical_feature_keys=list(clinical),
        train_loader_call=None, max_epochs=10, warmup_steps=0, start_decay=5, crop_size=[8, 16], **kw)


def test_factory_builds_and_refuses():
    from adell_mri_amd.modules.classification.pl import ClassNetPL, OrdNetPL, ViTClassifierPL
    from adell_mri_amd.modules.config_parsing import parse_config_cat
    from adell_mri_amd.utils.batch_preprocessing import BatchPreprocessing

    resnet = {k: v for k, v in net_kwargs("cat2").items() if k != "n_classes"}
    cfg = parse_config_cat(dict(resnet, act_fn="gelu", norm_fn="batch", batch_size=2,
                                learning_rate=0.01))
    net = _factory("cat", cfg, mixup_alpha=0.4)
    assert isinstance(net, ClassNetPL) and net.n_classes == 2 and net.network.in_channels == 2
    assert isinstance(net.training_batch_preproc, BatchPreprocessing)
    assert net.training_batch_preproc.mixup_alpha == 0.4 and net.learning_rate == 0.01
    assert "act_fn" in cfg                                     # the caller's mapping is not changed
    ordnet = _factory("ord", dict(resnet, classification_structure=[16]), n_classes=4)
    assert isinstance(ordnet, OrdNetPL) and list(ordnet.val_metrics) == [
        "V_Pearson", "V_Spearman", "V_MSE", "V_Kappa"]
    vit = {k: v for k, v in net_kwargs("vit_cls").items()
           if k not in ("n_classes", "in_channels", "image_size")}
    vnet = _factory("vit", vit, n_classes=3)
    assert isinstance(vnet, ViTClassifierPL) and tuple(vnet.image_size) == (8, 16)
    assert list(vnet.val_metrics) == ["V_Rec", "V_Spe", "V_Pr", "V_F1", "V_AUC"]
    with pytest.raises(ValueError, match="net_type 'resnet' not valid"):
        _factory("resnet", {})
    for net_type in ("unet", "factorized_vit", "vgg"):
        with pytest.raises(NotImplementedError, match=net_type):
            _factory(net_type, {})
    with pytest.raises(NotImplementedError, match="clinical_feature_keys"):
        _factory("cat", dict(resnet), clinical=["age"])


def test_unbuilt_members_name_their_argument():
    from adell_mri_amd import classification_metrics as CM
    from adell_mri_amd.modules.classification import CatNet, ViTClassifier
    from adell_mri_amd.modules.classification.pl import ClassNetPL

    kw = net_kwargs("cat2")
    with pytest.raises(NotImplementedError, match="gaussian_process"):
        CatNet(gaussian_process=True, **kw)
    with pytest.raises(NotImplementedError, match="batch_ensemble"):
        CatNet(batch_ensemble=True, **kw)
    with pytest.raises(NotImplementedError):
        CatNet(res_type="resnext", **kw)
    with pytest.raises(NotImplementedError, match="seqpool"):
        ViTClassifier(**dict(net_kwargs("vit_cls"), use_class_token="seqpool"))
    with pytest.raises(NotImplementedError, match="vgg"):
        ClassNetPL(net_type="vgg", **kw)
    with pytest.raises(NotImplementedError, match="CalErr"):
        CM.get_metric_dict(2, ["Rec", "CalErr"])
    assert "CalErr" not in "".join(CM.get_metric_dict(3, None, prefix="V_").keys())

    class Features(torch.nn.Module):
        output_features = 24

    assert CatNet(feature_extraction=Features(), n_classes=3).last_size == 24


def test_ordinal_label_tables():
    from adell_mri_amd.modules.classification import label_to_ordinal, ordinal_prediction_to_class

    g = case_gold()
    labels = torch.from_numpy(g["table:labels"])
    assert torch.equal(label_to_ordinal(labels, 5), torch.from_numpy(g["table:ordinal"]))
    assert torch.equal(label_to_ordinal(labels, 5, ignore_0=False),
                       torch.from_numpy(g["table:ordinal_keep0"]))
    assert torch.equal(ordinal_prediction_to_class(torch.from_numpy(g["table:probs"])),
                       torch.from_numpy(g["table:classes"]))
