"""Deconfounded classification without a GPU: the surface against the recorded one of the real
reference (tests/golden/deconfounded_surface.json, tools/make_deconfounded_golden.py), the fp64
restatements (tests/deconfounded_ref.py) against its recorded results, ``CategoricalConversion``, the
arguments that raise, ``deconf_route`` on both sides of every limit, the factory's argument handling
and the optimiser groups."""
import inspect

import numpy as np
import pytest
import torch

import deconfounded_cases as C
import deconfounded_ref as R

PIN = 1e-12                     # fp64 against fp64


def adn(dim=3):
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn

    return get_adn_fn(dim, "batch", "swish", 0.0)


def build_pl(name, **extra):
    from adell_mri_amd.modules.classification.deconfounded_classification import CategoricalConversion
    from adell_mri_amd.modules.classification.losses import CrossEntropyLoss
    from adell_mri_amd.modules.classification.pl import DeconfoundedNetPL

    kw = C.net_kwargs(name)
    args = dict(embedder=CategoricalConversion(C.CAT_VARS[name]), cat_confounder_key="cat",
                cont_confounder_key=None if C.NETS[name][4] is None else "cont",
                learning_rate=C.STEP_LR, optimizer_eps=C.STEP_EPS, weight_decay=C.STEP_WD,
                adn_fn=adn(kw["n_dim"]))
    if kw["n_classes"] > 2:
        args["loss_fn"] = CrossEntropyLoss()
    args.update(extra)
    return DeconfoundedNetPL(**args, **kw)


# ---- surface ---------------------------------------------------------------------------------------------
def test_signatures_match_the_reference():
    from adell_mri_amd.modules.classification import deconfounded_classification as D

    want = C.surface_gold()["signatures"]
    for name, sig in want.items():
        cls, fn = name.split(".")
        got = C.signature_of(getattr(getattr(D, cls), fn))
        # the reference's parameters, in its order, with its defaults; own keywords may follow
        assert got[:len(sig)] == sig, (name, got, sig)
        for extra in got[len(sig):]:
            assert extra[2] is not None, (name, extra)          # ... with defaults of their own
    assert C.signature_of(D.DeconfoundedNetGeneric.forward)[len(want["DeconfoundedNetGeneric.forward"]):] \
        == [["heads", "POSITIONAL_OR_KEYWORD", "True"]]


def _source_like(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        prefix = {p.VAR_POSITIONAL: "*", p.VAR_KEYWORD: "**"}.get(p.kind, "")
        out.append([prefix + p.name, None if p.default is p.empty else p.default])
    return out


def test_wrapper_and_factory_signatures_match_the_reference():
    from adell_mri_amd.modules.classification import pl as P
    from adell_mri_amd.utils import network_factories as NF

    want = C.surface_gold()
    for got, sig in ((_source_like(P.DeconfoundedNetPL.__init__),
                      want["source_signatures"]["DeconfoundedNetPL.__init__"]),
                     (_source_like(NF.get_deconfounded_classification_network),
                      want["source_signatures"]["get_deconfounded_classification_network"])):
        assert [a for a, _ in got] == [a for a, _ in sig]
        for (name, default), (_, text) in zip(got, sig):
            if text is None:
                assert default is None, name
            elif text == "OPTIMIZER_EPS_DEFAULT":
                assert default == 1e-8
            elif text == "F.binary_cross_entropy":
                assert default is None          # BCEWithLogitsLoss() at construction: the class says why
            else:
                assert default == eval(text), name      # literals: numbers, strings, None, {}
    missing = set(want["methods"]["DeconfoundedNetPL"]) - set(dir(P.DeconfoundedNetPL))
    assert not missing, missing


@pytest.mark.parametrize("name", list(C.NETS))
def test_state_dict_matches_the_reference(name):
    from adell_mri_amd.modules.classification.deconfounded_classification import DeconfoundedNetGeneric

    kw = C.net_kwargs(name)
    net = DeconfoundedNetGeneric(adn_fn=adn(kw["n_dim"]), **kw)
    got = {k: list(v.shape) for k, v in net.state_dict().items()}
    want = C.surface_gold()["state"][name]
    assert got == want, sorted(set(got) ^ set(want))
    for prefix in ("feature_extraction_module.", "confound_classifiers.0.", "classification_layer.0."):
        assert any(k.startswith(prefix) for k in got), prefix
    assert any(k.startswith("confound_regressions.") for k in got) == (name == "a")
    assert net.n_output_features == 16
    pl = build_pl(name)
    assert {k: list(v.shape) for k, v in pl.state_dict().items()} == want
    for attr in ("n_classes", "in_channels", "classification_structure", "n_dim",
                 "n_features_deconfounder", "n_cat_deconfounder", "n_cont_deconfounder",
                 "exclude_surrogate_variables", "deconfounder_structure", "args", "kwargs",
                 "n_output_features", "confound_classifiers", "confound_regressions", "gp"):
        assert hasattr(net, attr), attr
    assert pl.loss_str == ["loss", "cat_loss", "cont_loss", "feat_loss"] and pl.conf_mult == 1.0


def test_defaults_fill_in_as_in_the_reference():
    from adell_mri_amd.modules.classification.deconfounded_classification import DeconfoundedNetGeneric

    kw = C.net_kwargs("a")
    for k in ("n_features_deconfounder", "n_cat_deconfounder", "n_cont_deconfounder"):
        kw.pop(k)
    net = DeconfoundedNetGeneric(adn_fn=adn(), **kw)
    assert (net.n_features_deconfounder, net.n_cat_deconfounder, net.n_cont_deconfounder,
            net.deconfounder_structure) == (0, [], 0, [])
    assert net.confound_classifiers is None and net.confound_regressions is None
    assert net.linear_heads() is None


def test_feature_width_from_a_probe_on_the_modules_device():
    """A module without ``output_features``: the reference's probe shape, under ``no_grad``."""
    from adell_mri_amd.modules.classification.deconfounded_classification import DeconfoundedNetGeneric

    seen = []

    class Extractor(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.ones(1))

        def forward_features(self, X):
            seen.append((tuple(X.shape), X.device, torch.is_grad_enabled()))
            return X.flatten(2).mean(-1).repeat(1, 7) * self.w

    net = DeconfoundedNetGeneric(2, in_channels=3, feature_extraction_module=Extractor(), n_dim=2,
                                 classification_structure=[8], n_features_deconfounder=4,
                                 n_cat_deconfounder=[2])
    assert net.n_output_features == 21
    assert seen == [((1, 3, 64, 64), torch.device("cpu"), False)]
    assert net.classification_layer[0].op[0].in_features == 21


# ---- CategoricalConversion ---------------------------------------------------------------------------------
def test_categorical_conversion():
    from adell_mri_amd.modules.classification.deconfounded_classification import CategoricalConversion

    conv = CategoricalConversion([["s1", "s2", "s3"], [0, 1]])
    assert conv.key_lists == [["s1", "s2", "s3"], [0, 1]]
    assert conv.conversions == [{"s1": 0, "s2": 1, "s3": 2}, {"0": 0, "1": 1}]
    X = [["s2", "1"], ["s1", "0"], ["s3", "0"]]
    kept = [list(item) for item in X]
    out = conv(X)
    assert X == kept                                     # the input is left as it was
    assert [o.dtype for o in out] == [torch.int64] * 2
    assert [o.tolist() for o in out] == [[1, 0, 2], [1, 0, 0]]
    assert np.array_equal(torch.stack(CategoricalConversion(C.CAT_VARS["a"])(C.NETS["a"][3])).numpy(),
                          C.cat_table("a"))
    with pytest.raises(KeyError):
        conv([["s4", "0"]])
    with pytest.raises(AssertionError):
        conv([["s1"]])


# ---- raises ----------------------------------------------------------------------------------------------
def test_vgg_and_unknown_extractors_raise():
    from adell_mri_amd.modules.classification import deconfounded_classification as D
    from adell_mri_amd.modules.classification.pl import DeconfoundedNetPL

    with pytest.raises(NotImplementedError, match="(?i)vgg"):
        D.DeconfoundedNetGeneric(2)                      # the reference's default
    with pytest.raises(NotImplementedError, match="(?i)vgg"):
        D.DeconfoundedNetGeneric(2, feature_extraction_module="vgg")
    with pytest.raises(NotImplementedError, match="(?i)vgg"):
        D.DeconfoundedNet()
    with pytest.raises(NotImplementedError, match="(?i)vgg"):
        DeconfoundedNetPL(n_classes=2)
    with pytest.raises(ValueError, match="resnet"):
        D.DeconfoundedNetGeneric(2, feature_extraction_module="resnet")
    with pytest.raises(TypeError, match="forward_features"):
        D.DeconfoundedNetGeneric(2, feature_extraction_module=torch.nn.Linear(3, 3))
    kw = dict(C.net_kwargs("a"), n_features_deconfounder=16)
    with pytest.raises(ValueError, match="n_features_deconfounder"):
        D.DeconfoundedNetGeneric(adn_fn=adn(), **kw)


@pytest.mark.parametrize("n_conf", [0, -1, 7, 8])
def test_n_conf_outside_the_columns_raises(n_conf):
    """Argument checks come before any device work: they raise on CPU tensors too."""
    from adell_mri_amd import functional as HF

    x = torch.zeros(3, 7)
    for fn in (HF.deconf_correlation_loss, HF.split_columns):
        with pytest.raises(ValueError, match="n_conf"):
            fn(x, n_conf)
    W, b = torch.zeros(2, max(n_conf, 1)), torch.zeros(2)
    with pytest.raises(ValueError, match="n_conf"):
        HF.deconf_heads_loss(x, n_conf, [(W, b)], torch.zeros(1, 3, dtype=torch.int64), None, None)


def test_kernels_refuse_cpu_tensors_and_other_layouts():
    from adell_mri_amd import _lib
    from adell_mri_amd import functional as HF

    x = torch.zeros(3, 7)
    with pytest.raises(_lib.AdellHipError, match="CPU"):
        HF.deconf_correlation_loss(x, 2)
    with pytest.raises(_lib.AdellHipError, match="CPU"):
        HF.split_columns(x, 2)
    with pytest.raises(ValueError, match=r"\[B, F\]"):
        HF.deconf_correlation_loss(torch.zeros(3, 7, 2), 2)
    assert HF.deconf_heads_loss(x, 2, [], None, None, None) == (None, None)


# ---- the route -------------------------------------------------------------------------------------------
def test_deconf_route_on_both_sides_of_every_limit():
    from adell_mri_amd import functional as HF
    from adell_mri_amd import ops

    assert (ops.DECONF_MAX_HEADS, ops.DECONF_MAX_CLASSES, ops.DECONF_MAX_CONT, ops.DECONF_MAX_CONF) \
        == (C.MAX_HEADS, C.MAX_CLASSES, C.MAX_CONT, C.MAX_CONF)
    at = dict(n_conf=C.MAX_CONF, cat_classes=[C.MAX_CLASSES] * C.MAX_HEADS, n_cont=C.MAX_CONT)
    assert HF.deconf_route(**at) == "fused"
    assert HF.deconf_route(**dict(at, n_conf=C.MAX_CONF + 1)) == "composed"
    assert HF.deconf_route(**dict(at, cat_classes=[C.MAX_CLASSES] * (C.MAX_HEADS + 1))) == "composed"
    assert HF.deconf_route(**dict(at, cat_classes=[2, C.MAX_CLASSES + 1])) == "composed"
    assert HF.deconf_route(**dict(at, n_cont=C.MAX_CONT + 1)) == "composed"
    assert HF.deconf_route(1, [1]) == "fused" and HF.deconf_route(1, [], 1) == "fused"
    assert HF.deconf_route(8, [3, 2], 2, structure=[8]) == "composed"
    assert HF.deconf_route(8, [3, 2], 2, structure=[]) == "fused"
    for n, classes, n_cont in C.HEADS_BEYOND.values():
        assert HF.deconf_route(n, classes, n_cont) == "composed"
    with pytest.raises(Exception, match="deconf_route"):
        HF.deconf_route(8, [], 0)                        # no head at all
    with pytest.raises(Exception, match="deconf_route"):
        HF.deconf_route(8, [0])


def test_wrapper_names_its_route():
    a, b = build_pl("a"), build_pl("b")
    assert a.heads_route("cuda") == "fused" and a.heads_route("cpu") == "composed"
    assert b.heads_route("cuda") == "composed"           # deconfounder_structure=[8]
    assert a.linear_heads() is not None and b.linear_heads() is None
    cat, cont = a.linear_heads()
    assert [tuple(W.shape) for W, _ in cat] == [(3, 6), (2, 6)] and tuple(cont[0].shape) == (2, 6)
    assert build_pl("a", cat_confounder_key=None, cont_confounder_key=None).heads_route("cuda") \
        == "composed"                                    # nothing to predict: no loss to fuse


# ---- the restatement against the reference ---------------------------------------------------------------
@pytest.mark.parametrize("case", C.CORR_CASES + [C.CORR_DUP])
def test_correlation_restatement_equals_the_reference(case):
    """The loss for every case; the gradient where the reference's is finite (no constant column):
    the ``sqrt'(0) = 0`` rule changes nothing there."""
    g = C.kernel_gold()
    B, F, n = case
    tag = f"corr:{B}:{F}:{n}"
    x = C.dup_input() if case == C.CORR_DUP else C.corr_input(B, F, n)
    loss, grad = R.correlation_loss_and_grad(x, n)
    assert abs(loss - float(g[tag + ":loss"])) <= PIN * float(g[tag + ":loss"])
    zero = C.corr_zero_columns(B, F, n) if case != C.CORR_DUP else []
    assert np.isfinite(grad).all() and (grad[:, zero] == 0).all()
    if case == C.CORR_DUP:
        assert loss > 1.0 / (n * (F - n)) - 1e-12        # the duplicated pair alone gives r = 1
    if tag + ":live:grad" in g.files:
        live = C.corr_input(B, F, n, zero_columns=False)
        loss, grad = R.correlation_loss_and_grad(live, n)
        assert abs(loss - float(g[tag + ":live:loss"])) <= PIN
        assert R.rel(grad, g[tag + ":live:grad"]) < PIN


def test_reference_expression_is_nan_at_a_constant_column():
    """What the rule is for: ``sqrt``'s own backward at 0."""
    x = C.corr_input(5, 24, 8)
    _, grad = R.correlation_loss_and_grad(x, 8, sqrt=torch.sqrt)
    assert np.isnan(grad[:, [1, 9]]).all()


@pytest.mark.parametrize("B,n,heads", [(5, 8, "both"), (3, 1, "two"), (70, 65, "cont")])
def test_heads_restatement_equals_the_reference(B, n, heads):
    g = C.kernel_gold()
    tag = f"heads:{B}:{n}:{heads}"
    classes, n_cont = C.HEADS[heads]
    x, cat, labels, cont, target = C.heads_case(B, n + 3, n, classes, n_cont)
    cat_loss, cont_loss, grads = R.heads_losses(x, n, cat, labels, cont, target,
                                                float(g[tag + ":conf_mult"]))
    for got, key in ((cat_loss, "cat"), (cont_loss, "cont")):
        assert (got is None) == (f"{tag}:{key}" not in g.files)
        if got is not None:
            assert abs(got - float(g[f"{tag}:{key}"])) <= PIN * abs(float(g[f"{tag}:{key}"]))
    for k, v in grads.items():
        assert R.rel(v, g[f"{tag}:grad:{k}"]) < PIN, k


def test_heads_restatement_bad_label_is_nan():
    x, cat, labels, cont, target = C.heads_case(5, 9, 4, (2, 5), 2)
    labels[1, 3] = 5
    cat_loss, cont_loss, grads = R.heads_losses(x, 4, cat, labels, cont, target)
    assert np.isnan(cat_loss) and np.isfinite(cont_loss)
    assert np.isfinite(grads["W0"]).all() and np.isnan(grads["W1"]).all()
    assert np.isnan(grads["x"][3, :4]).all() and np.isfinite(np.delete(grads["x"], 3, 0)).all()


# ---- factory ---------------------------------------------------------------------------------------------
def _factory(**over):
    from adell_mri_amd.utils.network_factories import get_deconfounded_classification_network

    kw = C.net_kwargs("a")
    for k in ("n_classes", "in_channels", "n_features_deconfounder", "n_cat_deconfounder",
              "n_cont_deconfounder"):
        kw.pop(k)
    args = dict(network_config=dict(kw, act_fn="swish", norm_fn="batch", learning_rate=C.STEP_LR),
                dropout_param=0.0, seed=3, n_classes=2, keys=["image"], cat_confounder_key="cat",
                cont_confounder_key="cont", cat_vars=C.CAT_VARS["a"], cont_vars=2,
                train_loader_call=None, max_epochs=7, warmup_steps=2, start_decay=4,
                n_features_deconfounder=6)
    args.update(over)
    return get_deconfounded_classification_network(**args), args


def test_factory_argument_handling():
    from adell_mri_amd.modules.classification.deconfounded_classification import CategoricalConversion
    from adell_mri_amd.modules.classification.pl import DeconfoundedNetPL
    from adell_mri_amd.utils.batch_preprocessing import BatchPreprocessing

    net, args = _factory()
    assert "act_fn" in args["network_config"]            # the caller's config is not changed
    assert isinstance(net, DeconfoundedNetPL)
    assert (net.n_cat_deconfounder, net.n_cont_deconfounder, net.n_features_deconfounder) \
        == ([3, 2], 2, 6)
    assert isinstance(net.embedder, CategoricalConversion)
    assert net.embedder.key_lists == C.CAT_VARS["a"]
    assert (net.cat_confounder_key, net.cont_confounder_key) == ("cat", "cont")
    assert (net.image_key, net.label_key, net.n_epochs, net.warmup_steps, net.start_decay,
            net.optimizer_eps, net.learning_rate) == ("image", "label", 7, 2, 4, 1e-8, C.STEP_LR)
    assert isinstance(net.training_batch_preproc, BatchPreprocessing)
    assert net.in_channels == 1 and net.n_classes == 2 and not net.exclude_surrogate_variables
    want = C.surface_gold()["state"]["a"]
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == want
    # no categorical variables: no embedder, no categorical heads
    net, _ = _factory(cat_vars=None, cat_confounder_key=None)
    assert net.embedder is None and net.n_cat_deconfounder == [] and len(net.confound_classifiers) == 0
    assert net.confound_regressions is not None
    net, _ = _factory(exclude_surrogate_variables=True, keys=["a", "b"])
    assert net.in_channels == 2 and net.classification_layer[0].op[0].in_features == 16 - 6
    # the reference's default extractor
    cfg = {k: v for k, v in args["network_config"].items() if k != "feature_extraction_module"}
    with pytest.raises(NotImplementedError, match="(?i)vgg"):
        _factory(network_config=cfg)
    import adell_mri_amd.utils.network_factories as NF

    assert NF.get_deconfounded_classification_network.__module__ \
        == NF.get_classification_network.__module__


# ---- optimiser -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.NETS))
def test_optimizer_groups(name):
    """Adam, not AdamW: FusedAdam over the "confound" parameters at decay 0 and the rest at
    ``weight_decay`` -- the groups the fixture's step used."""
    from adell_mri_amd.modules.learning_rate import CosineAnnealingWithWarmupLR
    from adell_mri_amd.optim import FusedAdam

    net = build_pl(name)
    g = C.StepGold(name)
    cfg = net.configure_optimizers()
    opt = cfg["optimizer"]
    assert type(opt) is FusedAdam and not opt.decoupled
    assert isinstance(cfg["lr_scheduler"], CosineAnnealingWithWarmupLR) and cfg["monitor"] == "val_loss"
    names = {id(p): n for n, p in net.named_parameters()}
    groups = [[names[id(p)] for p in gr["params"]] for gr in opt.param_groups]
    assert len(groups) == int(g["groups:n"]) == 2
    for i, members in enumerate(groups):
        assert members == list(g[f"groups:{i}:names"])
        assert opt.param_groups[i]["weight_decay"] == float(g[f"groups:{i}:wd"])
    assert groups[0] and all("confound" in n for n in groups[0])
    assert not any("confound" in n for n in groups[1])
    assert [gr["weight_decay"] for gr in opt.param_groups] == [0, C.STEP_WD]
    assert all(gr["lr"] == C.STEP_LR and gr["eps"] == C.STEP_EPS for gr in opt.param_groups)
