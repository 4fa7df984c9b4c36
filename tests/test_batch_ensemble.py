"""Batch ensembles without a GPU: the fp64 restatements (tests/batch_ensemble_ref.py) against the
recorded results of the real reference (tests/golden/batch_ensemble_layers.npz,
tools/make_batch_ensemble_golden.py), the constructor signatures and module trees, the arguments that
raise, and the order in which a network draws its members."""
import numpy as np
import pytest
import torch

import batch_ensemble_cases as C
import batch_ensemble_ref as R

PIN = 1e-12                     # fp64 against fp64


def rel(a, r):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    assert a.shape == r.shape, (a.shape, r.shape)
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-300))


def torch_body(layer, n):
    """The body of a layer case as an fp64 torch module with the case's weights."""
    _, dim, cin, cout, _ = C.LAYERS[layer]
    op = {0: torch.nn.Linear, 2: torch.nn.Conv2d, 3: torch.nn.Conv3d}[dim]
    mod = op(cin, cout) if dim == 0 else op(cin, cout, 3)
    state = C.layer_state(layer, n)
    mod.load_state_dict({"weight": torch.from_numpy(state["mod.weight"]),
                         "bias": torch.from_numpy(state["mod.bias"])})
    return mod.double(), state


def adn():
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn

    return get_adn_fn(3, "batch", "swish", 0.0)


# ---- the restatement against the reference -------------------------------------------------------------
@pytest.mark.parametrize("layer,mode", C.layer_cases())
def test_layer_restatement_equals_the_reference(layer, mode):
    g = C.layer_gold()
    n, training, idx = C.MODES[mode]
    tag = f"{layer}:{mode}:"
    mod, state = torch_body(layer, n)
    x = torch.from_numpy(C.layer_input(layer)).double().requires_grad_(True)
    pre = torch.from_numpy(state["all_weights.pre"]).double().requires_grad_(True)
    post = torch.from_numpy(state["all_weights.post"]).double().requires_grad_(True)
    drawn = g[tag + "idxs"] if tag + "idxs" in g.files else None
    if training and idx is None and drawn is None:
        assert n == 1 and C.LAYERS[layer][0] == "BatchEnsembleWrapper"   # nothing drawn: member 0
        drawn = np.zeros(x.shape[0], dtype=np.int64)
    y = R.layer_forward(x, pre, post, mod, training, idx, drawn)
    assert rel(y.detach().numpy(), g[tag + "y"]) < PIN
    if tag + "dx" not in g.files:
        assert layer == "wrap" and mode == "mean"        # the wrapper's mean runs under no_grad
        return
    y.backward(torch.from_numpy(C.layer_dy(layer, y.shape)).double())
    for got, key in ((x.grad, "dx"), (pre.grad, "dall_weights.pre"), (post.grad, "dall_weights.post"),
                     (mod.weight.grad, "dmod.weight"), (mod.bias.grad, "dmod.bias")):
        assert rel(got.numpy(), g[tag + key]) < PIN, key


def test_kernel_restatements_equal_the_reference():
    """be_scale, members_expand, members_mean and their gradients, chained around the Linear of
    ``be0`` by hand, against the recorded layer results."""
    g = C.layer_gold()
    mod, state = torch_body("be0", C.N)
    W, bias = mod.weight.detach(), mod.bias.detach()
    x = C.layer_input("be0")
    pre, post = state["all_weights.pre"], state["all_weights.post"]
    dy = C.layer_dy("be0", g["be0:train:y"].shape)
    idxs = g["be0:train:idxs"]
    assert len(set(idxs.tolist())) > 1
    h = R.be_scale(x, pre, idxs)
    z = h @ W.T + bias
    assert rel(R.be_scale(z, post, idxs).numpy(), g["be0:train:y"]) < PIN
    dz, dpost = R.be_scale_backward(z, post, idxs, dy)
    dx, dpre = R.be_scale_backward(x, pre, idxs, dz @ W)
    for got, key in ((dx, "dx"), (dpre, "dall_weights.pre"), (dpost, "dall_weights.post")):
        assert rel(got.numpy(), g["be0:train:" + key]) < PIN, key
    never = sorted(set(range(C.N)) - set(idxs.tolist()))
    for m in never:
        assert not dpre[m].any() and not dpost[m].any()
    # the eval mean, in one piece and in chunks
    B = x.shape[0]
    for cuts in ([0, 3], [0, 2, 3], [0, 1, 2, 3]):
        acc = None
        for m0, m1 in zip(cuts[:-1], cuts[1:]):
            z = R.members_expand(x, pre, m0, m1) @ W.T + bias
            acc = R.members_mean(z, post, m0, m1, C.N, acc)
        assert rel(acc.numpy(), g["be0:mean:y"]) < PIN
    z = R.members_expand(x, pre, 0, C.N) @ W.T + bias
    assert z.shape[0] == C.N * B
    dz, dpost, dacc = R.members_mean_backward(z, post, 0, C.N, C.N, dy)
    dx, dpre = R.members_expand_backward(x, pre, 0, C.N, dz @ W)
    assert dacc is None
    for got, key in ((dx, "dx"), (dpre, "dall_weights.pre"), (dpost, "dall_weights.post")):
        assert rel(got.numpy(), g["be0:mean:" + key]) < PIN, key


def test_negative_entries_wrap_as_torch_indexing():
    assert R.wrap([2, 0, -1, 1, -3], 3).tolist() == [2, 0, 2, 1, 0]
    with pytest.raises(IndexError):
        R.wrap([0, 3], 3)


# ---- signatures and module trees -----------------------------------------------------------------------
def test_signatures_equal_the_reference():
    from adell_mri_amd.modules.layers import BatchEnsemble, BatchEnsembleWrapper

    want = C.surface_gold()["signatures"]
    for cls in (BatchEnsemble, BatchEnsembleWrapper):
        assert C.signature_of(cls.__init__) == want[f"{cls.__name__}.__init__"]
        # ``route`` (keyword only) is this package's: it forces a route of the eval mean
        mine = [p for p in C.signature_of(cls.forward) if p[0] != "route"]
        assert mine == want[f"{cls.__name__}.forward"]


def _tree(net):
    return {k: list(v.shape) for k, v in net.state_dict().items()}


def test_state_dict_keys_equal_the_reference():
    from adell_mri_amd.modules.classification import CatNet, OrdNet
    from adell_mri_amd.modules.layers import BatchEnsemble, BatchEnsembleWrapper
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.layers.linear_blocks import Linear
    from adell_mri_amd.modules.layers.res_net import ResNetBackbone

    want = C.surface_gold()["state"]
    structure = C.net_kwargs("cat")["resnet_structure"]
    assert _tree(BatchEnsemble(3, C.N, 4, 6, adn())) == want["BatchEnsemble"]
    assert _tree(BatchEnsemble(3, C.N, 4, 6, adn(), {"kernel_size": 3, "adn_fn": adn()},
                               res_blocks=True)) == want["BatchEnsemble.res_blocks"]
    assert _tree(BatchEnsembleWrapper(Linear(6, 5), C.N, 6, 5)) == want["BatchEnsembleWrapper"]
    backbone = ResNetBackbone(3, 1, structure, adn_fn=adn(), batch_ensemble=C.N)
    assert _tree(backbone) == want["ResNetBackbone"]
    assert "be_operations.1.all_weights.pre" in want["ResNetBackbone"]
    assert "be_operations.0.adn_op.op.normalization.weight" in want["ResNetBackbone"]
    assert _tree(ResNetBackbone(2, 1, structure, adn_fn=get_adn_fn(2, "batch", "swish", 0.0),
                                batch_ensemble=C.N)) == want["ResNetBackbone2d"]
    for stage in backbone.operations:
        assert [b.skip_activation for b in stage] == [None] * (len(stage) - 1) + [True]
    for name, cls in (("cat", CatNet), ("ord", OrdNet)):
        net = cls(adn_fn=adn(), **C.net_kwargs(name))
        g = C.StepGold(name)
        assert list(net.state_dict()) == [str(k) for k in g["state_keys"]]
        assert [k for k, _ in net.named_parameters()] == [str(k) for k in g["param_keys"]]
        assert _tree(net) == want[name]
        assert net.res_net.batch_ensemble == C.N


def test_without_members_the_backbone_is_what_it_was():
    from adell_mri_amd.modules.layers.res_net import ResNetBackbone

    structure = C.net_kwargs("cat")["resnet_structure"]
    net = ResNetBackbone(3, 1, structure, adn_fn=adn())
    assert _tree(net) == C.surface_gold()["state"]["ResNetBackbone.0"]
    assert not any("be_operations" in k for k in net.state_dict())
    assert list(net.be_operations) == [None, None]
    assert all(b.skip_activation is None for stage in net.operations for b in stage)


def test_member_tables_are_drawn_in_the_reference_order():
    from adell_mri_amd.modules.layers import BatchEnsemble

    np.random.seed(5)
    layer = BatchEnsemble(0, 4, 3, 2)
    np.random.seed(5)
    pre = np.random.normal(1, 0.1, size=[4, 3])
    post = np.random.normal(1, 0.1, size=[4, 2])
    assert torch.equal(layer.all_weights["pre"].detach(), torch.as_tensor(pre, dtype=torch.float32))
    assert torch.equal(layer.all_weights["post"].detach(), torch.as_tensor(post, dtype=torch.float32))
    assert layer.op_kwargs == {} and BatchEnsemble(2, 2, 3, 2).op_kwargs == {"kernel_size": 3}
    assert tuple(BatchEnsemble(3, 2, 3, 2).mod.padding) == (0, 0, 0)


# ---- what raises ---------------------------------------------------------------------------------------
def test_what_is_not_built_says_why():
    from adell_mri_amd.modules.classification import CatNet, OrdNet
    from adell_mri_amd.modules.layers import BatchEnsemble
    from adell_mri_amd.modules.layers.conv_next import ConvNeXtBackbone

    with pytest.raises(NotImplementedError, match="1-D convolution"):
        BatchEnsemble(1, 2, 3, 3)
    with pytest.raises(NotImplementedError, match="be_operations"):
        ConvNeXtBackbone(3, 1, [(8, 8, 3, 2)], batch_ensemble=2)
    kw = C.net_kwargs("cat")
    for cls in (CatNet, OrdNet):
        with pytest.raises(NotImplementedError, match="gaussian_process"):
            cls(adn_fn=adn(), gaussian_process=True, **kw)
        with pytest.raises(NotImplementedError, match="number of members"):
            cls(adn_fn=adn(), **dict(kw, batch_ensemble=True))


def test_idx_errors_are_raised_on_the_host():
    from adell_mri_amd.modules.layers import BatchEnsembleWrapper

    layer = BatchEnsembleWrapper(torch.nn.Identity(), 3, 4, 4)
    x = torch.zeros(5, 4)
    with pytest.raises(NotImplementedError, match="int, list or tuple"):
        layer(x, idx=np.array([0, 1, 2, 0, 1]))
    with pytest.raises(NotImplementedError, match="int, list or tuple"):
        layer(x, idx=1.0)
    with pytest.raises(AssertionError, match=r"len\(idx\) must be == X.shape\[0\]"):
        layer(x, idx=[0, 1, 2])
    for bad in ([0, 1, 3, 0, 1], (0, -4, 1, 0, 1)):
        with pytest.raises(IndexError):
            layer(x, idx=bad)
    for bad in (3, -4):
        with pytest.raises(IndexError):
            layer(x, idx=bad)


def test_route_of_the_eval_mean():
    from adell_mri_amd import functional as HF

    body = torch.nn.Sequential(torch.nn.Conv3d(2, 2, 1), torch.nn.BatchNorm3d(2)).eval()
    assert HF.be_route(3, 2, 1 << 10, body) == "batched"
    assert HF.be_route(1, 2, 1 << 10, body) == "loop"
    free = torch.nn.Sequential(torch.nn.Conv3d(2, 2, 1),
                               torch.nn.BatchNorm3d(2, track_running_stats=False)).eval()
    assert HF.be_route(3, 2, 1 << 10, free) == "loop"
    assert HF.be_route(3, 2, 1 << 10, body.train()) == "loop"      # batch statistics
    instance = torch.nn.Sequential(torch.nn.InstanceNorm3d(2), torch.nn.LayerNorm(2)).eval()
    assert HF.be_route(3, 2, 1 << 10, instance) == "batched"
    # a batch of which not even two members fit the budget
    assert HF.be_route(3, 2, HF.BE_BATCH_BUDGET_BYTES // 3, instance) == "loop"
    assert HF.be_chunk(4, 2, HF.BE_BATCH_BUDGET_BYTES // 6) == 3
    assert HF.be_chunk(4, 1, 1) == 4 and HF.be_chunk(4, 2, HF.BE_BATCH_BUDGET_BYTES) == 1


# ---- the draw order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.NETS))
def test_a_network_draws_once_per_stage_in_call_order(monkeypatch, name):
    """The backbone of a fixture network with every body replaced by the identity and the scale
    kernel by a recorder: under the fixture's seed the stages draw the recorded members, one draw per
    stage per forward; eval, an int ``batch_idx`` and ``return_intermediate`` draw nothing."""
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.classification import CatNet, OrdNet

    g = C.StepGold(name)
    net = {"cat": CatNet, "ord": OrdNet}[name](adn_fn=adn(), **C.net_kwargs(name))
    backbone = net.res_net
    backbone.input_layer = backbone.first_pooling = torch.nn.Identity()
    for i in range(len(backbone.operations)):
        backbone.operations[i] = torch.nn.Identity()
        backbone.pooling_operations[i] = torch.nn.Identity()
        backbone.be_operations[i].adn_op = torch.nn.Identity()
    seen = []

    def be_scale(x, table, idx=None):
        seen.append((tuple(table.shape), None if idx is None else idx.tolist()))
        return x

    monkeypatch.setattr(HF, "be_scale", be_scale)
    monkeypatch.setattr(HF, "be_members_expand", lambda x, pre, m0, m1: torch.cat([x] * (m1 - m0)))
    monkeypatch.setattr(HF, "be_members_mean",
                        lambda y, post, m0, m1, n, acc=None: y[:y.shape[0] // (m1 - m0)])
    x = torch.zeros(C.NETS[name][2])
    backbone.train()
    np.random.seed(C.STEP_SEED)
    backbone(x)
    drawn = g["idxs"]
    assert drawn.shape == (2, x.shape[0])
    widths = [(8, 8), (8, 16)]
    want = []
    for (cin, cout), row in zip(widths, drawn.tolist()):
        want += [((C.N, cin), row), ((C.N, cout), row)]           # pre and post of one draw
    assert seen == want
    follow = np.random.randint(C.N, size=4).tolist()
    np.random.seed(C.STEP_SEED)
    for _ in range(2):
        np.random.randint(C.N, size=x.shape[0])
    assert np.random.randint(C.N, size=4).tolist() == follow       # two draws, no more
    # nothing drawn: a given member, the eval mean, and forward(return_intermediate=True), which
    # hands no batch_idx on (as written in the reference) and so draws in training
    state = np.random.get_state()[1].copy()
    del seen[:]
    backbone(x, batch_idx=C.BATCH_IDX)
    assert seen == [((1, 8), None), ((1, 8), None), ((1, 8), None), ((1, 16), None)]
    backbone.eval()
    backbone(x)
    backbone.forward_intermediate(x, batch_idx=[0] * x.shape[0])
    assert np.array_equal(np.random.get_state()[1], state)
    backbone.train()
    del seen[:]
    backbone(x, return_intermediate=True, batch_idx=C.BATCH_IDX)
    assert [s[1] is not None for s in seen] == [True] * 4          # drawn, batch_idx ignored


def test_config_carries_batch_ensemble_to_the_backbone():
    from adell_mri_amd.modules.classification.pl import ClassNetPL, OrdNetPL
    from adell_mri_amd.modules.config_parsing import parse_config_cat
    from adell_mri_amd.utils.network_factories import get_classification_network

    resnet = {k: v for k, v in C.net_kwargs("cat").items() if k not in ("n_classes", "in_channels")}
    assert resnet["batch_ensemble"] == C.N
    cfg = parse_config_cat(dict(resnet, act_fn="swish", norm_fn="batch", batch_size=2))
    common = dict(network_config=cfg, dropout_param=0.0, seed=42, keys=["a"], clinical_feature_keys=[],
                  train_loader_call=None, max_epochs=10, warmup_steps=0, start_decay=5,
                  crop_size=[16, 16, 8])
    net = get_classification_network(net_type="cat", n_classes=2, **common)
    assert isinstance(net, ClassNetPL) and net.network.res_net.batch_ensemble == C.N
    assert [op.n for op in net.network.res_net.be_operations] == [C.N, C.N]
    cfg["classification_structure"] = [16]
    ordnet = get_classification_network(net_type="ord", n_classes=4, **dict(common, network_config=cfg))
    assert isinstance(ordnet, OrdNetPL) and ordnet.network.res_net.batch_ensemble == C.N
    # the member tables decay with the body: the reference's rule names the Gaussian-process head only
    groups = net.configure_optimizers()["optimizer"].param_groups
    names = {id(p): k for k, p in net.named_parameters()}
    tables = [k for k in names.values() if ".all_weights." in k]
    assert len(tables) == 4
    body = [names[id(p)] for p in groups[-1]["params"]]
    assert set(tables) <= set(body) and groups[-1]["weight_decay"] == net.weight_decay
