"""Multiple-instance classification without a GPU: construction of the six fixture networks,
``state_dict`` keys and shapes against the names recorded from the reference
(tests/golden/mil_step_*.npz), the YAML parser, every host-side raise, and the fp64 restatements of
tests/mil_ref.py against the reference's recorded intermediates (1e-12 relative: this pins the
restatements the GPU tests compare the kernels with)."""
import numpy as np
import pytest
import torch

import mil_ref as MR
from mil_cases import CONFIGS, NETS, SHAPE, STEP_EPS, STEP_LR, StepGold, build_net


def build_pl(name, **extra):
    """The wrapper of one fixture network, dropout rates zeroed (returned too)."""
    from adell_mri_amd.modules.classification import pl
    from adell_mri_amd.modules.classification.losses import configure_loss_fn
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.layers.res_net import ResNetBackbone

    class Wrappers:
        MultipleInstanceClassifier = pl.MultipleInstanceClassifierPL
        TransformableTransformer = pl.TransformableTransformerPL

    cfg = {}
    configure_loss_fn(cfg, "cat", CONFIGS[name][1]["n_classes"], None)
    return build_net(name, Wrappers, ResNetBackbone, get_adn_fn, loss_fn=cfg["loss_fn"],
                     learning_rate=STEP_LR, optimizer_eps=STEP_EPS, weight_decay=CONFIGS[name][3],
                     **extra)


@pytest.mark.parametrize("name", NETS)
def test_construction_and_state_dict(name):
    g = StepGold(name)
    net, rates = build_pl(name)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["state_keys"]]
    assert [",".join(str(d) for d in v.shape) for v in sd.values()] == [str(s) for s in
                                                                        g["state_shapes"]]
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in g["param_keys"]]
    assert [k for k, p in net.named_parameters() if p.requires_grad] == [
        str(k) for k in g["trainable_keys"]]
    assert rates == list(g["dropout_rates"])
    assert net.dim == 2 and net.n_slices == SHAPE[-1]
    # the optimiser's groups: the reference's, without the frozen module
    groups, base_wd = net.optimizer_groups()
    names = {id(p): k for k, p in net.named_parameters()}
    assert [[names[id(p)] for p in gr["params"]] for gr in groups] == [
        [str(k) for k in g[f"groups:{i}:names"]] for i in range(int(g["groups:n"]))]
    assert [gr["weight_decay"] for gr in groups] == [float(g[f"groups:{i}:wd"])
                                                     for i in range(int(g["groups:n"]))]
    assert base_wd == float(g["groups:base_wd"])
    frozen = {id(p) for k, p in net.named_parameters() if not p.requires_grad}
    assert (len(frozen) == 0) == CONFIGS[name][4]
    assert not any(id(p) in frozen for gr in groups for p in gr["params"])


def test_exports():
    import adell_mri_amd.modules.classification as C
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules import config_parsing

    for name in ("MILAttention", "MultipleInstanceClassifier", "TransformableTransformer",
                 "MultipleInstanceClassifierPL", "TransformableTransformerPL"):
        assert hasattr(C, name), name
    for name in ("volume_to_slices", "mil_gated_pool", "mil_attention", "slice_tokens"):
        assert callable(getattr(HF, name)), name
    assert callable(config_parsing.parse_config_2d_classifier_3d)
    att = C.MILAttention(5)
    assert sorted(att.state_dict()) == ["U.bias", "U.weight", "V.bias", "V.weight", "W.bias",
                                        "W.weight"]
    assert att.W.weight.shape == (1, 5) and att.along_dim == -2


def test_parse_config_2d_classifier_3d(tmp_path):
    from adell_mri_amd.modules.config_parsing import parse_config_2d_classifier_3d
    from adell_mri_amd.modules.layers.adn_fn import ActDropNormBuilder

    path = tmp_path / "mil.yaml"
    path.write_text("module_out_dim: 16\nn_classes: 2\nfeat_extraction_structure: [16, 16]\n"
                    "classification_structure: [16]\nclassification_mode: vocabulary\n"
                    "vocabulary_size: 6\nn_slices: 8\nattention: true\nnorm_fn: layer\n"
                    "act_fn: swish\nclassification_adn_fn:\n  norm_fn: layer\n  act_fn: gelu\n"
                    "  dropout_param: 0.0\n")
    config, correct = parse_config_2d_classifier_3d(str(path), 0.25, mil_method="standard")
    assert config["batch_size"] == 1 and config["norm_fn"] == "layer" and config["act_fn"] == "swish"
    assert "norm_fn" not in correct and "act_fn" not in correct
    assert sorted(correct) == sorted(k for k in config if k not in ("norm_fn", "act_fn"))
    assert isinstance(correct["adn_fn"], ActDropNormBuilder)
    assert isinstance(correct["classification_adn_fn"], ActDropNormBuilder)
    assert correct["adn_fn"].dropout_param == 0.25
    assert correct["classification_adn_fn"].dropout_param == 0.0
    assert correct["feat_extraction_structure"] == [16, 16] and correct["attention"] is True
    # defaults: "layer" / "gelu", and the network takes the dictionary as it is
    path.write_text("module_out_dim: 4\nn_classes: 3\nfeat_extraction_structure: []\n"
                    "classification_structure: [4]\nn_slices: 2\nbatch_size: 3\n")
    config, correct = parse_config_2d_classifier_3d(str(path), 0.0)
    assert config["batch_size"] == 3 and "classification_adn_fn" not in correct
    from adell_mri_amd.modules.classification import MultipleInstanceClassifier

    correct.pop("batch_size")
    net = MultipleInstanceClassifier(module=torch.nn.Identity(), **correct)
    assert net.final_prediction is not None and net.positional_embedding.shape == (1, 2, 1)


@pytest.mark.parametrize("cls", ["MultipleInstanceClassifier", "TransformableTransformer"])
def test_host_side_raises(cls):
    import adell_mri_amd.modules.classification as C

    kw = dict(module=torch.nn.Identity(), module_out_dim=4, n_classes=2, classification_structure=[4])
    if cls == "MultipleInstanceClassifier":
        kw["feat_extraction_structure"] = [4]
    else:
        kw.update(number_of_blocks=1, n_heads=2, mlp_structure=[4])
    make = getattr(C, cls)
    with pytest.raises(ValueError, match="n_slices"):
        make(**kw)                                      # the default: None
    with pytest.raises(ValueError, match="n_slices"):
        make(n_slices=None, **kw)
    for bad in ("sum", None, "average"):
        with pytest.raises(ValueError, match="reduce_fn"):
            make(n_slices=3, reduce_fn=bad, **kw)
    with pytest.raises(AssertionError, match="dim"):
        make(n_slices=3, dim=3, **kw)
    net = make(n_slices=3, dim=0, **kw)
    assert net.dim == 0                                 # stored, otherwise unused
    # raised before anything touches a kernel: CPU tensors get this far and no further
    with pytest.raises(ValueError, match="n_slices=3"):
        net(torch.zeros((2, 1, 4, 4, 5)))
    with pytest.raises(ValueError, match="n_slices=3"):
        net(torch.zeros((2, 1, 4, 3)))


def test_functional_argument_checks():
    """Shape and mode errors are raised on the host before the device is looked at."""
    from adell_mri_amd import functional as HF

    x = torch.zeros((2, 3, 4))
    with pytest.raises(ValueError, match="mode"):
        HF.mil_gated_pool(x, mode="median")
    with pytest.raises(ValueError, match="all or none"):
        HF.mil_gated_pool(x, x, None, None, None)
    with pytest.raises(ValueError, match="pos"):
        HF.slice_tokens(x, torch.zeros((1, 3, 4)))
    with pytest.raises(ValueError, match="class_token"):
        HF.slice_tokens(x, None, torch.zeros((1, 1, 5)))
    with pytest.raises(ValueError, match="volume"):
        HF.volume_to_slices(torch.zeros((2, 3, 4, 5)))


# ---- the restatements against the reference ---------------------------------------------------------
def close(a, r, rtol=1e-12):
    a, r = np.asarray(a, dtype=np.float64), np.asarray(r, dtype=np.float64)
    assert a.shape == r.shape, (a.shape, r.shape)
    assert np.abs(a - r).max() <= rtol * np.abs(r).max(), np.abs(a - r).max() / np.abs(r).max()


@pytest.mark.parametrize("name", [n for n in NETS if n.startswith("mil_")])
def test_pooling_restatement_equals_the_reference(name):
    g = StepGold(name)
    mode = CONFIGS[name][1]["classification_mode"]
    gate = {}
    if CONFIGS[name][1]["attention"]:
        gate = dict(hv=g["i:hv"], hu=g["i:hu"], w=g["i:w"], b=g["i:b"])
        assert g["i:hv"].dtype == np.float64
    pooled, A, arg = MR.gated_pool(g["i:feat"], mode=mode, **gate)
    close(pooled, g["i:pooled"])
    # (without the gate the reference builds A = ones / S in fp32 whatever the network's dtype:
    # 1 / 8 is exact in both)
    assert g["i:pooled"].dtype == np.float64
    assert g["i:A"].dtype == (np.float64 if gate else np.float32)
    assert A.shape == g["i:A"].shape == (SHAPE[0], SHAPE[-1], 1)
    close(A, g["i:A"])
    assert np.array_equal(g["attention"], g["i:A"].astype(np.float32))   # what the GPU step test reads
    close(A.sum(1), np.ones((SHAPE[0], 1)))
    close(MR.slice_tokens(g["i:tokens_in"], g["i:pos"]), g["i:tokens_out"])
    if not gate:
        close(A, np.full(A.shape, 1.0 / SHAPE[-1]))


@pytest.mark.parametrize("name", ["tt_cls", "tt_mean_train"])
def test_token_restatement_equals_the_reference(name):
    g = StepGold(name)
    ct = g["i:class_token"] if CONFIGS[name][1]["use_class_token"] else None
    out = MR.slice_tokens(g["i:tokens_in"], g["i:pos"], ct)
    assert out.shape == (SHAPE[0], SHAPE[-1] + (ct is not None), g["i:tokens_in"].shape[-1])
    close(out, g["i:tokens_out"])


def test_backward_restatements_by_finite_differences():
    """The fp64 backward formulas of mil_ref against central differences of its forward."""
    rng = np.random.default_rng(3)
    B, S, N, F = 2, 4, 3, 5
    hv, hu = rng.normal(size=(B, S, N)), rng.normal(size=(B, S, N))
    w, b, feat = rng.normal(size=N), rng.normal(size=1), rng.normal(size=(B, S, F))
    g, gA = rng.normal(size=(B, F)), rng.normal(size=(B, S, 1))
    for mode in ("mean", "max", "vocabulary"):
        def value(feat=feat, hv=hv, hu=hu, w=w, b=b):
            pooled, A, _ = MR.gated_pool(feat, hv, hu, w, b, mode)
            return (pooled * g).sum() + (A * gA).sum()

        grads = MR.gated_pool_bwd(feat, hv, hu, w, b, mode, g, gA)
        for key, arr in (("dfeat", feat), ("dhv", hv), ("dhu", hu), ("dw", w), ("db", b)):
            fd = np.zeros_like(arr)
            for idx in np.ndindex(arr.shape):
                hi, lo = arr.copy(), arr.copy()
                hi[idx] += 1e-6
                lo[idx] -= 1e-6
                fd[idx] = (value(**{key[1:]: hi}) - value(**{key[1:]: lo})) / 2e-6
            np.testing.assert_allclose(grads[key].reshape(arr.shape), fd, rtol=1e-6, atol=1e-8,
                                       err_msg=f"{mode} {key}")
        assert abs(grads["db"][0]) < 1e-12
    x = rng.normal(size=(2, 3, 4))
    dx, dpos, dcls = MR.slice_tokens_bwd(np.ones((2, 4, 4)), True)
    assert dx.shape == x.shape and np.all(dpos == 8.0) and np.all(dcls == 2.0)
    v = rng.normal(size=(2, 3, 4, 5, 6))
    assert np.array_equal(MR.slices_to_volume(MR.volume_to_slices(v), 6), v)
    assert np.array_equal(MR.volume_to_slices(v)[1 * 6 + 2], v[1, ..., 2])
