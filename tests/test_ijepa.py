"""I-JEPA without a GPU: the plain-torch restatement (tests/ijepa_ref.py, the GPU tests' reference)
reproduces the real reference's fp64 results (tests/golden/ijepa_step.npz,
tools/make_ijepa_golden.py), ``_sample_mask_indices`` draws the index sets the reference drew, the
state keys are the reference's in its order, ``ssl_method="ijepa"`` builds ``IJEPAPL`` where the
reference's factory builds it and raises where it -- or its loss -- fails, and nothing runs quietly
on the CPU."""
import os

import numpy as np
import pytest
import torch

import ijepa_ref as JR
from ijepa_cases import DRAWS, GOLD, NETS, StepGold, empty_config, step_config


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ijepa_step.npz"), allow_pickle=False)


def rel(a, r):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else a
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-300))


# ---- the restatement, pinned to the reference ------------------------------------------------------
def test_predictor_input_restatement_matches_the_reference(gold):
    cases = [str(c) for c in gold["predictor_cases"]]
    assert len(cases) == 3
    for name in cases:
        g = {k: gold[f"{name}:{k}"] for k in ("ctx", "tgt", "e", "pos", "mask", "r", "out", "de",
                                              "dpos", "dmask")}
        e = torch.from_numpy(g["e"]).double().requires_grad_(True)
        pos = torch.from_numpy(g["pos"]).double().requires_grad_(True)
        mask = torch.from_numpy(g["mask"]).double().requires_grad_(True)
        out = JR.predictor_input(e, pos, mask, g["ctx"], g["tgt"])
        assert out.shape == g["out"].shape and rel(out, g["out"]) < 1e-14, name
        (out * torch.from_numpy(g["r"]).double()).sum().backward()
        assert rel(e.grad, g["de"]) < 1e-14 and rel(pos.grad, g["dpos"]) < 1e-13, name
        assert rel(mask.grad, g["dmask"]) < 1e-13, name
        untouched = np.setdiff1d(np.arange(g["pos"].shape[1]), np.concatenate([g["ctx"], g["tgt"]]))
        assert not g["dpos"][:, untouched].any()


def test_block_loss_restatement_matches_the_reference(gold):
    cases = [str(c) for c in gold["loss_cases"]]
    assert len(cases) == 3
    for name in cases:
        pred = torch.from_numpy(gold[f"{name}:pred"]).double().requires_grad_(True)
        loss = JR.block_loss(pred, gold[f"{name}:h"], gold[f"{name}:rows"])
        np.testing.assert_allclose(loss.item(), gold[f"{name}:loss"], rtol=1e-13)
        loss.backward()
        assert rel(pred.grad, gold[f"{name}:dpred"]) < 1e-13, name
    # the layer norm of one feature is 0: the loss of l1 is that of pred against 0
    p = float(gold["l1:pred"].reshape(-1)[0])
    want = 0.5 * p * p if abs(p) < 1 else abs(p) - 0.5
    np.testing.assert_allclose(gold["l1:loss"], want, rtol=1e-12)


@pytest.mark.parametrize("name", NETS)
def test_step_loss_restatement_matches_the_reference(name):
    """What follows the encoders: the recorded predictions, the teacher's raw output and the drawn
    index sets give the recorded targets and the recorded loss."""
    g, cfg = StepGold(name), step_config(name)
    ba = cfg["backbone_args"]
    skip_n = ba.get("n_registers", 0) + int(ba["use_class_token"])
    _, tgts = g.draw(0)
    rows = [t + skip_n for t in tgts]
    preds = [g[f"pred{i}"] for i in range(len(tgts))]
    for i, t in enumerate(JR.targets(g["h"], rows)):
        assert t.shape == g[f"target{i}"].shape and rel(t, g[f"target{i}"]) < 1e-5, (name, i)
    # (predictions and h are stored in fp32: 1e-6 is their rounding, not the restatement's)
    np.testing.assert_allclose(JR.step_loss(preds, g["h"], rows).item(), g["loss"], rtol=1e-6)


# ---- the draws ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_sample_mask_indices_reproduces_the_recorded_draws(name):
    from adell_mri_amd.modules.self_supervised.jepa import IJEPA
    from adell_mri_amd.utils.masking import get_masker

    g, cfg = StepGold(name), step_config(name)
    net = IJEPA(**cfg)
    assert list(net.patch_masker_.parameters()) == []
    restated = get_masker("generic_transformer", image_dimensions=cfg["feature_map_dimensions"],
                          min_patch_size=cfg["min_patch_size"], max_patch_size=cfg["max_patch_size"],
                          n_patches=cfg["n_patches"], n_features=cfg["n_encoder_features"],
                          seed=cfg["seed"])
    assert int(g["draws"]) == 2 == len(DRAWS[name])
    T = int(np.prod(cfg["feature_map_dimensions"]))
    for i, (n_ctx, n_tgts) in enumerate(DRAWS[name]):
        want_ctx, want_tgts = g.draw(i)
        ctx, tgts = net._sample_mask_indices()
        np.testing.assert_array_equal(ctx, want_ctx)
        assert ctx.dtype == np.int64 and len(tgts) == len(want_tgts)
        for t, want in zip(tgts, want_tgts):
            np.testing.assert_array_equal(t, want)
            assert np.intersect1d(t, ctx).size == 0 and int(t.max()) < T
        # the counts the issue states, the dropped block included
        raw_ctx, raw_tgts = JR.sample_mask_indices(restated, cfg["n_patches"], cfg["n_masked_patches"])
        assert len(raw_ctx) == n_ctx == len(ctx) and [len(t) for t in raw_tgts] == n_tgts
        assert [len(t) for t in tgts] == [n for n in n_tgts if n > 0]
    assert [len(t) for t in g.draw(0)[1]] == ([6, 4, 4] if name == "net2d" else [7, 2, 3])


def test_all_targets_dropped_raises_on_the_host(gold):
    from adell_mri_amd.modules.self_supervised.jepa import IJEPA

    assert str(gold["empty:raises"]) == "RuntimeError" and int(gold["empty:blocks"]) == 0
    net = IJEPA(**empty_config())
    ctx, tgts = net._sample_mask_indices()
    np.testing.assert_array_equal(ctx, gold["empty:context"])
    assert len(ctx) == DRAWS["empty"][0][0] and tgts == []
    net.patch_masker_.rng = np.random.default_rng(net.seed)
    # CPU input: a kernel launch would raise AdellHipError, not RuntimeError with this message
    with pytest.raises(RuntimeError, match="target blocks lie inside"):
        net.forward_training(torch.zeros((2, 1, 32, 32)))


# ---- the module surface ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_state_keys_are_the_references_in_order(name):
    from adell_mri_amd.modules.self_supervised.jepa import IJEPA, IJEPAPredictor

    g = StepGold(name)
    net = IJEPA(**step_config(name))
    assert list(net.state_dict()) == [str(k) for k in g["state_keys"]]
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in g["param_keys"]]
    assert isinstance(net.predictor_, IJEPAPredictor)
    T = int(np.prod(net.feature_map_dimensions))
    width = 32
    assert tuple(net.predictor_.predictor_pos_embed_.shape) == (1, T, width)
    assert tuple(net.predictor_.mask_token_.shape) == (1, 1, width)
    assert net.predictor_.predictor_proj_.bias is None
    assert net.extra_tokens == (0 if name == "net2d" else 3)
    assert net.encoder_dim_ == (64 if name == "net2d" else 32) and net.reduce_fn == "mean"
    assert net._get_teacher_encoder(None) is net.encoder_
    holder = type("EMA", (), {"shadow": net})()
    assert net._get_teacher_encoder(holder) is net.encoder_


def test_construction_asserts():
    from adell_mri_amd.modules.self_supervised.jepa import IJEPA

    with pytest.raises(AssertionError, match="encoder architecture"):
        IJEPA(**step_config("net2d"), encoder_architecture="convnext")
    with pytest.raises(AssertionError, match="predictor architecture"):
        IJEPA(**step_config("net2d"), predictor_architecture="mlp")
    with pytest.raises(ValueError, match="strictly smaller"):
        IJEPA(**{**step_config("net2d"), "max_patch_size": [8, 8]})


def _valid_cfg():
    cfg = step_config("net2d")      # 48 wide: the default predictor has 3 heads
    cfg["backbone_args"].update(embedding_size=48, attention_dim=48, hidden_dim=48)
    return {"backbone_args": cfg["backbone_args"], "batch_size": 6, "learning_rate": 3e-4,
            "min_patch_size": [2, 2], "max_patch_size": [4, 4]}


def test_factory_builds_ijepapl_with_the_references_defaults():
    from adell_mri_amd.modules.self_supervised.jepa import IJEPA
    from adell_mri_amd.modules.self_supervised.pl import IJEPAPL
    from adell_mri_amd.optim import FusedAdamW
    from adell_mri_amd.utils import ExponentialMovingAverage
    from adell_mri_amd.utils.network_factories import get_ssl_network

    ema = ExponentialMovingAverage(0.99)
    net = get_ssl_network(None, 10, 100, 5, "ijepa", ema, "vit", _valid_cfg(), True)
    assert type(net) is IJEPAPL and isinstance(net, IJEPA)
    assert net.ema is ema and ema.shadow is not None          # the teacher, made in __init__
    assert isinstance(net.loss, torch.nn.SmoothL1Loss) and net.ssl_method == "ijepa"
    assert net.image_key == "image" and net.feature_map_dimensions == [8, 8]
    assert net.n_encoder_features == 48 and net.predictor_dim is None
    assert net.projection_head_args == {"number_of_blocks": 2, "attention_dim": 48,
                                        "hidden_dim": 48, "n_heads": 3}
    assert (net.min_patch_size, net.max_patch_size) == ([2, 2], [4, 4])
    assert (net.n_patches, net.n_masked_patches) == (1, 4) and net.seed == 42
    assert net.batch_size == 6 and net.learning_rate == 3e-4 and net.warmup_steps == 5
    assert net.weight_decay == 0.005 and net.n_steps == 100 and net.n_epochs == 10
    assert net.predictor_.predictor_dim == 48 and len(net.predictor_.predictor_.transformer_blocks) == 2
    # the factory's own patch sizes, on a feature map they fit; attention_dim as the fallback width
    cfg = _valid_cfg()
    del cfg["min_patch_size"], cfg["max_patch_size"]
    cfg["backbone_args"] = dict(cfg["backbone_args"], image_size=[48, 48], patch_size=[4, 4],
                                attention_dim=24, hidden_dim=24, n_heads=3)
    del cfg["backbone_args"]["embedding_size"]
    cfg.update(n_patches=2, n_masked_patches=3, predictor_dim=12,
               projection_head_args={"number_of_blocks": 1, "attention_dim": 12, "hidden_dim": 12,
                                     "n_heads": 3})
    net = get_ssl_network(None, 10, None, 0, "ijepa", ExponentialMovingAverage(0.99), "vit", cfg, True)
    assert (net.min_patch_size, net.max_patch_size) == ([4, 4], [8, 8])
    assert net.feature_map_dimensions == [12, 12] and net.n_encoder_features == 24
    assert (net.n_patches, net.n_masked_patches, net.predictor_dim) == (2, 3, 12)
    opt = net.configure_optimizers()
    assert isinstance(opt["optimizer"], FusedAdamW) and opt["monitor"] == "val_loss"
    assert opt["lr_scheduler"]["interval"] == "epoch"
    names = [k for k, _ in net.named_parameters()]
    order = [k for k in names if "normalization" not in k] + [k for k in names if "normalization" in k]
    params = dict(net.named_parameters())
    got = [p for group in opt["optimizer"].param_groups for p in group["params"]]
    assert len(got) == len(order) and all(a is params[k] for a, k in zip(got, order))


def test_factory_errors():
    from adell_mri_amd.utils import ExponentialMovingAverage
    from adell_mri_amd.utils.network_factories import get_ssl_network

    def build(cfg, ema="new", net_type="vit", method="ijepa"):
        ema = ExponentialMovingAverage(0.99) if ema == "new" else ema
        return get_ssl_network(None, 10, 100, 0, method, ema, net_type, cfg, True)

    with pytest.raises(TypeError, match="IJEPA only supports"):
        build(_valid_cfg(), net_type="convnext")
    with pytest.raises(TypeError):             # the reference's order: the net type comes first
        build({}, net_type="convnext")
    with pytest.raises(ValueError, match="I-JEPA requires an EMA"):
        build(_valid_cfg(), ema=None)
    with pytest.raises(NotImplementedError, match="backbone_args"):
        build({})
    for other in ("mae", "barlow"):
        with pytest.raises(NotImplementedError):
            build({}, method=other)
    cfg = _valid_cfg()                          # the default patches do not fit an 8 x 8 map
    del cfg["min_patch_size"], cfg["max_patch_size"]
    with pytest.raises(ValueError, match="strictly smaller"):
        build(cfg)


def test_ijepa_fails_loudly_without_gpu():
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.self_supervised.pl import IJEPAPL
    from adell_mri_amd.utils import ExponentialMovingAverage

    z = torch.zeros((2, 7, 4))
    for call in (lambda: HF.gather_tokens(z, [1, 3]),
                 lambda: HF.predictor_tokens(z[:, :2], torch.zeros((1, 9, 4)), torch.zeros((1, 1, 4)),
                                             [0, 4], [2, 8]),
                 lambda: HF.ijepa_block_loss(z[:, :2].contiguous(), z, [1, 3])):
        with pytest.raises(Exception) as info:
            call()
        assert not isinstance(info.value, (IndexError, NotImplementedError))
    with pytest.raises(IndexError, match="index 7 is out of bounds"):     # on the host
        HF.gather_tokens(z, [1, 7])
    with pytest.raises(IndexError):
        HF.ijepa_block_loss(z[:, :2].contiguous(), z, [1, 7])
    with pytest.raises(ValueError, match="disjoint"):
        HF.predictor_tokens(z[:, :2], torch.zeros((1, 9, 4)), torch.zeros((1, 1, 4)), [0, 4], [4, 8])
    pl = IJEPAPL(ema=ExponentialMovingAverage(0.99), **step_config("net2d"))
    with pytest.raises(Exception, match="MI355X"):
        pl.training_step({"image": torch.zeros((2, 1, 32, 32))}, 0)
    # the composed loss is plain torch on two lists
    a, b = [torch.ones((2, 3, 4)), torch.zeros((2, 1, 4))], [torch.zeros((2, 3, 4)), torch.zeros((2, 1, 4))]
    np.testing.assert_allclose(pl.calculate_loss(a, b).item(), 0.25)
