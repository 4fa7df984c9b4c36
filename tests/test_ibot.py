"""iBOT without a GPU: the mirror's masker draws the coordinates the real reference drew
(tests/golden/ibot_step.npz, tools/make_ibot_golden.py), the plain-torch restatement (tests/ibot_ref.py,
the GPU tests' reference for shapes too large to store) reproduces the reference's fp64 results, the
state keys are the reference's, ``ssl_method="ibot"`` builds ``iBOTPL`` where the reference's factory
builds it and raises where it -- or its forward -- fails, and nothing runs quietly on the CPU."""
import os

import numpy as np
import pytest
import torch

import ibot_ref as IR
from ibot_cases import GOLD, MASK_SEED, NETS, StepGold, step_config

VIEWS = ["v2d", "v3d"]


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ibot_step.npz"), allow_pickle=False)


def rel(a, r):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else a
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-300))


def recorded_draws(g):
    return [g[f"coords{i}"] for i in range(int(g["draws"]))]


# ---- masker ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_masker_reproduces_the_recorded_draws(name):
    from adell_mri_amd.utils.masking import GenericTransformerMasker, get_masker

    g, cfg = StepGold(name), step_config(name)
    assert int(g.top["mask_seed"]) == MASK_SEED == cfg["seed"]
    ba = cfg["backbone_args"]
    skip_n = ba.get("n_registers", 0) + int(ba["use_class_token"])
    masker = get_masker("generic_transformer", image_dimensions=cfg["feature_map_dimensions"],
                        min_patch_size=cfg["min_patch_size"], max_patch_size=cfg["max_patch_size"],
                        n_patches=cfg["n_patches"], n_features=cfg["n_encoder_features"],
                        seed=cfg["seed"])
    assert type(masker) is GenericTransformerMasker and list(masker.parameters()) == []
    assert masker.n_features == cfg["n_encoder_features"] and masker.n_dim == len(ba["image_size"])
    restated = IR.Masker(cfg["feature_map_dimensions"], cfg["min_patch_size"], cfg["max_patch_size"],
                         cfg["seed"])
    draws = recorded_draws(g)
    assert len(draws) >= 4
    for want in draws:                 # in order: the two of the step, then the further ones
        x, patches = masker(torch.zeros((1, 4, 2)), n_patches=cfg["n_patches"])    # no mask vector:
        got = np.unique(np.concatenate(patches) + (skip_n,))      # X untouched, per-patch indices
        assert x.shape == (1, 4, 2) and len(patches) == cfg["n_patches"]
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(restated.draw(cfg["n_patches"], skip_n), want)
        assert int(want.max()) < int(g["patch_tokens"])


def test_masker_refuses_what_the_reference_refuses():
    from adell_mri_amd.utils.masking import _check_patch_size, get_masker

    with pytest.raises(ValueError, match="strictly smaller"):
        get_masker("generic_transformer", image_dimensions=[8, 8], min_patch_size=[2, 2],
                   max_patch_size=[4, 8])
    with pytest.raises(ValueError):
        _check_patch_size([4, 4, 3], [3, 3, 3])
    _check_patch_size([4, 4, 3], [3, 3, 2])
    for other in ("transformer", "convolutional", "something"):
        with pytest.raises(NotImplementedError):
            get_masker(other, image_dimensions=[8, 8], min_patch_size=[2, 2], max_patch_size=[4, 4])


def test_row_tables_are_checked_on_the_host():
    from adell_mri_amd import functional as HF
    from adell_mri_amd import ops

    rows = ops.token_rows(np.array([1, 4, 5]), 7, "cpu")
    assert rows.dev.dtype == torch.int32 and rows.dev.tolist() == [1, 4, 5]
    assert rows.inv.tolist() == [-1, 0, -1, -1, 1, 2, -1]
    assert ops.token_rows([1, 4, 5], 7, "cpu") is rows              # kept: one upload per mask
    for bad, err in (([1, 7], IndexError), ([-1, 2], IndexError), ([], ValueError),
                     ([3, 3], ValueError), ([4, 1], ValueError), ([0.5], TypeError)):
        with pytest.raises(err):
            ops.token_rows(np.array(bad), 7, "cpu")
    x = torch.zeros((2, 7, 3))
    with pytest.raises(IndexError):                                  # before any kernel call
        HF.mask_tokens(x, [2, 7], torch.zeros(3))
    with pytest.raises(IndexError):
        HF.ibot_view(x, x, [6], torch.zeros(3), 0.1, 0.1, True, "cls")     # 6 patch rows: 0 .. 5
    with pytest.raises(ValueError, match="class token"):
        HF.ibot_view(x, x, [1], torch.zeros(3), 0.1, 0.1, False, "cls")
    assert HF.patch_rows([0, 5], 7, 1, "cpu").dev.tolist() == [1, 6]


# ---- the restatement against the reference's fp64 ------------------------------------------------------
@pytest.mark.parametrize("case", VIEWS)
def test_restatement_of_masker_and_splice(gold, case):
    assert [str(c) for c in gold["view_cases"]] == VIEWS
    nb, T, K, c, n_patches = (int(v) for v in gold[f"{case}:conf"])
    masker = IR.Masker(gold[f"{case}:dims"].tolist(), gold[f"{case}:min"].tolist(),
                       gold[f"{case}:max"].tolist(), int(gold[f"{case}:seed"]))
    m = masker.draw(n_patches, c)
    np.testing.assert_array_equal(m, gold[f"{case}:coords"])
    x = torch.from_numpy(gold[f"{case}:x"]).double().requires_grad_(True)
    token = torch.from_numpy(gold[f"{case}:token"]).double().requires_grad_(True)
    y = IR.splice(x, m, token)
    (y * torch.from_numpy(gold[f"{case}:r"]).double()).sum().backward()
    np.testing.assert_allclose(y.detach().numpy(), gold[f"{case}:spliced"], rtol=1e-12)
    np.testing.assert_allclose(x.grad.numpy(), gold[f"{case}:dx"], rtol=1e-12)
    np.testing.assert_allclose(token.grad.numpy(), gold[f"{case}:dtoken"], rtol=1e-12)
    assert float(x.grad[:, torch.as_tensor(m)].abs().max()) == 0.0


@pytest.mark.parametrize("method", ["center", "sk"])
@pytest.mark.parametrize("case", VIEWS)
def test_restatement_of_the_view_losses(gold, case, method):
    nb, T, K, c, _ = (int(v) for v in gold[f"{case}:conf"])
    t1, t2 = (float(t) for t in gold[f"{case}:t"])
    reduce_fn = str(gold[f"{case}:reduce_fn"])
    s = torch.from_numpy(gold[f"{case}:s"]).double().requires_grad_(True)
    y = torch.from_numpy(gold[f"{case}:y"]).double()
    centers = torch.from_numpy(gold[f"{case}:centers"]).double()
    s_red, loss = IR.view(s, y, gold[f"{case}:coords"], centers, t1, t2, c, reduce_fn, method)
    (loss + (s_red * torch.from_numpy(gold[f"{case}:w"]).double()).sum()).backward()
    # "sk": the reference runs its Sinkhorn-Knopp in fp32 whatever comes in
    tol = 1e-12 if method == "center" else 2e-6
    np.testing.assert_allclose(loss.item(), gold[f"{case}:{method}:loss"], rtol=tol)
    assert rel(s.grad, gold[f"{case}:{method}:ds"]) < max(tol, 1e-11)
    np.testing.assert_allclose(s_red.detach().numpy(), gold[f"{case}:s_red"], rtol=1e-12)
    total, rows = IR.mask_center_sum(y, torch.from_numpy(gold[f"{case}:y_other"]).double(), c)
    assert rows == int(gold[f"{case}:center_rows"]) == 2 * nb * T
    np.testing.assert_allclose(total.reshape(-1).numpy(), gold[f"{case}:center_sum"], rtol=1e-12)
    np.testing.assert_allclose((IR.token_sums(y, c) * (1.0 / T)).numpy(),
                               IR.reduce(y, c, "mean")[0].numpy(), rtol=1e-12)
    with pytest.raises(IndexError):
        IR.view(s, y, [T], centers, t1, t2, c, reduce_fn, method)


@pytest.mark.parametrize("name", NETS)
def test_restatement_reproduces_the_losses_of_the_step(name):
    """The recorded outputs are the fp64 step's, stored in fp32: the losses recomputed from them agree
    to fp32 rounding of the inputs (1e-6), the centre sums and centres likewise."""
    import dino_ref as R

    g, cfg = StepGold(name), step_config(name)
    nb, T, temp, m = int(g.top["B"]), int(g["patch_tokens"]), float(g.top["temperature"]), \
        float(g.top["center_m"])
    s, t = (torch.from_numpy(g[k]).double() for k in ("student_tokens", "teacher_tokens"))
    s_red, t_red = (torch.from_numpy(g[k]).double() for k in ("student_red", "teacher_red"))
    assert tuple(s.shape) == (2 * nb, T, cfg["out_dim"]) and tuple(s_red.shape) == (2 * nb, cfg["out_dim"])
    if cfg["reduce_fn"] == "mean":
        np.testing.assert_allclose(s.mean(1).numpy(), s_red.numpy(), rtol=1e-5, atol=1e-7)
    sums = {"mask": R.center_sum(t), "global": R.center_sum(t_red)}
    centers = {}
    for which, (total, rows) in sums.items():
        np.testing.assert_allclose(total.numpy(), g[f"{which}:center_sum"], rtol=1e-5)
        c0 = torch.from_numpy(g[f"{which}:centers0"]).double()
        centers[which] = R.center_apply(c0, total, rows, m)
        np.testing.assert_allclose(centers[which].numpy(), g[f"{which}:centers1"], rtol=1e-5)
    m1, m2 = (torch.as_tensor(g[k]) for k in ("coords0", "coords1"))
    loss_mask = (R.dino_loss(s[:nb][:, m1], t[:nb][:, m1], centers["mask"], temp, temp) / 2 +
                 R.dino_loss(s[nb:][:, m2], t[nb:][:, m2], centers["mask"], temp, temp) / 2)
    loss_global = (R.dino_loss(s_red[:nb], t_red[nb:], centers["global"], temp, temp) / 2 +
                   R.dino_loss(s_red[nb:], t_red[:nb], centers["global"], temp, temp) / 2)
    np.testing.assert_allclose(loss_mask.item(), g["loss_mask"], rtol=1e-6)
    np.testing.assert_allclose(loss_global.item(), g["loss_global"], rtol=1e-6)
    np.testing.assert_allclose(float(g["loss_mask"]) + float(g["loss_global"]), g["loss"], rtol=1e-12)


# ---- modules ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_state_keys_equal_the_reference(name):
    from adell_mri_amd.modules.self_supervised.ibot import iBOT

    g = StepGold(name)
    net = iBOT(**step_config(name))
    keys = list(net.state_dict().keys())
    assert keys == [str(k) for k in g["state_keys"]] and keys[0] == "mask_token_"
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in g["param_keys"]]
    for k, p in net.named_parameters():
        assert tuple(p.shape) == g["step1:" + k].shape, k
    assert tuple(net.mask_token_.shape) == (net.n_encoder_features,)
    assert list(net.patch_masker_.state_dict()) == []
    pair = net.last_layer_.parametrizations.weight
    assert pair.original0.requires_grad is False and pair.original1.requires_grad is True
    assert tuple(pair.original0.shape) == (net.out_dim, 1) and bool((pair.original0 == 1).all())
    ba = step_config(name)["backbone_args"]
    assert net.extra_tokens == (ba.get("n_registers", 0) + int(ba["use_class_token"]),)
    # the recorded gradients cover every trainable parameter the step uses (map_to_in is the
    # embedding's way back to patches: no part of iBOT)
    assert sorted(k[5:] for k in g.files if k.startswith("grad:")) == sorted(
        k for k, p in net.named_parameters() if p.requires_grad and ".map_to_in." not in k)
    assert "grad:mask_token_" in g.files


def _valid_cfg():
    cfg = step_config("net2d")
    return {"backbone_args": cfg["backbone_args"], "projection_head_args": cfg["projection_head_args"],
            "out_dim": 48, "temperature": 0.07, "centers_m": 0.8, "teacher_score_method": "sk",
            "min_patch_size": [2, 2], "max_patch_size": [4, 4], "batch_size": 6,
            "learning_rate": 3e-4}


def test_factory_builds_ibotpl():
    from adell_mri_amd.modules.self_supervised.losses import DinoLoss
    from adell_mri_amd.modules.self_supervised.pl import iBOTPL
    from adell_mri_amd.utils import ExponentialMovingAverage
    from adell_mri_amd.utils.network_factories import get_ssl_network

    ema = ExponentialMovingAverage(0.99)
    net = get_ssl_network(None, 10, 100, 5, "ibot", ema, "vit", _valid_cfg(), True)
    assert type(net) is iBOTPL and net.ssl_method == "ibot" and net.ema is ema
    assert ema.shadow is not None        # the constructor's first update makes the teacher
    assert net.loss_mask is not net.loss_global
    for crit in (net.loss_mask, net.loss_global):
        assert isinstance(crit, DinoLoss)
        assert (crit.t1, crit.t2) == (0.07, 0.07) and crit.center_m == 0.8
        assert crit.teacher_score_method == "sk" and crit.n_features == 48
        assert tuple(crit.centers.shape) == (48,) and crit.updated is True
    assert (net.aug_image_key_1, net.aug_image_key_2) == ("augmented_image_1", "augmented_image_2")
    assert net.feature_map_dimensions == [8, 8] and net.n_encoder_features == 64
    assert net.patch_masker_.image_dimensions == [8, 8]
    assert (net.min_patch_size, net.max_patch_size) == ([2, 2], [4, 4])
    assert net.n_patches == 4 and net.reduce_fn == "mean" and net.seed == 42     # iBOT's defaults
    assert net.batch_size == 6 and net.learning_rate == 3e-4 and net.warmup_steps == 5
    assert net.n_steps == 100 and net.n_epochs == 10 and net.stop_gradient is True
    assert {"loss_mask.centers", "loss_global.centers"} <= set(net.state_dict())
    # the factory's own defaults; n_encoder_features falls back to attention_dim
    cfg = _valid_cfg()
    for k in ("out_dim", "temperature", "centers_m", "teacher_score_method", "min_patch_size",
              "max_patch_size"):
        del cfg[k]
    cfg["backbone_args"] = dict(cfg["backbone_args"], image_size=[48, 48], patch_size=[4, 4],
                                attention_dim=16, hidden_dim=16)
    del cfg["backbone_args"]["embedding_size"]
    cfg["projection_head_args"] = {"structure": [16, 8]}
    net = get_ssl_network(None, 10, None, 0, "ibot", ExponentialMovingAverage(0.99), "vit", cfg, True)
    assert net.out_dim == 65536 and net.temperature == 0.1 and net.centers_m == 0.9
    assert net.teacher_score_method == "center" and net.loss_mask.n_features == 65536
    assert (net.min_patch_size, net.max_patch_size) == ([4, 4], [8, 8])
    assert net.feature_map_dimensions == [12, 12] and net.n_encoder_features == 16
    opt = net.configure_optimizers()
    assert opt["lr_scheduler"]["interval"] == "epoch" and opt["monitor"] == "val_loss"


def test_factory_errors():
    from adell_mri_amd.utils import ExponentialMovingAverage
    from adell_mri_amd.utils.network_factories import get_ssl_network

    def build(cfg, ema="new", net_type="vit"):
        ema = ExponentialMovingAverage(0.99) if ema == "new" else ema
        return get_ssl_network(None, 10, 100, 0, "ibot", ema, net_type, cfg, True)

    with pytest.raises(TypeError):
        build(_valid_cfg(), net_type="convnext")
    with pytest.raises(ValueError, match="EMA"):
        build(_valid_cfg(), ema=None)
    with pytest.raises(NotImplementedError, match="backbone_args"):
        build({})
    with pytest.raises(TypeError):             # the reference's order: the net type comes first
        build({}, net_type="convnext")
    for other in ("ijepa", "mae", "barlow"):
        with pytest.raises(NotImplementedError):
            get_ssl_network(None, 10, 100, 0, other, ExponentialMovingAverage(0.99), "vit", {}, True)
    # the default masker (patches up to [8, 8]) does not fit an 8 x 8 feature map
    cfg = _valid_cfg()
    del cfg["min_patch_size"], cfg["max_patch_size"]
    with pytest.raises(ValueError, match="strictly smaller"):
        build(cfg)


def test_configurations_the_reference_cannot_run_raise_at_construction():
    from adell_mri_amd.modules.self_supervised.ibot import iBOT

    def build(**changes):
        cfg = step_config("net2d")
        backbone = changes.pop("backbone", {})
        for k, v in backbone.items():
            if v is None:
                del cfg["backbone_args"][k]
            else:
                cfg["backbone_args"][k] = v
        cfg.update(changes)
        return iBOT(**cfg)

    build()
    # tokens of 16 patch features into a projection of attention_dim = 64 inputs
    with pytest.raises(NotImplementedError, match="attention_dim"):
        build(backbone={"embedding_size": None}, n_encoder_features=16)
    with pytest.raises(ValueError, match="n_encoder_features"):
        build(n_encoder_features=32)
    with pytest.raises(ValueError, match="class"):
        build(reduce_fn="cls")
    with pytest.raises(NotImplementedError, match="max"):
        build(reduce_fn="max")
    with pytest.raises(KeyError):
        build(projection_head_args={})
    build(backbone={"use_class_token": True}, reduce_fn="cls")


def test_ibot_fails_loudly_without_gpu():
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.self_supervised.ibot import iBOT
    from adell_mri_amd.modules.self_supervised.pl import iBOTPL
    from adell_mri_amd.utils import ExponentialMovingAverage

    net = iBOT(**step_config("net2d"))
    x = torch.zeros((2, 1, 32, 32))
    for call in (lambda: net.forward_training(x), lambda: net.forward_training(x, mask=True),
                 lambda: net(x), lambda: HF.mask_tokens(torch.zeros((2, 7, 3)), [1], torch.zeros(3)),
                 lambda: HF.token_mean(torch.zeros((2, 7, 3))),
                 lambda: HF.ibot_view(torch.zeros((2, 7, 3)), torch.zeros((2, 7, 3)), [1],
                                      torch.zeros(3), 0.1, 0.1, False, "mean")):
        with pytest.raises(Exception) as info:
            call()
        assert not isinstance(info.value, IndexError)
    pl = iBOTPL(ema=ExponentialMovingAverage(0.99), **step_config("net2d"))
    a = torch.zeros((2, 64, 48))
    with pytest.raises(IndexError):              # on the host, before any kernel call
        pl.calculate_loss_mask(a, a, np.array([3, 64]))
    with pytest.raises(Exception) as info:
        pl.calculate_loss_mask(a, a, np.array([3, 63]))
    assert not isinstance(info.value, IndexError)
    with pytest.raises(Exception):
        pl.calculate_loss_global(a[:, 0], a[:, 1])
    with pytest.raises(Exception):
        pl.training_step({"aug_image_1": x, "aug_image_2": x}, 0)


@pytest.mark.parametrize("B", [1, 2, 8, 64])
def test_token_sum_plan_covers_every_token_once(B):
    from adell_mri_amd import ops

    for T in (1, 7, 8, 9, 63, 216, 1000):
        for K in (5, 256, 1025, 8192, 65536):
            splits, per = ops.ibot_token_sums_plan(B, T, K)
            assert splits >= 1 and per >= 1 and (splits - 1) * per < T <= splits * per, (B, T, K)
            assert splits == 1 or per >= 4
    # few items: the token axis is split; many waves already: it is not
    assert ops.ibot_token_sums_plan(2, 216, 8192)[0] > 1
    assert ops.ibot_token_sums_plan(64, 216, 65536)[0] == 1
