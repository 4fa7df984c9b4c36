"""The masked autoencoder without a GPU: the plain-torch restatement (tests/mae_ref.py, the GPU tests'
reference) reproduces the real reference's fp64 results (tests/golden/mae_step.npz,
tools/make_mae_golden.py), ``random_masking`` draws the ids the reference drew, the state keys are
the reference's in its order, ``ssl_method="mae"`` builds ``ViTMaskedAutoEncoderPL`` from a full
configuration and raises for an incomplete one, the shuffle table is checked on the host, and
nothing runs quietly on the CPU."""
import os

import numpy as np
import pytest
import torch

import mae_ref as MR
from mae_cases import B, CONFIGS, GOLD, NETS, StepGold, step_config


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "mae_step.npz"), allow_pickle=False)


def rel(a, r):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else a
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-300))


# ---- the restatement, pinned to the reference ------------------------------------------------------
def test_restore_and_loss_restatement_matches_the_reference(gold):
    cases = [str(c) for c in gold["small_cases"]]
    assert len(cases) == 3
    for name in cases:
        g = {k: gold[f"{name}:{k}"] for k in ("ids_shuffle", "K", "image_shape", "mask", "e", "r", "x",
                                              "pos", "mask_token", "scale", "out", "recon", "de",
                                              "dpos", "dmask_token", "dscale", "loss", "dpred")}
        K = int(g["K"])
        leaves = [torch.from_numpy(g[k]).double().requires_grad_(True)
                  for k in ("e", "pos", "mask_token", "scale")]
        e, pos, mask_token, scale = leaves
        out = MR.restore(MR.keep(e, g["ids_shuffle"], K), mask_token, scale, pos, g["ids_shuffle"])
        assert out.shape == g["out"].shape and rel(out, g["out"]) < 1e-14, name
        (out * torch.from_numpy(g["r"]).double()).sum().backward()
        for leaf, k in zip(leaves, ("de", "dpos", "dmask_token", "dscale")):
            want = g[k]
            if not want.any():          # K == L: no masked row
                assert K == g["ids_shuffle"].shape[1] and k in ("dmask_token", "dscale")
                assert leaf.grad is None or not leaf.grad.any(), (name, k)
            else:
                assert rel(leaf.grad, want) < 1e-13, (name, k)
        shape = tuple(int(v) for v in g["image_shape"])
        recon = MR.to_image(out.detach(), shape)
        assert recon.shape == g["recon"].shape and np.array_equal(recon.numpy(), g["recon"]), name
        pred = out.detach().clone().requires_grad_(True)
        loss = MR.loss(pred, g["x"])
        np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-13)
        loss.backward()
        assert rel(pred.grad, g["dpred"]) < 1e-13, name
        # the mask is 0 on the K kept tokens of every item
        assert g["mask"].shape == g["ids_shuffle"].shape and (g["mask"] == 0).sum(1).tolist() == [K] * len(g["mask"])
    assert int(gold["r3:K"]) == gold["r3:ids_shuffle"].shape[1]         # the case without a masked row
    assert not gold["r3:dmask_token"].any() and not gold["r3:dscale"].any()


def test_the_image_is_the_index_map_the_issue_states(gold):
    """recon[b, c].flatten()[l P + p] = pred[b, l, p C + c]; for one channel a pure view."""
    for name in NETS:
        g = StepGold(name)
        pred, recon = g["pred"], g["recon"]
        Bn, C, H, W = recon.shape
        L, P = pred.shape[1], pred.shape[2] // C
        want = pred.reshape(Bn, L, P, C).transpose(0, 3, 1, 2).reshape(Bn, C, H, W)
        assert np.array_equal(recon, want)
        assert np.array_equal(MR.to_image(torch.from_numpy(pred), recon.shape).numpy(), recon)
        if C == 1:
            assert np.array_equal(recon.reshape(-1), pred.reshape(-1))
        np.testing.assert_allclose(MR.loss(pred, g["x"]).item(), g["loss"], rtol=1e-6)   # fp32 records


# ---- the draws ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_random_masking_reproduces_the_recorded_draws(name):
    from adell_mri_amd.modules.self_supervised import autoencoders as AE

    g, (cfg, L, E, K) = StepGold(name), CONFIGS[name]
    assert MR.len_keep(L, cfg["mask_fraction"]) == K == 4
    rng = np.random.default_rng(int(g.top["seed"]))
    for i in range(2):
        want = g[f"ids_shuffle{i}"]
        assert want.shape == (B, L) and want.dtype == np.int64
        ids_shuffle, ids_restore, mask = MR.masking_ids(g[f"noise{i}"], cfg["mask_fraction"])
        np.testing.assert_array_equal(ids_shuffle, want)
        np.testing.assert_array_equal(mask, g[f"mask{i}"])
        shuffle = AE._shuffle(B, L, cfg["mask_fraction"], rng, "cpu")      # the module's own draw
        np.testing.assert_array_equal(shuffle.host, want)
        np.testing.assert_array_equal(shuffle.restore_host, ids_restore)
        assert shuffle.K == K and shuffle.keep.dtype == torch.int32
        np.testing.assert_array_equal(shuffle.keep.numpy(), want[:, :K])
        np.testing.assert_array_equal(shuffle.restore.numpy(), ids_restore)
        np.testing.assert_array_equal(shuffle.mask.numpy(), g[f"mask{i}"])
        assert shuffle.mask.dtype == torch.float32
        inv = shuffle.inv.numpy()
        assert ((inv >= 0) == (g[f"mask{i}"] == 0)).all()
        for b in range(B):
            kept = np.nonzero(inv[b] >= 0)[0]
            np.testing.assert_array_equal(want[b, inv[b, kept]], kept)
    assert not np.array_equal(g["ids_shuffle0"], g["ids_shuffle1"])
    assert len({tuple(r) for r in g["ids_shuffle0"]}) == B        # a shuffle per item


# ---- the module surface ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_state_keys_are_the_references_in_order(name):
    from adell_mri_amd.modules.self_supervised.autoencoders import ViTAutoEncoder, ViTMaskedAutoEncoder

    g, (cfg, L, E, K) = StepGold(name), CONFIGS[name]
    net = ViTMaskedAutoEncoder(**step_config(name))
    assert isinstance(net, ViTAutoEncoder)
    assert list(net.state_dict()) == [str(k) for k in g["state_keys"]]
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in g["param_keys"]]
    assert list(net.state_dict())[:4] == ["positional_embedding", "mask_token_scale", "mask_token",
                                          "proj.positional_embedding"]
    assert net.positional_embedding is net.proj.positional_embedding
    assert sum(p is net.positional_embedding for p in net.parameters()) == 1
    assert (net.n_patches, net.n_features, net.patch_elems) == (L, E, E // cfg["in_channels"])
    assert tuple(net.mask_token.shape) == (1, 1, E) and net.mask_token_scale.tolist() == [1.0]
    assert net.decoder_pred[0].out_features == 4 * E and net.decoder_pred[2].out_features == E
    assert net.input_dim_size == 96 and net.seed == 42 and net.mask_fraction == cfg["mask_fraction"]
    for k, v in g.top.items():      # every recorded tensor of the network fits the module
        if k.startswith(name + ":step1:"):
            assert tuple(v.shape) == tuple(net.state_dict()[k.split(":", 2)[2]].shape), k


def test_construction_errors():
    from adell_mri_amd.modules.self_supervised.autoencoders import ViTMaskedAutoEncoder

    cfg = step_config("c1")
    with pytest.raises(ValueError, match="2-D images"):
        ViTMaskedAutoEncoder(**{**cfg, "image_size": [16, 16, 16], "patch_size": [4, 4, 4]})
    with pytest.raises(ValueError, match="keeps int"):      # int(16 * (1 - 0.95)) == 0
        ViTMaskedAutoEncoder(**{**cfg, "mask_fraction": 0.95})
    assert ViTMaskedAutoEncoder(**{**cfg, "mask_fraction": 0.9}).mask_fraction == 0.9   # keeps 1


# ---- the factory -------------------------------------------------------------------------------------
def _full_cfg():
    cfg = step_config("c2")
    enc = dict(cfg["encoder_args"], image_size=cfg["image_size"], patch_size=cfg["patch_size"],
               in_channels=cfg["in_channels"])
    return {"encoder_args": enc, "decoder_args": cfg["decoder_args"], "batch_size": 6,
            "learning_rate": 3e-4, "mask_fraction": 0.6}


def test_factory_builds_the_wrapper_with_the_references_defaults():
    from adell_mri_amd.modules.self_supervised.autoencoders import ViTMaskedAutoEncoder
    from adell_mri_amd.modules.self_supervised.pl import ViTMaskedAutoEncoderPL
    from adell_mri_amd.utils import ExponentialMovingAverage
    from adell_mri_amd.utils.network_factories import get_ssl_network

    # an EMA is handed in and dropped; there is no net_type check
    net = get_ssl_network(None, 10, 100, 5, "mae", ExponentialMovingAverage(0.99), "convnext",
                          _full_cfg(), True)
    assert type(net) is ViTMaskedAutoEncoderPL and type(net.model) is ViTMaskedAutoEncoder
    assert not hasattr(net, "ema") and isinstance(net.criterion, torch.nn.MSELoss)
    assert net.image_key == "image" and net.model.mask_fraction == 0.6
    assert net.model.image_size == [16, 24] and net.model.patch_size == [4, 8]
    assert net.model.in_channels == 2 and net.model.input_dim_size == 96
    assert net.batch_size == 6 and net.learning_rate == 3e-4 and net.weight_decay == 1e-6
    assert (net.n_epochs, net.n_steps, net.warmup_steps, net.start_decay) == (10, 100, 5, 0)
    cfg = _full_cfg()               # the defaults: one channel, mask_fraction 0.75, embed_dim
    del cfg["mask_fraction"], cfg["encoder_args"]["in_channels"]
    cfg["encoder_args"]["embed_dim"] = 48
    net = get_ssl_network(None, 10, None, 0, "mae", None, "vit", cfg, True)
    assert net.model.mask_fraction == 0.75 and net.model.in_channels == 1
    assert net.model.input_dim_size == 48 and net.model.n_features == 32 and net.n_steps is None


def test_factory_raises_for_an_incomplete_configuration():
    from adell_mri_amd.utils.network_factories import get_ssl_network

    def build(cfg, method="mae"):
        return get_ssl_network(None, 10, 100, 0, method, None, "vit", cfg, True)

    with pytest.raises(NotImplementedError, match="encoder_args"):
        build({})
    cfg = _full_cfg()
    del cfg["decoder_args"]
    with pytest.raises(NotImplementedError, match="decoder_args"):
        build(cfg)
    for side, keys in (("encoder_args", ("number_of_blocks", "hidden_dim", "n_heads", "mlp_structure",
                                         "image_size", "patch_size")),
                       ("decoder_args", ("number_of_blocks", "hidden_dim", "n_heads",
                                         "mlp_structure"))):
        for key in keys:
            cfg = _full_cfg()
            del cfg[side][key]
            with pytest.raises(NotImplementedError, match=f"`{side}` lacks `{key}`"):
                build(cfg)
    with pytest.raises(NotImplementedError):
        build({}, method="barlow")
    with pytest.raises(NotImplementedError):
        build(_full_cfg(), method="barlow")


def test_parse_config_ssl_passes_a_mae_configuration_through(tmp_path):
    from adell_mri_amd.modules.config_parsing import parse_config_ssl
    from adell_mri_amd.modules.self_supervised.pl import ViTMaskedAutoEncoderPL
    from adell_mri_amd.utils.network_factories import get_ssl_network

    path = tmp_path / "mae.yaml"
    path.write_text(
        "batch_size: 4\nmask_fraction: 0.5\nnorm_fn: layer\nact_fn: gelu\n"
        "encoder_args:\n  image_size: [16, 16]\n  patch_size: [4, 4]\n  in_channels: 1\n"
        "  number_of_blocks: 1\n  hidden_dim: 16\n  n_heads: 2\n  mlp_structure: [16]\n"
        "decoder_args:\n  number_of_blocks: 1\n  hidden_dim: 16\n  n_heads: 2\n  mlp_structure: [16]\n")
    config, correct = parse_config_ssl(str(path), 0.0, 2, is_vit=True)
    assert correct["encoder_args"]["in_channels"] == 2 and "norm_fn" not in correct
    net = get_ssl_network(None, 10, None, 0, "mae", None, "vit", correct, True)
    assert type(net) is ViTMaskedAutoEncoderPL and net.model.in_channels == 2
    assert net.model.mask_fraction == 0.5 and net.model.n_features == 32 and net.batch_size == 4


# ---- the optimiser -----------------------------------------------------------------------------------
def test_configure_optimizers_bare_or_with_warmup():
    from adell_mri_amd.modules.learning_rate import CosineAnnealingWithWarmupLR
    from adell_mri_amd.modules.self_supervised.pl import ViTMaskedAutoEncoderPL
    from adell_mri_amd.optim import FusedAdamW

    net = ViTMaskedAutoEncoderPL(image_key="image", **step_config("c1"))
    assert (net.learning_rate, net.weight_decay, net.warmup_steps, net.n_epochs) == (1e-3, 1e-6, 0, 100)
    assert net.model.mask_fraction == 0.75 and net.batch_size == 4
    opt = net.configure_optimizers()
    assert isinstance(opt, FusedAdamW)                       # the bare optimiser
    group = opt.param_groups[0]
    assert group["betas"] == (0.9, 0.95) and group["lr"] == 1e-3 and group["weight_decay"] == 1e-6
    # the positional embedding, under two state keys, is held once
    params = [p for g in opt.param_groups for p in g["params"]]
    assert sum(p is net.model.positional_embedding for p in params) == 1
    assert len(params) == len(list(net.parameters())) == len({id(p) for p in params})
    assert len(list(net.named_parameters(remove_duplicate=False))) == len(params) + 1
    flat = [p for f in opt.flat_groups for p in f.params]
    assert len(flat) == len(params) and sum(p is net.model.positional_embedding for p in flat) == 1
    warm = ViTMaskedAutoEncoderPL(image_key="image", warmup_steps=5, n_steps=50, learning_rate=2e-3,
                                  **step_config("c1"))
    conf = warm.configure_optimizers()
    assert isinstance(conf, dict) and isinstance(conf["optimizer"], FusedAdamW)
    assert conf["optimizer"].param_groups[0]["betas"] == (0.9, 0.95)
    sched = conf["lr_scheduler"]
    assert isinstance(sched["scheduler"], CosineAnnealingWithWarmupLR)
    assert sched["scheduler"].base_lrs == [2e-3] and sched["interval"] == "step"
    assert conf["optimizer"].defaults["lr"] == 0.0
    by_epoch = ViTMaskedAutoEncoderPL(image_key="image", warmup_steps=5, **step_config("c1"))
    assert by_epoch.configure_optimizers()["lr_scheduler"]["interval"] == "epoch"
    with pytest.raises(ValueError, match="training_dataloader_call"):
        net.train_dataloader()


# ---- the host checks -----------------------------------------------------------------------------------
def test_shuffle_refuses_on_the_host():
    from adell_mri_amd import ops

    ids = np.array([[2, 0, 1, 3], [3, 2, 1, 0]])
    s = ops.MaeShuffle(ids, 2, "cpu")
    assert (s.B, s.L, s.K) == (2, 4, 2) and s.keep.tolist() == [[2, 0], [3, 2]]
    assert s.restore.tolist() == [[1, 2, 0, 3], [3, 2, 1, 0]]
    assert s.inv.tolist() == [[1, -1, 0, -1], [-1, -1, 1, 0]]
    assert s.mask.tolist() == [[0.0, 1.0, 0.0, 1.0], [1.0, 1.0, 0.0, 0.0]]
    assert ops.MaeShuffle(torch.from_numpy(ids), 4, "cpu").mask.sum().item() == 0.0
    with pytest.raises(ValueError, match="permutation"):
        ops.MaeShuffle([[0, 1, 1, 3], [0, 1, 2, 3]], 2, "cpu")
    with pytest.raises(IndexError, match="index 4 is out of bounds for a sequence of 4 tokens"):
        ops.MaeShuffle([[0, 1, 2, 4], [0, 1, 2, 3]], 2, "cpu")
    with pytest.raises(IndexError, match="index -1 is out of bounds"):
        ops.MaeShuffle([[0, 1, 2, -1], [0, 1, 2, 3]], 2, "cpu")
    for bad in (0, 5, -1, 1.5):
        with pytest.raises(ValueError, match="len_keep"):
            ops.MaeShuffle(ids, bad, "cpu")
    with pytest.raises(TypeError, match="integer"):
        ops.MaeShuffle(ids.astype(np.float32), 2, "cpu")
    with pytest.raises(ValueError, match=r"\[B, L\]"):
        ops.MaeShuffle(ids[0], 2, "cpu")


def test_mae_fails_loudly_without_gpu():
    from adell_mri_amd import functional as HF, ops
    from adell_mri_amd.modules.self_supervised.pl import ViTMaskedAutoEncoderPL

    s = ops.MaeShuffle(np.array([[2, 0, 1, 3], [3, 2, 1, 0]]), 2, "cpu")
    x, enc = torch.zeros((2, 4, 6)), torch.zeros((2, 2, 6))
    token, scale, pos = torch.zeros((1, 1, 6)), torch.ones(1), torch.zeros((1, 4, 6))
    image = torch.zeros((2, 2, 3, 4))
    for call in (lambda: HF.mae_keep_tokens(x, s),
                 lambda: HF.mae_restore_tokens(enc, token, scale, pos, s),
                 lambda: HF.mae_reconstruction_loss(x, image, 3),
                 lambda: HF.mae_to_image(x, image.shape)):
        with pytest.raises(Exception, match="MI355X") as info:
            call()
        assert not isinstance(info.value, (ValueError, IndexError, NotImplementedError))
    # shape errors are ValueError, on the host
    with pytest.raises(ValueError, match="3 tokens for a shuffle of 4"):
        HF.mae_keep_tokens(x[:, :3], s)
    with pytest.raises(ValueError, match="a shuffle of 2 items"):
        HF.mae_keep_tokens(torch.zeros((3, 4, 6)), s)
    with pytest.raises(ValueError, match="rows for a shuffle with 2"):
        HF.mae_restore_tokens(x, token, scale, pos, s)
    with pytest.raises(ValueError, match="pos"):
        HF.mae_restore_tokens(enc, token, scale, pos[:, :3], s)
    with pytest.raises(ValueError, match="mask token"):
        HF.mae_restore_tokens(enc, token[..., :5], scale, pos, s)
    with pytest.raises(ValueError, match="do not divide"):
        HF.mae_reconstruction_loss(x, image, 5)
    with pytest.raises(ValueError, match="pred"):
        HF.mae_reconstruction_loss(x, image, 2)
    with pytest.raises(ValueError, match="image"):
        HF.mae_reconstruction_loss(x, image[0], 3)
    with pytest.raises(TypeError, match="MaeShuffle"):
        HF.mae_keep_tokens(x, [[0, 1], [1, 0]])
    # one channel: the image is a view, nothing is launched
    one = HF.mae_to_image(torch.arange(24.0).reshape(2, 4, 3), (2, 1, 3, 4))
    assert one.shape == (2, 1, 3, 4) and one.reshape(-1).tolist() == list(range(24))
    pl = ViTMaskedAutoEncoderPL(image_key="image", **step_config("c1"))
    for step in (pl.training_step, pl.validation_step, pl.test_step):
        with pytest.raises(Exception, match="MI355X"):
            step({"image": torch.zeros((2, 1, 16, 16))}, 0)


def test_step_runner_takes_a_bare_optimiser():
    """``trainer.StepRunner`` reads ``configure_optimizers()`` as a dict or as the optimiser itself."""
    from adell_mri_amd.modules.self_supervised.pl import ViTMaskedAutoEncoderPL
    from adell_mri_amd.optim import FusedAdamW
    from adell_mri_amd.trainer import StepRunner

    bare = StepRunner(ViTMaskedAutoEncoderPL(image_key="image", **step_config("c1")))
    assert isinstance(bare.optimizer, FusedAdamW) and bare.optimizer.defaults["lr"] == 1e-3
    warm = StepRunner(ViTMaskedAutoEncoderPL(image_key="image", warmup_steps=3, **step_config("c1")))
    assert isinstance(warm.optimizer, FusedAdamW) and warm.optimizer.defaults["lr"] == 0.0
