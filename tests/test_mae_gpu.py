"""The masked autoencoder on the GPU: the row kernels of csrc/mae.hip against plain indexing and the
fp64 restatement (tests/mae_ref.py), every result computed twice and compared bit for bit; one
transformer block at the sequence lengths a small keep count produces; one training step and a
following validation step of both fixture networks against the real reference
(tests/golden/mae_step.npz).

Tolerances are the project's for the same kinds of quantity (tests/test_ijepa_gpu.py,
tools/make_ijepa_golden.py): bit equality for copies and single adds, 5e-5 of the largest reference
magnitude for fixed-order sums and the loss; in the step tests loss 1e-4, gradients 5e-3 by
``cases.grad_rel_err``, parameters (2e-4, 2e-6) -- the fixture's own fp32-against-fp64 error uses at
most a quarter of them (recorded as ``<net>:fp32_vs_fp64``)."""
import copy

import numpy as np
import pytest
import torch

import mae_ref as MR
from cases import grad_rel_err
from mae_cases import B as STEP_B, CONFIGS, NETS, StepGold, fill, step_config
from oracle.weights import fill_state_dict
from test_ijepa_gpu import _block_reference

pytestmark = pytest.mark.gpu

SUM_BOUND = 5e-5


def rel(a, r):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(a).double()
    r = r.detach().double().cpu() if isinstance(r, torch.Tensor) else torch.as_tensor(r).double()
    return float((a - r).abs().max() / (r.abs().max() + 1e-300))


def uniform(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g) * (hi - lo) + lo


def twice(fn):
    """fn() run two times: the first result, after asserting that the second is bit-identical."""
    a, b = fn(), fn()
    a_, b_ = (a, b) if isinstance(a, (tuple, list)) else ((a,), (b,))
    assert all(torch.equal(u, v) for u, v in zip(a_, b_)), "two runs differ"
    return a


def shuffles(B, L, seed):
    """ids_shuffle [B, L]: another permutation for every item."""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(L) for _ in range(B)])
    if B > 1 and L > 2:
        assert len({tuple(r) for r in ids}) == B
    return ids


# ---- keep ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,E,K", [(1, 1, 1, 1), (3, 7, 5, 3), (2, 67, 64, 67), (2, 10, 260, 3),
                                     (2, 9, 770, 2)])
def test_keep_tokens(cuda, B, L, E, K):
    from adell_mri_amd import functional as HF, ops

    ids = shuffles(B, L, 100 * L + K)
    shuffle = ops.MaeShuffle(ids, K, cuda)
    x, r = uniform((B, L, E), 1), uniform((B, K, E), 2)

    def run():
        xd = x.to(cuda).requires_grad_(True)
        y = HF.mae_keep_tokens(xd, shuffle)
        y.backward(r.to(cuda))
        return y.detach(), xd.grad

    y, dx = twice(run)
    want = torch.stack([x[b, ids[b, :K]] for b in range(B)])
    assert y.shape == (B, K, E) and torch.equal(y.cpu(), want)
    assert torch.equal(want, MR.keep(x, ids, K).float())
    want_dx = torch.zeros_like(x)
    for b in range(B):
        want_dx[b, ids[b, :K]] = r[b]
    assert torch.equal(dx.cpu(), want_dx)          # zeros included: the whole gradient is written


def test_shuffle_is_refused_on_the_host(cuda, monkeypatch):
    from adell_mri_amd import functional as HF, ops

    launched = []
    real = ops.mae_gather_rows
    monkeypatch.setattr(ops, "mae_gather_rows", lambda *a: launched.append(1) or real(*a))
    x = torch.zeros((2, 4, 8), device=cuda)
    with pytest.raises(IndexError, match="index 4 is out of bounds for a sequence of 4 tokens"):
        ops.MaeShuffle([[0, 1, 2, 4], [0, 1, 2, 3]], 2, cuda)
    with pytest.raises(ValueError, match="permutation"):
        ops.MaeShuffle([[0, 1, 1, 3], [0, 1, 2, 3]], 2, cuda)
    with pytest.raises(ValueError, match="len_keep"):
        ops.MaeShuffle([[0, 1, 2, 3], [0, 1, 2, 3]], 5, cuda)
    good = ops.MaeShuffle([[3, 1, 2, 0], [0, 1, 2, 3]], 2, cuda)
    with pytest.raises(ValueError, match="5 tokens for a shuffle of 4"):
        HF.mae_keep_tokens(torch.zeros((2, 5, 8), device=cuda), good)
    with pytest.raises(ValueError, match="a shuffle of 2 items"):
        HF.mae_keep_tokens(torch.zeros((3, 4, 8), device=cuda), good)
    assert launched == []                      # raised on the host, before any launch
    assert HF.mae_keep_tokens(x, good).shape == (2, 2, 8) and launched == [1]


# ---- restore ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,E,K", [(1, 2, 1, 1), (3, 16, 16, 4), (2, 12, 64, 12), (2, 9, 250, 2),
                                     (2, 10, 260, 3)])
def test_restore_tokens(cuda, B, L, E, K):
    from adell_mri_amd import functional as HF, ops

    ids = shuffles(B, L, 100 * L + K + 7)
    shuffle = ops.MaeShuffle(ids, K, cuda)
    restore_ids = shuffle.restore_host
    visible = torch.from_numpy(restore_ids < K)                    # [B, L]
    enc, token, pos = uniform((B, K, E), 3), uniform((1, 1, E), 4, -0.5, 0.5), uniform((1, L, E), 5, 0, 1)
    scale = torch.tensor([0.75])
    r = uniform((B, L, E), 6)

    def run():
        leaves = [t.to(cuda).requires_grad_(True) for t in (enc, token, scale, pos)]
        out = HF.mae_restore_tokens(*leaves, shuffle)
        out.backward(r.to(cuda))
        return (out.detach(), *[t.grad for t in leaves])

    out, denc, dtoken, dscale, dpos = twice(run)
    ref = [t.double().requires_grad_(True) for t in (enc, token, scale, pos)]
    want = MR.restore(*ref, ids)
    (want * r.double()).sum().backward()
    want_enc, want_token, want_scale, want_pos = [t.grad for t in ref]
    assert out.shape == want.shape == (B, L, E)
    # visible rows: one fp32 add per element, exact
    single = torch.stack([enc[b, np.minimum(restore_ids[b], K - 1)] for b in range(B)]) + pos
    assert torch.equal(out.cpu()[visible], single[visible])
    assert torch.equal(out.cpu()[visible], want.detach().float()[visible])
    assert rel(out, want) < SUM_BOUND                              # the masked rows with them
    assert denc.shape == enc.shape and torch.equal(denc.cpu(), want_enc.float())
    assert dpos.shape == pos.shape and rel(dpos, want_pos) < SUM_BOUND
    assert dtoken.shape == token.shape and dscale.shape == scale.shape
    if K == L:          # no masked row: both gradients exactly zero
        assert float(dtoken.abs().max()) == 0.0 and float(dscale.abs().max()) == 0.0
        assert want_token is None or float(want_token.abs().max()) == 0.0
    else:
        err_token, err_scale = rel(dtoken, want_token), rel(dscale, want_scale)
        print(f"({B},{L},{E},{K}): dpos {rel(dpos, want_pos):.2e}, dmask_token {err_token:.2e}, "
              f"dscale {err_scale:.2e}")
        assert err_token < SUM_BOUND and err_scale < SUM_BOUND

    # only what is asked for is computed
    leaves = [t.to(cuda) for t in (enc, token, scale, pos)]
    leaves[1].requires_grad_(True)
    HF.mae_restore_tokens(*leaves, shuffle).backward(r.to(cuda))
    assert torch.equal(leaves[1].grad, dtoken) and all(t.grad is None for t in (leaves[0], leaves[2], leaves[3]))


# ---- reconstruction loss and image layout ------------------------------------------------------------
def _patch(P):
    ph = max(d for d in range(1, int(P ** 0.5) + 1) if P % d == 0)
    return ph, P // ph


@pytest.mark.parametrize("B,C,L,P", [(1, 1, 1, 1), (1, 1, 5, 7), (3, 1, 16, 16), (2, 2, 12, 32),
                                     (2, 3, 4, 16), (2, 1, 64, 64)])
def test_reconstruction_loss_and_image(cuda, B, C, L, P):
    from adell_mri_amd import functional as HF

    ph, pw = _patch(P)
    H, W = L, P                                   # any H W = L P: the map is flat per (b, c) plane
    pred, x = uniform((B, L, P * C), 7), uniform((B, C, H, W), 8)
    r = uniform((B, C, H, W), 9)

    def run():
        pd = pred.to(cuda).requires_grad_(True)
        loss = HF.mae_reconstruction_loss(pd, x.to(cuda), P)
        (loss * 1.5).backward()
        return loss.detach(), pd.grad

    loss, dpred = twice(run)
    pr = pred.double().requires_grad_(True)
    want = MR.loss(pr, x)
    want.backward()
    assert loss.ndim == 0 and dpred.shape == pred.shape
    print(f"({B},{C},{L},{P}): loss {abs(loss.item() - want.item()) / abs(want.item()):.2e}, "
          f"dpred {rel(dpred, 1.5 * pr.grad):.2e}")
    np.testing.assert_allclose(loss.item(), want.item(), rtol=SUM_BOUND)
    assert rel(dpred, 1.5 * pr.grad) < SUM_BOUND

    def image():
        pd = pred.to(cuda).requires_grad_(True)
        out = HF.mae_to_image(pd, (B, C, H, W))
        out.backward(r.to(cuda))
        return out.detach(), pd.grad, out.data_ptr() == pd.data_ptr()

    chain = pred.view(B, L, ph, pw, C).permute(0, 4, 1, 2, 3).contiguous().view(B, C, H, W)
    a, b = image(), image()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    out, dtokens, is_view = a
    assert out.shape == (B, C, H, W) and torch.equal(out.cpu(), chain)
    assert is_view == (C == 1)                  # one channel: a view, nothing launched
    want_d = r.view(B, C, L, ph, pw).permute(0, 2, 3, 4, 1).contiguous().view(B, L, P * C)
    assert torch.equal(dtokens.cpu(), want_d)
    # the loss of the image equals the fused loss
    composed = torch.nn.functional.mse_loss(chain.double(), x.double())
    np.testing.assert_allclose(loss.item(), composed.item(), rtol=SUM_BOUND)


# ---- one transformer block at the encoder's shortest sequences ---------------------------------------
@pytest.mark.parametrize("tokens", [1, 4])
def test_transformer_block_at_short_sequences(cuda, tokens):
    """The encoder block of fixture network c1 (width 16, 2 heads) on 1 and 4 kept tokens, forward
    and backward against fp64 at the bounds of tests/test_ijepa_gpu.py: output 1e-5, gradients 5e-5
    of their largest entry."""
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.layers.vit import TransformerBlock

    block = TransformerBlock(16, 16, 32, n_heads=2, mlp_structure=[32],
                             adn_fn=get_adn_fn(1, "identity", "gelu", 0.0))
    sd = fill_state_dict(block.state_dict(), gain=1.5, norm_weight_offset=1.0)
    block.load_state_dict(sd)
    block = block.to(cuda).train()
    x, r = uniform((3, tokens, 16), tokens), uniform((3, tokens, 16), tokens + 1)
    xd = x.to(cuda).requires_grad_(True)
    y = block(xd)
    y.backward(r.to(cuda))
    ref = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    xr = x.double().requires_grad_(True)
    want = _block_reference(ref, xr, 2)
    want.backward(r.double())
    errs = {"out": rel(y, want), "dx": rel(xd.grad, xr.grad)}
    for k, p in block.named_parameters():
        errs[k] = rel(p.grad, ref[k].grad)
    # exactly zero in exact arithmetic: the k-norm bias (one bias on every key moves a whole row of
    # scores, which the softmax ignores) is compared against the k-norm weight's gradient, the tensor
    # the same kernel writes beside it, as tests/test_ijepa_gpu.py does; with ONE token the softmax of
    # one score is constant, so all four q / k norm gradients vanish, and they are compared against
    # the gradient of the qkv weight, which the same backward pass feeds
    got = dict(block.named_parameters())
    for k in ("mha.k_norm.bias", "mha.k_norm.weight", "mha.q_norm.weight", "mha.q_norm.bias"):
        if float(ref[k].grad.abs().max()) < 1e-12:
            assert k == "mha.k_norm.bias" or tokens == 1, k
            scale = ref["mha.k_norm.weight" if tokens > 1 else "mha.qkv.weight"].grad.abs().max()
            errs[k] = float((got[k].grad.double().cpu() - ref[k].grad).abs().max() / scale)
    print(tokens, {k: f"{e:.2e}" for k, e in errs.items()})
    assert errs.pop("out") < 1e-5
    bad = {k: e for k, e in errs.items() if not e < 5e-5}
    assert not bad, bad


# ---- the modules' own forwards -----------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_random_masking_on_the_device(cuda, name):
    """``random_masking(x, mask_ratio, rng)`` with the reference's seed: the kept rows of every item in
    its shuffled order, the recorded mask and ids_restore, for both draws."""
    from adell_mri_amd.modules.self_supervised.autoencoders import random_masking

    g, (cfg, L, E, K) = StepGold(name), CONFIGS[name]
    rng = np.random.default_rng(int(g.top["seed"]))
    x = uniform((STEP_B, L, E), 11)
    for i in range(2):
        ids = g[f"ids_shuffle{i}"]
        x_masked, mask, ids_restore = random_masking(x.to(cuda), cfg["mask_fraction"], rng)
        assert x_masked.shape == (STEP_B, K, E) and ids_restore.dtype == torch.int64
        assert torch.equal(x_masked.cpu(), torch.stack([x[b, ids[b, :K]] for b in range(STEP_B)]))
        assert torch.equal(mask.cpu(), torch.from_numpy(g[f"mask{i}"]))
        assert np.array_equal(ids_restore.cpu().numpy(), np.argsort(ids, axis=1, kind="stable"))


def test_autoencoder_without_masking(cuda):
    """``ViTAutoEncoder.forward`` against the masked autoencoder that keeps every token: the blocks
    carry no positional information of their own, so encoding the shuffled tokens and putting them
    back is encoding them in place. Two fp32 evaluations that differ in the order of the attention
    sums: the output bound of the transformer-block tests, 1e-5 of the largest entry."""
    from adell_mri_amd.modules.self_supervised.autoencoders import ViTAutoEncoder, ViTMaskedAutoEncoder

    g, cfg = StepGold("c2"), step_config("c2")
    masked = ViTMaskedAutoEncoder(**{**cfg, "mask_fraction": 0.0})
    sd = fill(masked.state_dict(), float(g["gain"]))
    masked.load_state_dict(sd)
    del cfg["mask_fraction"]
    plain = ViTAutoEncoder(**cfg)
    plain.load_state_dict({k: v for k, v in sd.items() if not k.startswith("mask_token")})
    assert list(plain.state_dict()) == [k for k in sd if not k.startswith("mask_token")]
    masked, plain = masked.to(cuda).eval(), plain.to(cuda).eval()
    x = torch.from_numpy(g["x"]).to(cuda)
    with torch.no_grad():
        want, mask = masked.forward_tokens(x)
        got = plain(x)
    assert float(mask.abs().max()) == 0.0 and got.shape == want.shape == (STEP_B, 12, 64)
    assert rel(got, want) < 1e-5


# ---- one training step -------------------------------------------------------------------------------
def build_pl(name, cuda):
    """The wrapper of one fixture network with the fixture's weights, in ``eval()`` mode as the
    fixture's steps (the stacks' default ``adn_fn`` carries a dropout of 0.1 that the MAE arguments
    cannot turn off: tools/make_mae_golden.py)."""
    from adell_mri_amd.modules.self_supervised.pl import ViTMaskedAutoEncoderPL

    g = StepGold(name)
    net = ViTMaskedAutoEncoderPL(image_key="image", **step_config(name))
    assert list(net.model.state_dict()) == [str(k) for k in g["state_keys"]]
    net.model.load_state_dict(fill(net.model.state_dict(), float(g["gain"])))
    net = net.to(cuda).eval()
    assert net.model.positional_embedding is net.model.proj.positional_embedding
    return net, g, {"image": torch.from_numpy(g["x"]).to(cuda)}


@pytest.mark.parametrize("name", NETS)
def test_training_step_matches_reference(cuda, name):
    """``forward`` (embedding, per-item shuffle, the encoder on the kept tokens, the un-shuffle with
    the scaled mask token, decoder, head, image layout), then ``training_step`` through
    ``StepRunner`` (bare optimiser): loss, every parameter gradient -- the positional embedding's is
    the sum of its two uses -- and one FusedAdamW step with betas (0.9, 0.95); then a validation
    step, which must draw the recorded second shuffle from the module's own rng."""
    from adell_mri_amd.optim import FusedAdamW
    from adell_mri_amd.trainer import StepRunner

    net, g, batch = build_pl(name, cuda)
    cfg, L, E, K = CONFIGS[name]
    seed = int(g.top["seed"])
    with torch.no_grad():       # the outputs with the step's first draw, then the draw again
        pred, mask = net.model.forward_tokens(batch["image"])
        assert pred.shape == g["pred"].shape == (STEP_B, L, E)
        assert torch.equal(mask.cpu(), torch.from_numpy(g["mask0"])) and mask.dtype == torch.float32
        assert int((mask == 0).sum()) == STEP_B * K
        assert rel(pred, g["pred"]) < 1e-4
        net.model.rng = np.random.default_rng(seed)
        recon, mask = net(batch["image"])
        assert recon.shape == g["recon"].shape and rel(recon, g["recon"]) < 1e-4
        assert torch.equal(mask.cpu(), torch.from_numpy(g["mask0"]))
        composed = torch.nn.MSELoss()(recon.double().cpu(), torch.from_numpy(g["x"]).double())
        np.testing.assert_allclose(composed.item(), g["loss"], rtol=1e-4)
    net.model.rng = np.random.default_rng(seed)
    runner = StepRunner(net)
    assert isinstance(runner.optimizer, FusedAdamW)
    assert runner.optimizer.param_groups[0]["betas"] == (0.9, 0.95)
    runner.optimizer.zero_grad()
    loss = net.training_step(batch, 0)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-4)
    loss.backward()
    params = list(net.model.named_parameters())
    assert [k for k, _ in params] == [str(k) for k in g["param_keys"]]
    assert sum(k.startswith("grad:") for k in g.files) == len(params)
    worst = 0.0
    for k, p in params:
        e = grad_rel_err(g, k, p.grad.cpu().numpy())
        worst = max(worst, e)
        assert e < 5e-3, (k, e)
    print(f"{name}: loss {abs(loss.item() - g['loss']) / g['loss']:.2e}, worst gradient {worst:.2e}")
    runner.optimizer.step()
    for k, p in params:
        np.testing.assert_allclose(p.detach().cpu().numpy(), g["step1:" + k], rtol=2e-4, atol=2e-6,
                                   err_msg=k)
    assert net.model.positional_embedding is net.model.proj.positional_embedding
    # a validation step: the second draw of the same rng, no gradient
    ahead = copy.deepcopy(net.model.rng)
    drawn = np.argsort(ahead.uniform(size=[STEP_B, L]), axis=1, kind="stable")
    np.testing.assert_array_equal(drawn, g["ids_shuffle1"])
    grads = {k: None if p.grad is None else p.grad.clone() for k, p in params}
    with torch.no_grad():
        val = net.validation_step(batch, 0)
    np.testing.assert_allclose(val.item(), g["val_loss"], rtol=1e-4)
    assert not val.requires_grad
    assert net.model.rng.bit_generator.state == ahead.bit_generator.state      # exactly one draw
    for k, p in params:
        assert (p.grad is None) if grads[k] is None else torch.equal(p.grad, grads[k]), k


def test_training_mode_step_runs_with_the_stacks_default_dropout(cuda):
    """In ``train()`` mode the MLPs of both stacks drop 10 % of their hidden units (the default
    ``adn_fn``, which the MAE arguments cannot replace -- as in the reference): the step runs, every
    parameter receives a finite gradient, and the loss is not the ``eval()`` loss of the same draw."""
    net, g, batch = build_pl("c1", cuda)
    net.train()
    drops = [m.p for m in net.modules() if isinstance(m, torch.nn.Dropout) and m.p > 0]
    assert drops and set(drops) == {0.1}
    loss = net.training_step(batch, 0)
    loss.backward()
    assert torch.isfinite(loss) and abs(loss.item() - float(g["loss"])) > 1e-4 * float(g["loss"])
    for k, p in net.model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k

