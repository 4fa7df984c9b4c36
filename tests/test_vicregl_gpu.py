"""VICRegL on the device: the top-gamma pair ranking (csrc/vicregl.hip) against the plain-torch
restatement (tests/vicregl_ref.py) with the indices compared exactly, the row gather's backward
under duplicates, the loss against the fixtures of the real reference
(tools/make_vicregl_golden.py) and the training step of the wrappers that build it.

A ranking is compared only where it is pinned: the restatement runs in fp64 on the fp32 inputs, the
kernel's squared distances carry fp32 rounding (relative 1e-6 at these channel counts), so the
inputs are walked (a few seeds) until the distances next to the gamma-th largest are 1e-5 apart in
relative terms -- exact ties excepted, which the kernel reproduces exactly (identical rows give
identical sums) and orders by flat index."""
import os

import numpy as np
import pytest
import torch

import vicregl_ref as R
from cases import grad_rel_err
from oracle.weights import fill_state_dict

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SSL_GAIN = 3.0
SSL_OPT = dict(learning_rate=1e-3, weight_decay=5e-3, optimizer_eps=1e-8)


def pinned(d2, gamma, tol=1e-5):
    """Every item: the distances below the gamma-th largest are tol (relative) away from it -- and,
    where the gamma-th largest is an exact tie, so are the distances above it (the tie's members
    are ordered by flat index; what is above a lone gamma-th value is selected whatever its order)."""
    v = d2.flatten(1).sqrt()
    for row in v:
        t = torch.sort(row, descending=True).values[gamma - 1]
        above, below = row[row > t], row[row < t]
        tied = int((row == t).sum()) > 1
        if tied and above.numel() and float((above.min() - t) / t) < tol:
            return False
        if below.numel() and float((t - below.max()) / t) < tol:
            return False
    return True


def flat_sets(pairs, T):
    p = pairs.detach().cpu().long()
    return torch.sort(p[..., 0] * T + p[..., 1], 1).values


def check_ranking(pairs, dist2, d2_ref, gamma):
    """pairs int32 [B, gamma, 2] of the kernel against the fp64 matrix: the same SET of pairs, the
    documented order on the kernel's own distances, the distances themselves."""
    T = d2_ref.shape[-1]
    want = R.top_pairs(d2_ref, gamma)
    assert torch.equal(flat_sets(pairs, T), flat_sets(want, T))
    p, d = pairs.cpu().long(), dist2.cpu()
    flat = p[..., 0] * T + p[..., 1]
    ok = (d[:, :-1] > d[:, 1:]) | ((d[:, :-1] == d[:, 1:]) & (flat[:, :-1] < flat[:, 1:]))
    assert bool(ok.all())
    ref = torch.gather(d2_ref.flatten(1), 1, flat)
    np.testing.assert_allclose(d.numpy(), ref.numpy(), rtol=1e-5)


def feature_inputs(B, T, C, gamma, seed0):
    for seed in range(seed0, seed0 + 20):
        g = torch.Generator().manual_seed(seed)
        a = torch.randn((B, T, C), generator=g)
        b = 0.5 * a + torch.randn((B, T, C), generator=g)
        d2 = R.sq_dists(a.double(), b.double())
        if pinned(d2, gamma):
            return a, b, d2
    raise AssertionError("no pinned input in 20 seeds")


# T = 60: one partial 64 x 64 tile; T = 400: 7 strips x several column runs and the merge
@pytest.mark.parametrize("spatial,C,gamma", [((3, 4, 5), 5, 1), ((3, 4, 5), 5, 10),
                                             ((20, 20), 24, 10), ((20, 20), 24, 64)])
def test_top_pairs_match_the_restatement(cuda, spatial, C, gamma):
    from adell_mri_amd import ops

    T = int(np.prod(spatial))
    a, b, d2 = feature_inputs(3, T, C, gamma, 10 * T + gamma)
    pairs, dist2 = ops.top_pairs(a.to(cuda), b.to(cuda), gamma, return_dist2=True)
    assert pairs.dtype == torch.int32 and tuple(pairs.shape) == (3, gamma, 2)
    check_ranking(pairs, dist2, d2, gamma)


def test_top_pairs_break_ties_by_flat_index_and_repeat_bit_for_bit(cuda):
    """Rows 3 and 7 of view 1 are one outlier token twice: d(3, j) == d(7, j) exactly, the largest
    distances come in tied couples and an odd gamma cuts the last couple -- the lower flat index
    (row 3) stays."""
    from adell_mri_amd import ops

    T, C, gamma = 60, 5, 9
    for seed in range(20):
        g = torch.Generator().manual_seed(seed)
        a = torch.randn((2, T, C), generator=g)
        b = torch.randn((2, T, C), generator=g)
        a[:, 3] *= 10.0
        a[:, 7] = a[:, 3]
        d2 = R.sq_dists(a.double(), b.double())
        if pinned(d2, gamma):
            break
    else:
        raise AssertionError("no pinned input in 20 seeds")
    want = R.top_pairs(d2, gamma)
    assert sorted(want[0, :, 0].tolist()) == [3] * 5 + [7] * 4       # the cut couple keeps row 3
    runs = [ops.top_pairs(a.to(cuda), b.to(cuda), gamma, return_dist2=True) for _ in range(2)]
    check_ranking(runs[0][0], runs[0][1], d2, gamma)
    # the full order, ties included, is the restatement's
    assert torch.equal(runs[0][0].cpu().long(), want)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("spatial", [(5, 6), (3, 4, 5)])
def test_top_pairs_of_box_coordinates(cuda, spatial):
    from adell_mri_amd import ops

    ndim, B, gamma = len(spatial), 3, 10
    for seed in range(20):
        g = torch.Generator().manual_seed(100 + seed)
        lo1, lo2 = 20.0 * torch.rand((B, ndim), generator=g), 20.0 * torch.rand((B, ndim), generator=g)
        b1 = torch.cat([lo1, lo1 + 16.0 + 32.0 * torch.rand((B, ndim), generator=g)], 1)
        b2 = torch.cat([lo2, lo2 + 8.0 + 16.0 * torch.rand((B, ndim), generator=g)], 1)   # unequal sizes
        d2 = R.sq_dists(R.grid_coords(spatial, b1.double()), R.grid_coords(spatial, b2.double()))
        if pinned(d2, gamma):
            break
    else:
        raise AssertionError("no pinned boxes in 20 seeds")
    pairs, dist2 = ops.top_pairs_boxes(b1.to(cuda), b2.to(cuda), spatial, gamma, return_dist2=True)
    check_ranking(pairs, dist2, d2, gamma)


def test_top_pairs_reject_what_the_kernel_does_not_do(cuda):
    from adell_mri_amd import ops

    a = torch.zeros((1, 3, 4), device=cuda)
    with pytest.raises(ValueError):
        ops.top_pairs(a, a, 65)
    with pytest.raises(ValueError):
        ops.top_pairs(a, a, 10)          # 9 pairs only


def test_gather_rows_backward_adds_duplicates_in_a_fixed_order(cuda):
    """One token of view 1 scaled x 10: most selected pairs share its row."""
    from adell_mri_amd import functional as HF

    B, T, C, gamma = 2, 60, 24, 10
    for seed in range(20):
        g = torch.Generator().manual_seed(seed)
        a, b = torch.randn((B, T, C), generator=g), torch.randn((B, T, C), generator=g)
        a[:, 11] *= 10.0
        d2 = R.sq_dists(a.double(), b.double())
        if pinned(d2, gamma):
            break
    else:
        raise AssertionError("no pinned input in 20 seeds")
    want = R.top_pairs(d2, gamma)
    assert all(len(set(r.tolist())) < gamma / 2 for r in want[..., 0])        # duplicates
    w = torch.randn((B * gamma, C), generator=torch.Generator().manual_seed(1))
    grads = []
    for _ in range(2):
        x = a.to(cuda).requires_grad_(True)
        pairs = HF.top_pairs(x, b.to(cuda), gamma)
        assert not pairs.requires_grad
        assert torch.equal(flat_sets(pairs, T), flat_sets(want, T))
        rows = pairs[..., 0].cpu().long()           # in the kernel's order of the pairs
        out = HF.gather_rows(x, pairs, 0)
        assert torch.equal(out.detach().cpu(), R.gather_rows(a, rows))
        (out * w.to(cuda)).sum().backward()
        grads.append(x.grad.clone())
    assert torch.equal(grads[0], grads[1])
    ref = torch.zeros((B, T, C), dtype=torch.float64)
    for bi in range(B):
        ref[bi].index_add_(0, rows[bi], w.double().view(B, gamma, C)[bi])
    np.testing.assert_allclose(grads[0].cpu().numpy(), ref.numpy(), rtol=1e-6, atol=1e-7)


# (B >= 128 rows, what B * gamma gathered rows reach: column statistics + tiled Gram matrix + fold,
# csrc/ssl.hip; 128 and 130: whole and partial 64-row tiles, D = 24 and 300: partial 32-column chunks;
# construction and tolerance of tests/test_ssl.py::test_vicreg_loss_matches_oracle_at_other_sizes)
@pytest.mark.parametrize("B,D", [(128, 24), (130, 300), (320, 512)])
def test_vicreg_terms_on_many_rows_match_oracle(cuda, B, D):
    from adell_mri_amd.modules.self_supervised.losses import VICRegLoss
    from oracle.torch_ref.convnext import vicreg_loss

    gen = torch.Generator().manual_seed(B * D)
    a = torch.randn((B, D), generator=gen, dtype=torch.float64).requires_grad_(True)
    b = (0.3 * a.detach() + torch.randn((B, D), generator=gen, dtype=torch.float64)
         ).requires_grad_(True)
    ref = vicreg_loss(a, b)
    sum(ref).backward()
    x1 = a.detach().float().to(cuda).requires_grad_(True)
    x2 = b.detach().float().to(cuda).requires_grad_(True)
    terms = VICRegLoss()(x1, x2)
    np.testing.assert_allclose(torch.stack(terms).detach().cpu().numpy(),
                               torch.stack(ref).detach().numpy(), rtol=5e-5)
    sum(terms).backward()
    assert rel(x1.grad, a.grad.numpy()) < 5e-5 and rel(x2.grad, b.grad.numpy()) < 5e-5


# ---- the loss against the real reference ----------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "vicregl_loss.npz"), allow_pickle=False)


def rel(a, r):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-30))


def channels_last(x, cuda):
    fmt = torch.channels_last_3d if x.dim() == 5 else torch.channels_last
    return x.to(cuda).contiguous(memory_format=fmt)


@pytest.mark.parametrize("detach2", [False, True])
@pytest.mark.parametrize("layout", ["channels_last", "channels_first"])
@pytest.mark.parametrize("name", ["a3d", "b2d", "c3d"])
def test_loss_terms_grads_and_indices_match_the_reference(cuda, gold, name, layout, detach2):
    """Tolerances: those of tests/test_ssl.py for the VICReg terms and their input gradients
    against the reference fixture (terms rtol 2e-5, gradients 2e-5 of the largest entry)."""
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.self_supervised.losses import VICRegLocalLoss
    from adell_mri_amd.modules.self_supervised.losses.vicreg import _tokens

    g = gold
    gamma = int(g[f"{name}:gamma"])
    put = (lambda x: channels_last(x, cuda)) if layout == "channels_last" else (lambda x: x.to(cuda))
    x1 = put(torch.from_numpy(g[f"{name}:x1"])).requires_grad_(True)
    x2 = put(torch.from_numpy(g[f"{name}:x2"])).requires_grad_(not detach2)
    b1, b2 = torch.from_numpy(g[f"{name}:box1"]).to(cuda), torch.from_numpy(g[f"{name}:box2"]).to(cuda)
    loss = VICRegLocalLoss(gamma=gamma)
    # the selected rows, as multisets: rows for (X1, X2), columns for (X2, X1)
    with torch.no_grad():
        picked = {"loc": HF.top_pairs_boxes(b1, b2, x1.shape[2:], gamma),
                  "feat": HF.top_pairs(_tokens(x1), _tokens(x2), gamma)}
    for kind, pairs in picked.items():
        for tag, col in ((f"{kind}12", 0), (f"{kind}21", 1)):
            got = np.sort(pairs[..., col].cpu().numpy(), 1)
            assert np.array_equal(got, g[f"{name}:rows_{tag}"]), tag
    terms = loss(x1, x2, b1, b2)
    assert len(terms) == 4
    np.testing.assert_allclose(torch.stack(terms).detach().cpu().numpy(), g[f"{name}:terms"],
                               rtol=2e-5)
    sum(terms).backward()
    assert rel(x1.grad, g[f"{name}:dx1"]) < 2e-5
    if detach2:
        assert x2.grad is None
    else:
        assert rel(x2.grad, g[f"{name}:dx2"]) < 2e-5
    # the parts, by the reference's signatures: short + long of both directions is the local term
    with torch.no_grad():
        parts = (loss.location_local_loss(x1, x2, b1, b2) + loss.location_local_loss(x2, x1, b2, b1)
                 + loss.feature_local_loss(x1, x2) + loss.feature_local_loss(x2, x1)) * 0.1 / 2
    np.testing.assert_allclose(float(parts), float(g[f"{name}:terms"][3]), rtol=2e-5)


# ---- training steps --------------------------------------------------------------------------------
def build_resnet2d(cuda, **kw):
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.self_supervised.pl import SelfSLResNetPL

    adn, adn1 = get_adn_fn(2, "batch", "swish", 0.0), get_adn_fn(1, "layer", "gelu", 0.0)
    net = SelfSLResNetPL(
        aug_image_key_1="a", aug_image_key_2="b", box_key_1="box_a", box_key_2="box_b",
        ssl_method="vicregl", n_epochs=10, batch_size=4, **SSL_OPT, **kw,
        backbone_args=dict(spatial_dim=2, in_channels=1, structure=[[8, 8, 5, 2], [16, 16, 3, 2]],
                           maxpool_structure=[[2, 2], [2, 2]], res_type="resnet", adn_fn=adn),
        projection_head_args=dict(in_channels=16, structure=[32, 24], adn_fn=adn1),
        prediction_head_args=dict(in_channels=24, structure=[32, 24], adn_fn=adn1))
    net.load_state_dict(fill_state_dict(net.state_dict(), gain=SSL_GAIN))
    return net.to(cuda).train()


def step_batch(g, cuda):
    return {"a": torch.from_numpy(g["x1"]).to(cuda), "b": torch.from_numpy(g["x2"]).to(cuda),
            "box_a": torch.from_numpy(g["box1"]).to(cuda), "box_b": torch.from_numpy(g["box2"]).to(cuda)}


def test_resnet2d_vicregl_step_matches_reference(cuda):
    """The 2-D ResNet of tests/test_ssl.py::test_resnet2d_vicreg_step_matches_reference with
    ssl_method="vicregl" and boxes in the batch, at that test's tolerances."""
    from adell_mri_amd.modules.self_supervised.losses import VICRegLocalLoss
    from adell_mri_amd.trainer import StepRunner

    g = np.load(os.path.join(GOLD, "ssl_resnet2d_vicregl.npz"), allow_pickle=False)
    for tag in ("loc12", "loc21", "feat12", "feat21"):      # the fixture's own condition
        assert (g[f"gap_{tag}"] >= 5e-3).all(), tag
    net = build_resnet2d(cuda, stop_gradient=False, ema=None,
                         vic_reg_loss_params={"gamma": int(g["gamma"])})
    assert isinstance(net.loss, VICRegLocalLoss) and net.loss.gamma == int(g["gamma"])
    batch = step_batch(g, cuda)
    assert tuple(net(batch["a"], ret="representation").shape) == tuple(g["representation_shape"])
    loss = net.training_step(batch, 0)
    assert len(net.last_losses) == 4
    np.testing.assert_allclose(torch.stack(list(net.last_losses)).detach().cpu().numpy(),
                               g["losses"], rtol=5e-4, atol=1e-6)
    loss.backward()
    keys = set(g["grad_keys"].tolist())
    for k, p in net.named_parameters():
        if k in keys:
            assert grad_rel_err(g, k, p.grad.cpu().numpy()) < 5e-3, k
        else:                      # the heads take no part in this loss
            assert p.grad is None, k
    net.zero_grad()
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    after = StepRunner(net).train_step(batch)
    assert np.isfinite(float(after.detach()))
    moved = [k for k, p in net.named_parameters() if not torch.equal(before[k], p.detach())]
    assert moved and all(k in keys for k in moved)
    assert np.isfinite(float(net.training_step(batch, 1).detach()))


def test_resnet2d_vicregl_stop_gradient_step_runs(cuda):
    """The default stop_gradient=True with an EMA target: view 2 goes through the shadow under
    no_grad, which gets no gradient; the online network does."""
    from adell_mri_amd.utils import ExponentialMovingAverage

    g = np.load(os.path.join(GOLD, "ssl_resnet2d_vicregl.npz"), allow_pickle=False)
    net = build_resnet2d(cuda, ema=None, vic_reg_loss_params={"gamma": int(g["gamma"])})
    assert net.stop_gradient is True
    net.ema = ExponentialMovingAverage(0.9)
    net.ema.update(net)
    batch = step_batch(g, cuda)
    loss = net.training_step(batch, 0)
    assert len(net.last_losses) == 4 and np.isfinite(float(loss.detach()))
    loss.backward()
    for _, p in net.ema.shadow.named_parameters():
        assert p.grad is None and not p.requires_grad
    assert net.backbone.input_layer[0].weight.grad is not None
    # without a target network the second view is the same network under no_grad
    net.ema = None
    net.zero_grad()
    loss = net.training_step(batch, 1)
    loss.backward()
    assert np.isfinite(float(loss)) and net.backbone.input_layer[0].weight.grad is not None


def test_selfsl_unet_vicregl_step(cuda):
    """SelfSLUNetPL: forward(x) is the bottleneck map; the four terms against the restatement on
    the module's own maps (tolerances of tests/test_ssl.py::test_selfsl_unet_vicreg_step)."""
    from adell_mri_amd.modules.activations import activation_factory
    from adell_mri_amd.modules.self_supervised.pl import SelfSLUNetPL
    from adell_mri_amd.trainer import StepRunner

    torch.manual_seed(0)
    gamma = 5
    net = SelfSLUNetPL(aug_image_key_1="a", aug_image_key_2="b", box_key_1="box_a", box_key_2="box_b",
                       ssl_method="vicregl", vic_reg_loss_params={"gamma": gamma},
                       stop_gradient=False, learning_rate=1e-3, weight_decay=1e-3,
                       spatial_dimensions=3, depth=[8, 16, 32], kernel_sizes=[3, 3, 3],
                       strides=[2, 2, 2], norm_type="instance", padding=1, in_channels=1,
                       activation_fn=activation_factory["swish"], dropout_param=0.0).to(cuda).train()
    zz = torch.arange(16.0)[None, None, :, None, None]
    for seed in range(3, 23):
        g = torch.Generator().manual_seed(seed)
        x1 = torch.stack([torch.sin((b + 1) * 0.4 * zz[0]) + 0.3 * torch.rand((1, 16, 16, 16), generator=g)
                          for b in range(4)])
        x2 = x1 + 0.2 * torch.randn(x1.shape, generator=g)
        lo1, lo2 = 20.0 * torch.rand((4, 3), generator=g), 20.0 * torch.rand((4, 3), generator=g)
        b1 = torch.cat([lo1, lo1 + 16.0 + 32.0 * torch.rand((4, 3), generator=g)], 1)
        b2 = torch.cat([lo2, lo2 + 16.0 + 32.0 * torch.rand((4, 3), generator=g)], 1)
        batch = {"a": x1.to(cuda), "b": x2.to(cuda), "box_a": b1.to(cuda), "box_b": b2.to(cuda)}
        with torch.no_grad():
            y1, y2 = net(batch["a"]).cpu().double(), net(batch["b"]).cpu().double()
        # (the maps carry the encoder's fp32 error, 1e-4 of their scale: pinned an order above it)
        if (pinned(R.sq_dists(R.tokens(y1), R.tokens(y2)), gamma, 5e-3)
                and pinned(R.sq_dists(R.grid_coords(y1.shape[2:], b1.double()),
                                      R.grid_coords(y1.shape[2:], b2.double())), gamma)):
            break
    else:
        raise AssertionError("no pinned batch in 40 seeds")
    assert tuple(y1.shape) == (4, 32, 4, 4, 4)
    loss = net.training_step(batch, 0)
    got = [float(t.detach()) for t in net.last_losses]
    want, _, _ = R.vicregl_loss(y1, y2, b1.double(), b2.double(), gamma=gamma)
    np.testing.assert_allclose(got, [float(t) for t in want], rtol=2e-4, atol=1e-6)
    np.testing.assert_allclose(float(loss.detach()), sum(got), rtol=1e-6)
    before = {k: p.detach().clone() for k, p in net.named_parameters()}
    StepRunner(net).train_step(batch)
    moved = sum(not torch.equal(before[k], p.detach()) for k, p in net.named_parameters())
    assert moved > 0.8 * len(before)
