"""VICRegL without a GPU: ``ssl_method="vicregl"`` constructs where the reference's factory builds
it, the plain-torch restatement (tests/vicregl_ref.py, the GPU tests' reference beyond the fixture)
reproduces the fixture of the real reference (tools/make_vicregl_golden.py), and the argument
checks raise."""
import os

import numpy as np
import pytest
import torch

import vicregl_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["a3d", "b2d", "c3d"]
BACKBONE = dict(spatial_dim=2, in_channels=1, structure=[[8, 8, 3, 2]], maxpool_structure=[[2, 2]],
                res_type="resnet", adn_fn=torch.nn.Identity)
HEADS = dict(projection_head_args=dict(in_channels=8, structure=[16, 8], adn_fn=torch.nn.Identity),
             prediction_head_args=dict(in_channels=8, structure=[16, 8], adn_fn=torch.nn.Identity))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "vicregl_loss.npz"), allow_pickle=False)


def test_vicregl_constructs_where_the_reference_builds_it():
    from adell_mri_amd.modules.self_supervised.losses import VICRegLocalLoss, VICRegLoss
    from adell_mri_amd.modules.self_supervised.pl import SelfSLResNetPL, SelfSLUNetPL
    from adell_mri_amd.utils.network_factories import get_ssl_network

    net = SelfSLResNetPL(ssl_method="vicregl", vic_reg_loss_params={"gamma": 7},
                         backbone_args=dict(BACKBONE), **{k: dict(v) for k, v in HEADS.items()})
    assert isinstance(net.loss, VICRegLocalLoss) and isinstance(net.loss, VICRegLoss)
    assert net.loss.gamma == 7 and net.loss.alpha == 0.9
    assert net._heads_for_method({"box_1": 1, "box_2": 2}) == ("representation", "representation",
                                                               [1, 2])
    assert net._views_share_a_pass("representation", "representation") is False
    cfg = {"backbone_args": dict(BACKBONE), **{k: dict(v) for k, v in HEADS.items()},
           "vic_reg_loss_params": {"gamma": 3, "lam": 10.0}}
    made = get_ssl_network(None, 10, 100, 0, "vicregl", None, "resnet", cfg, False)
    assert type(made).__name__ == "SelfSLResNetPL" and isinstance(made.loss, VICRegLocalLoss)
    assert (made.loss.gamma, made.loss.lam, made.stop_gradient) == (3, 10.0, False)
    unet = SelfSLUNetPL(ssl_method="vicregl", vic_reg_loss_params={"gamma": 4},
                        spatial_dimensions=3, depth=[4, 8], kernel_sizes=[3, 3], strides=[2, 2],
                        padding=1, in_channels=1)
    assert isinstance(unet.loss, VICRegLocalLoss) and unet.loss.gamma == 4


def test_convnext_wrapper_still_raises():
    from adell_mri_amd.modules.self_supervised.pl import SelfSLConvNeXtPL

    with pytest.raises(NotImplementedError):
        SelfSLConvNeXtPL(ssl_method="vicregl",
                         backbone_args=dict(spatial_dim=3, in_channels=1, structure=[[8, 16, 3, 2]],
                                            maxpool_structure=[2]),
                         projection_head_args=dict(in_channels=8, structure=[16, 8]),
                         prediction_head_args=dict(in_channels=8, structure=[16, 8]))


def test_argument_checks_raise_value_errors():
    from adell_mri_amd.modules.self_supervised.losses import VICRegLocalLoss

    with pytest.raises(ValueError):
        VICRegLocalLoss(gamma=65)
    with pytest.raises(ValueError):
        VICRegLocalLoss(gamma=0)
    loss = VICRegLocalLoss(gamma=10)
    box = torch.tensor([[0.0, 0.0, 8.0, 8.0]] * 2)
    with pytest.raises(ValueError):      # differing view shapes (the reference mis-indexes view 2)
        loss(torch.zeros((2, 4, 4, 4)), torch.zeros((2, 4, 4, 3)), box, box)
    with pytest.raises(ValueError):      # gamma beyond the T * T pairs
        loss(torch.zeros((2, 4, 1, 3)), torch.zeros((2, 4, 1, 3)), box, box)


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_fixture(gold, name):
    g = gold
    gamma = int(g[f"{name}:gamma"])
    for tag in ("loc12", "loc21", "feat12", "feat21"):      # the fixture's own condition
        assert (g[f"{name}:gap_{tag}"] >= 1e-4).all(), (tag, g[f"{name}:gap_{tag}"])
    x1 = torch.from_numpy(g[f"{name}:x1"]).double().requires_grad_(True)
    x2 = torch.from_numpy(g[f"{name}:x2"]).double().requires_grad_(True)
    b1, b2 = torch.from_numpy(g[f"{name}:box1"]).double(), torch.from_numpy(g[f"{name}:box2"]).double()
    terms, ploc, pfeat = R.vicregl_loss(x1, x2, b1, b2, gamma=gamma)
    np.testing.assert_allclose(torch.stack(terms).detach().numpy(), g[f"{name}:terms"], rtol=1e-9)
    # rows for direction (X1, X2), columns -- the rows of the transposed matrix -- for (X2, X1)
    for kind, pairs in (("loc", ploc), ("feat", pfeat)):
        for tag, col in ((f"{kind}12", 0), (f"{kind}21", 1)):
            got = np.sort(pairs[..., col].numpy(), 1)
            assert np.array_equal(got, g[f"{name}:rows_{tag}"]), tag
    sum(terms).backward()
    np.testing.assert_allclose(x1.grad.numpy(), g[f"{name}:dx1"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(x2.grad.numpy(), g[f"{name}:dx2"], rtol=1e-5, atol=1e-9)
    # ... and in fp32, the reference's own fp32 run
    t32, _, _ = R.vicregl_loss(x1.detach().float(), x2.detach().float(), b1.float(), b2.float(),
                               gamma=gamma)
    np.testing.assert_allclose(torch.stack(t32).numpy(), g[f"{name}:terms_fp32"], rtol=2e-5)


def test_restatement_tie_order_is_distance_then_flat_index():
    d2 = torch.tensor([[[1.0, 5.0, 5.0], [5.0, 0.0, 2.0], [5.0, 5.0, 3.0]]])
    assert R.top_pairs(d2, 4)[0].tolist() == [[0, 1], [0, 2], [1, 0], [2, 0]]
    a = torch.tensor([[[0.0, 0.0], [3.0, 4.0], [3.0, 4.0]]])
    got = R.top_pairs(R.sq_dists(a, a), 4)[0].tolist()
    assert got == [[0, 1], [0, 2], [1, 0], [2, 0]]
