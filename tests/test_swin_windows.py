"""SWIN attention beyond the small-window kernel (more than 64 tokens per window, heads wider than
32), host side: the shift mask as region labels, the routing of MultiHeadSelfAttention, and the
construction of the three nets of tests/swin_window_cases.py against their reference fixtures."""
import numpy as np
import pytest
import torch

from adell_mri_amd.modules.layers.linear_blocks import attention_route
from adell_mri_amd.modules.layers.vit import (SWINTransformerBlock, generate_mask,
                                              shift_region_labels)
from swin_window_cases import SWIN_WINDOW_CASES, build_net, load_fixture


@pytest.mark.parametrize("image,window,shift", [
    ([12, 12, 12], [6, 6, 6], 2),
    ([16, 32], [4, 4], 1),
    ([12, 8, 8], [6, 4, 2], [2, 0, 1]),       # a per-axis shift list, one axis unshifted
], ids=["3d", "2d", "per_axis"])
def test_labels_reproduce_the_mask(image, window, shift):
    lab = shift_region_labels(image, window, shift)
    n_win = int(np.prod([i // w for i, w in zip(image, window)]))
    assert lab.dtype == torch.int32 and lab.shape == (n_win, int(np.prod(window)))
    assert lab.is_contiguous()
    mask = generate_mask(image, window, shift)
    want = torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0)
    assert mask.dtype == torch.float32 and torch.equal(mask, want)
    assert float(mask.min()) == -100.0            # the shift does mask something


def test_no_shift_no_labels():
    assert shift_region_labels([12, 12, 12], [6, 6, 6], 0) is None
    assert shift_region_labels([16, 32], [4, 4], [0, 0]) is None
    assert generate_mask([16, 32], [4, 4], 0) is None


@pytest.mark.parametrize("shape,route", [
    ((8, 4, 4), "window"), ((64, 32, 32), "window"), ((65, 32, 32), "seq"),
    ((216, 32, 32), "seq"), ((16, 64, 64), "seq"), ((16, 128, 128), "seq"),
    ((125, 24, 24), "general"), ((8, 64, 64), "general"),
])
def test_routing(shape, route):
    assert attention_route(*shape) == route


@pytest.mark.parametrize("name", list(SWIN_WINDOW_CASES))
def test_nets_build_with_the_reference_parameters(name):
    g = load_fixture(name)
    net = build_net(name)
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in g["param_keys"]]
    shapes = {str(k): tuple(int(i) for i in str(s).split(",")) for k, s in
              zip(g["param_keys"], g["param_shapes"])}
    for k, p in net.named_parameters():
        assert tuple(p.shape) == shapes[k], k
    tables = [k for k in shapes if k.endswith("relative_position_bias_table")]
    assert len(tables) == 4 and all("grad64:" + k in g for k in tables)
    assert tuple(g["x"].shape) == SWIN_WINDOW_CASES[name][1]


def test_block_with_512_token_windows_holds_no_dense_mask():
    blk = SWINTransformerBlock(image_size=[16, 16, 8], patch_size=[1, 1, 1], window_size=[8, 8, 8],
                               in_channels=2, embedding_size=64, shift_size=2, n_heads=2)
    assert blk.attention_mask is None
    assert blk.attention_labels.shape == (4, 512) and blk.attention_labels.dtype == torch.int32
    big = [n for n, t in list(blk.named_buffers()) + list(vars(blk).items())
           if torch.is_tensor(t) and t.numel() >= 4 * 512 * 512]
    assert not big, big
    # inside the small-window box the dense mask is what the window kernel reads: still built
    small = SWINTransformerBlock(image_size=[16, 16, 8], patch_size=[4, 4, 4], window_size=[8, 8, 8],
                                 in_channels=2, embedding_size=16, shift_size=1, n_heads=4)
    assert small.attention_mask.shape == (4, 8, 8)
    assert torch.equal(small.attention_mask, generate_mask([4, 4, 2], [2, 2, 2], 1))


def test_route_needs_affine_qk_norms_for_the_in_place_form():
    assert attention_route(216, 32, 32, qk_affine=False) == "general"
    assert attention_route(8, 4, 4, qk_affine=False) == "window"


def test_window_kernel_refuses_labels_and_large_windows_refuse_odd_masks():
    """Both refusals come before any kernel runs."""
    from adell_mri_amd.modules.layers.linear_blocks import MultiHeadSelfAttention

    small = MultiHeadSelfAttention(16, 16, 16, 16, n_heads=4, window_size=[2, 2, 2])
    lab = torch.zeros(4, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="dense mask"):
        small(torch.zeros(1, 4, 8, 16), mask_labels=lab)
    big = MultiHeadSelfAttention(64, 64, 64, 64, n_heads=2, window_size=[6, 6, 6])
    x = torch.zeros(1, 8, 216, 64)
    for shape in ((8, 3, 216, 216), (8, 216, 215)):
        with pytest.raises(ValueError, match="windowed attention mask"):
            big(x, mask=torch.zeros(shape))
