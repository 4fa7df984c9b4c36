"""SWIN-UNet configurations outside the small-window attention kernel (more than 64 tokens per
window, or heads wider than 32): constructor arguments shared by tools/make_golden_swin_windows.py,
which generates their fixtures from the reference, and the tests that read them."""

_COMMON = dict(dropout_rate=0.0, mlp_structure=4.0, conv_type="regular", link_type="conv",
               upscale_type="transpose", norm_type="instance", padding="same", dropout_param=0.0,
               activation_fn="leaky_relu", in_channels=2, n_classes=2, depth=[8, 16],
               kernel_sizes=[3, 3])

# name: (constructor kwargs, input shape)
SWIN_WINDOW_CASES = {
    # 216 tokens in 8 windows, heads 32 / 32: resident MFMA kernels, labels + relative bias
    "swinunet3d_t216_a32": (dict(_COMMON, image_size=[24] * 3, patch_size=[2] * 3,
                                 window_size=[12] * 3, shift_sizes=[[0, 2], [0, 2]],
                                 embedding_size=[64, 64], n_heads=2, embed_method="convolutional",
                                 spatial_dimensions=3, strides=[2, 2]),
                            (2, 2, 24, 24, 24)),
    # 16 tokens (the smallest MFMA sequence) but heads 64 and 128 wide
    "swinunet2d_t16_a64": (dict(_COMMON, image_size=[32, 64], patch_size=[2, 2],
                                window_size=[8, 8], shift_sizes=[[0, 1], [0, 1]],
                                embedding_size=[64, 128], n_heads=1, embed_method="linear",
                                spatial_dimensions=2, strides=[[2, 1], 2]),
                           (2, 2, 32, 64)),
    # 125 tokens, heads 24 wide: not MFMA-shaped, the vector-ALU kernels through sliced q / k / v
    "swinunet3d_t125_a24": (dict(_COMMON, image_size=[20] * 3, patch_size=[2] * 3,
                                 window_size=[10] * 3, shift_sizes=[[0, 2], [0, 2]],
                                 embedding_size=[48, 48], n_heads=2, embed_method="linear",
                                 spatial_dimensions=3, strides=[2, 2]),
                            (1, 2, 20, 20, 20)),
}


def load_fixture(name):
    """The arrays of one case as a dict: <name>.npz and every <name>.gradN.npz of tests/golden
    (no committed file of this repository may pass 1 MiB, so the gradients are split into
    several files, whole parameters per file)."""
    import glob
    import os

    import numpy as np

    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = {}
    paths = [os.path.join(gold, name + ".npz")] + sorted(glob.glob(os.path.join(gold, name + ".grad*.npz")))
    assert len(paths) >= 2, paths
    for path in paths:
        with np.load(path) as g:
            out.update({k: g[k] for k in g.files})
    return out


def build_net(name, **over):
    """The package's SWINUNet of one case with the deterministic weights of the fixtures."""
    import copy

    from adell_mri_amd.modules.activations import activation_factory
    from adell_mri_amd.modules.segmentation.unetr import SWINUNet
    from oracle.weights import fill_state_dict

    kw = copy.deepcopy(SWIN_WINDOW_CASES[name][0])
    kw.update(over)
    kw["activation_fn"] = activation_factory[kw["activation_fn"]]
    net = SWINUNet(**kw)
    net.load_state_dict(fill_state_dict(net.state_dict()))
    return net
