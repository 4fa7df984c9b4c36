"""What the spectral-norm tests and tools/make_spectral_norm_golden.py share: the kernel-level cases
(shapes, ``dim``, inputs from a seed) and the two applied networks."""
import os

import numpy as np

_GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = os.path.join(_GOLD_DIR, "spectral_norm.npz")                    # the kernel-level cases
NET_GOLD = {tag: os.path.join(_GOLD_DIR, f"spectral_norm_{tag}.npz") for tag in ("unet", "cat")}
EPS = 1e-12
N_ITERS = (1, 3)
# name: (weight shape, dim). The first eight are the smallest shapes at which a kernel can go wrong
# (h = 1, w = 1, nothing a multiple of 64, more than one block, a transposed-conv weight); the rest
# sit one step below and above every threshold functional.spectral_norm_route names, in both dims:
# block <-> grid at 4 (h w + h + w) + 8 (max(h, w) + 1040) = 158 KiB, i.e. w = 1095 | 1096 for h = 32,
# grid <-> composed at 32768 columns and at 32768 rows.
KERNEL_CASES = {
    "h1": ((1, 1, 3, 3, 3), 0),
    "c8x1": ((8, 1, 3, 3, 3), 0),
    "odd": ((5, 3, 3, 3, 3), 0),
    "w1": ((3, 1), 0),
    "row": ((1, 7), 0),
    "lin": ((130, 300), 0),
    "conv70": ((70, 33, 3, 3, 3), 0),
    "convt": ((16, 8, 2, 2, 2), 1),
    "block_top_d0": ((32, 1095), 0),
    "grid_low_d0": ((32, 1096), 0),
    "block_top_d1": ((5, 32, 219), 1),
    "grid_low_d1": ((8, 32, 137), 1),
    "grid_top_d0": ((2, 32768), 0),
    "composed_low_d0": ((2, 32769), 0),
    "grid_top_d1": ((2, 2, 16384), 1),
    "composed_low_d1": ((3, 2, 10923), 1),
    "grid_top_rows": ((32768, 2), 0),
    "composed_low_rows": ((32769, 2), 0),
}
ROUTES = {"h1": "block", "c8x1": "block", "odd": "block", "w1": "block", "row": "block",
          "lin": "grid", "conv70": "grid", "convt": "block", "block_top_d0": "block",
          "grid_low_d0": "grid", "block_top_d1": "block", "grid_low_d1": "grid", "grid_top_d0": "grid",
          "composed_low_d0": "composed", "grid_top_d1": "grid", "composed_low_d1": "composed",
          "grid_top_rows": "grid", "composed_low_rows": "composed"}
MODES = [("train", n) for n in N_ITERS] + [("eval", 1)]


def matrix_dims(shape, dim):
    """(outer, h, inner): the matrix is [h, outer * inner] with ``dim`` in front."""
    return (int(np.prod(shape[:dim], dtype=np.int64)), int(shape[dim]),
            int(np.prod(shape[dim + 1:], dtype=np.int64)))


def kernel_inputs(name):
    """(W, u0, v0, G) fp32 of a case: normal draws from the case's own seed, u0 and v0 normalised."""
    shape, dim = KERNEL_CASES[name]
    outer, h, inner = matrix_dims(shape, dim)
    rs = np.random.RandomState(1000 + sorted(KERNEL_CASES).index(name))
    W = rs.standard_normal(shape).astype(np.float32)
    G = rs.standard_normal(shape).astype(np.float32)
    u = rs.standard_normal(h)
    v = rs.standard_normal(outer * inner)
    return (W, (u / np.linalg.norm(u)).astype(np.float32), (v / np.linalg.norm(v)).astype(np.float32), G)


def sample_stride(n):
    """Every how many-th element of an array the fixture keeps (all of them up to 1024)."""
    return 1 if n <= 1024 else n // 256


# ---- applied networks ---------------------------------------------------------------------------------------
UNET_KW = dict(spatial_dimensions=3, conv_type="regular", link_type="residual", upscale_type="transpose",
               norm_type="instance", padding=1, dropout_param=0.0, in_channels=2, n_classes=2,
               depth=[4, 16, 32], kernel_sizes=[3, 3, 3], strides=[2, 2, 2])
UNET_INPUT = (2, 2, 16, 16, 16)
UNET_LR, UNET_WD, UNET_GAIN = 1e-3, 5e-3, 1.0
FOCAL = {"gamma": 1.0, "eps": 1e-6}
CAT_NAME, CAT_GAIN = "cat2", 2.0          # tests/classification_cases.py
N_STEPS = 2


def unet_batch():
    rs = np.random.RandomState(77)
    x = rs.rand(*UNET_INPUT).astype(np.float32)
    y = (rs.rand(UNET_INPUT[0], 1, *UNET_INPUT[2:]) > 0.8).astype(np.float32)
    return x, y


def cat_input():
    from classification_cases import CONFIGS

    rs = np.random.RandomState(78)
    return rs.rand(*CONFIGS[CAT_NAME][2]).astype(np.float32)
