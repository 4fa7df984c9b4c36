"""What the ensemble tests share: the kernel cases (shapes and seeded fp32 inputs) and the five
fixture networks of tests/golden/ensemble_step_<net>.npz (tools/make_ensemble_golden.py), how either
side builds them, and views of the fixtures.

Every generic ensemble has two ``UNet(depth=[4, 8, 16], encoder_only=True)`` and one
``ResNetBackbone([(4, 8, 3, 1), (8, 16, 3, 1)])`` (swish, batch norm, no dropout),
``n_features=[16, 16, 8]``, ``head_structure=[12, 10]`` and
``head_adn_fn=get_adn_fn(1, "batch", "swish", 0.0)``; the averaging ensemble has three small
``CatNet``s. Inputs are [4, 1, 16, 16] and [4, 1, 16, 16, 8].

The weights are ``oracle.weights.fill_state_dict`` by key, except the buffers of a Gaussian-process
head: ``W`` and ``b`` are seeded draws of their initial distributions (``gp_buffers``),
``scaling_term`` and ``inv_conv`` stay as constructed."""
import os

import numpy as np

from classification_cases import STEP_EPS, STEP_LR, zero_dropout  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- kernel cases ------------------------------------------------------------------------------------
# (N, i, r, o): one row / one feature; non-multiples of 64 lanes and of 256 threads; more waves than
# outputs; more than one 16 x 16 tile of the precision matrix
GP_SHAPES = [(1, 1, 1, 1), (5, 24, 130, 3), (8, 32, 32, 1), (3, 65, 257, 2)]
# i above the fused route's 1024 inputs: functional.gp_route sends it to the composed route
GP_COMPOSED_SHAPE = (4, 1030, 16, 2)
GP_EPS = 1e-5
# name: (n_classes, ordinal, columns of the probabilities; 0: a vector [N])
PRECISION_KINDS = {"binary": (2, False, 0), "binary_col": (2, False, 1), "multi3": (3, False, 3),
                   "ordinal4": (4, True, 3)}
PRECISION_SHAPE = (5, 24, 40, 3)        # r = 40: two and a half tiles (the fixture keeps P in fp64)
PRECISION_M = 0.9           # a momentum that moves the matrix in three batches (the default is 0.999)
SAMPLE_S = (1, 7)
POOL_MEMBERS = [(2, 5, 3, 7), (2, 130, 2, 3, 5), (2, 33)]
AVERAGE_CASES = [(1, 1, 5), (3, 1, 5), (1, 3, 4), (3, 3, 4)]      # (K, C, B)


def gp_scale(r):
    """sqrt(2 / r) as the layer's fp32 ``scaling_term`` holds it."""
    return float(np.sqrt(np.float32(2.0 / r)))


def gp_case(shape, seed=None):
    """fp32 inputs of one Gaussian-process case and the gradients that arrive on its outputs."""
    N, i, r, o = shape
    g = np.random.default_rng(1000 + sum(shape) if seed is None else seed)
    f = np.float32
    return {
        "x": g.normal(size=(N, i)).astype(f) * 1.5 + 0.25,
        "gamma": (1.0 + 0.3 * g.normal(size=(i,))).astype(f),
        "beta": (0.2 * g.normal(size=(i,))).astype(f),
        "W": (g.normal(size=(1, r, i)) * np.sqrt(2.0 / i)).astype(f),
        "b": (g.uniform(size=(1, r)) * 2 * np.pi).astype(f),
        "weights": (g.uniform(-1, 1, size=(o, r)) / np.sqrt(r)).astype(f),
        "dlogits": g.normal(size=(N, o)).astype(f),
        "dphi": (0.5 * g.normal(size=(N, r))).astype(f),
    }


def precision_batches(kind):
    """Three batches (phi [N, r], probabilities) of one precision case: phi from ``gp_case`` inputs
    is the caller's; here the probabilities, fp32."""
    n_classes, ordinal, cols = PRECISION_KINDS[kind]
    N = PRECISION_SHAPE[0]
    g = np.random.default_rng(77 + cols + 10 * int(ordinal))
    out = []
    for _ in range(3):
        z = g.normal(size=(N, max(cols, 1))) * 1.5
        if ordinal or cols <= 1:
            p = 1.0 / (1.0 + np.exp(-z))
        else:
            e = np.exp(z - z.max(1, keepdims=True))
            p = e / e.sum(1, keepdims=True)
        out.append((p[:, 0] if cols == 0 else p).astype(np.float32))
    return out


def sample_eps(S, N, o, seed=5):
    return np.random.default_rng(seed + S).normal(size=(S, N, o)).astype(np.float32)


def pool_member(shape, seed=0):
    return np.random.default_rng(31 + len(shape) + seed).normal(size=shape).astype(np.float32)


def average_case(K, C, B):
    g = np.random.default_rng(K * 10 + C)
    return ([(g.normal(size=(B, C)) * 2).astype(np.float32) for _ in range(K)],
            g.normal(size=(B, C)).astype(np.float32))


# ---- fixture networks --------------------------------------------------------------------------------
NETS = ("gen2d", "gen3d_sae", "gen3d_gp", "gen2d_gp32", "avg3")
GP_NETS = ("gen3d_gp", "gen2d_gp32")
N_FEATURES, HEAD_STRUCTURE = [16, 16, 8], [12, 10]
UNET_DEPTH, RESNET_STRUCTURE = [4, 8, 16], [(4, 8, 3, 1), (8, 16, 3, 1)]
CATNET = dict(spatial_dimensions=3, in_channels=1, n_classes=2,
              resnet_structure=[(4, 8, 3, 1)], maxpool_structure=[(2, 2, 2)])
# name: (spatial dimensions, n_classes, sae, gaussian_process, gp_n_rff, labels, weight decay)
CONFIGS = {
    "gen2d": (2, 2, False, False, None, [0, 1, 1, 0], 0.05),
    "gen3d_sae": (3, 3, True, False, None, [0, 2, 1, 2], 0.05),
    "gen3d_gp": (3, 2, False, True, None, [0, 1, 1, 0], 0.05),
    "gen2d_gp32": (2, 3, False, True, 32, [0, 2, 1, 2], 0.05),
    "avg3": (3, 2, False, False, None, [0, 1, 1, 0], (0.05, 0.1)),
}
FIT_BATCHES = 3
PREDICT_SAMPLES = 7


def input_shape(name):
    return (4, 1, 16, 16) if CONFIGS[name][0] == 2 else (4, 1, 16, 16, 8)


def build_members(name, UNet, ResNetBackbone, CatNet, get_adn_fn, activation_factory):
    """The member networks of ``name`` from one side's classes."""
    sd = CONFIGS[name][0]
    if name == "avg3":
        return [CatNet(adn_fn=get_adn_fn(3, "batch", "swish", 0.0),
                       **{k: (list(v) if isinstance(v, list) else v) for k, v in CATNET.items()})
                for _ in range(3)]
    unets = [UNet(spatial_dimensions=sd, in_channels=1, depth=list(UNET_DEPTH), kernel_sizes=[3, 3, 3],
                  strides=[2, 2, 2], dropout_param=0.0, activation_fn=activation_factory["swish"],
                  encoder_only=True) for _ in range(2)]
    resnet = ResNetBackbone(sd, 1, list(RESNET_STRUCTURE), adn_fn=get_adn_fn(sd, "batch", "swish", 0.0))
    return unets + [resnet]


def ensemble_kwargs(name, members, get_adn_fn):
    """Constructor arguments of the reference's ensemble classes (``gp_n_rff`` is this package's own
    keyword: tools/make_ensemble_golden.py replaces the head instead)."""
    sd, n_classes, sae, gp, _, _, _ = CONFIGS[name]
    if name == "avg3":
        return dict(networks=members, n_classes=n_classes)
    return dict(spatial_dimensions=sd, networks=members, n_features=list(N_FEATURES),
                head_structure=list(HEAD_STRUCTURE), n_classes=n_classes,
                head_adn_fn=get_adn_fn(1, "batch", "swish", 0.0), sae=sae, gaussian_process=gp)


def gp_buffers(i, r):
    """Seeded draws of the layer's initial ``W`` [1, r, i] and ``b`` [1, r]."""
    g = np.random.default_rng(4000 + 7 * i + r)
    return ((g.normal(size=(1, r, i)) * np.sqrt(2.0 / i)).astype(np.float32),
            (g.uniform(size=(1, r)) * 2 * np.pi).astype(np.float32))


def fill(state_dict, gain):
    """The fixture weights of a state dict (see the module docstring)."""
    import torch
    from oracle.weights import fill_state_dict

    out = fill_state_dict(state_dict, gain=gain, norm_weight_offset=1.0)
    for k, v in state_dict.items():
        if k.endswith("gaussian_process_head.W"):
            W, b = gp_buffers(v.shape[2], v.shape[1])
            out[k] = torch.from_numpy(W).to(v.dtype)
            out[k[:-1] + "b"] = torch.from_numpy(b).to(v.dtype)
        elif k.endswith(("gaussian_process_head.scaling_term", "gaussian_process_head.inv_conv")):
            out[k] = v.clone()
    return out


def step_groups(named_parameters, weight_decay):
    """The parameter groups of ``ClassPLABC.configure_optimizers`` as (names, weight decay) and the
    base weight decay, restated on names: the Gaussian-process head's parameters first, without
    decay."""
    names = [n for n, p in named_parameters if p.requires_grad]
    gp = [n for n in names if "gaussian_process_head." in n]
    rest = [n for n in names if n not in gp]
    if isinstance(weight_decay, (list, tuple)):
        wd_body, wd_head = weight_decay
        head = [n for n in rest if "classification" in n]
        body = [n for n in rest if "classification" not in n]
        return [(gp, 0), ([], wd_body / 100), (head, wd_head), (body, wd_body)], wd_body / 100
    wd = float(weight_decay)
    return [(gp, 0), ([], wd / 100), (rest, wd)], wd / 100


def fit_inputs(x, k):
    """Batch ``k`` of the three the precision matrix is fitted on: the step's input, perturbed."""
    g = np.random.default_rng(900 + k)
    return (x + 0.3 * g.normal(size=x.shape)).astype(np.float32)


def predict_eps(N, o):
    return np.random.default_rng(12).normal(size=(2, PREDICT_SAMPLES, N, o)).astype(np.float32)


class StepGold:
    """The records of one network (``files`` and items: what cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, f"ensemble_step_{name}.npz"), allow_pickle=False)
        self.files = list(self._g.files)

    def __getitem__(self, k):
        return self._g[k]


def kernel_gold():
    """The reference's fp64 intermediates of the kernel cases."""
    return np.load(os.path.join(GOLD, "ensemble_kernels.npz"), allow_pickle=False)


def bounds():
    """tests/golden/ensemble_bounds.json: per quantity the reference's own fp32-against-fp64 error
    and the bound the tests use."""
    import json

    with open(os.path.join(GOLD, "ensemble_bounds.json")) as fh:
        return json.load(fh)
