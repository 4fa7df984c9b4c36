"""What the batch-ensemble tests and tools/make_batch_ensemble_golden.py share: the layer cases of
tests/golden/batch_ensemble_layers.npz, the two fixture networks of
tests/golden/batch_ensemble_step_<net>.npz, the weights both sides load and the bounds
(tests/golden/batch_ensemble_bounds.json)."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUM_BOUND = 5e-5
# the step tolerances of tests/test_classification_gpu.py
TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6))
STEP_LR, STEP_EPS = 1e-4, 1e-2          # tests/classification_cases.py says why

N = 3                                    # members of every case but "one"
DRAW_SEED = 11                           # np.random.seed directly before a forward that draws
# layer: (class, spatial_dim, in_channels, out_channels, input shape)
LAYERS = {
    "be0": ("BatchEnsemble", 0, 6, 5, (5, 6)),
    "be2": ("BatchEnsemble", 2, 4, 6, (3, 4, 9, 9)),
    "be3": ("BatchEnsemble", 3, 4, 6, (3, 4, 6, 6, 5)),
    "wrap": ("BatchEnsembleWrapper", 0, 6, 5, (5, 6)),
}
# mode: (members, training, idx): "train" draws, "one" is the single-member layer in training,
# "mean" the eval mean; "list" (one member per item, a negative entry) is the wrapper's alone
MODES = {
    "train": (N, True, None),
    "int": (N, True, 2),
    "list": (N, True, [2, 0, -1, 1, 0]),
    "one": (1, True, None),
    "mean": (N, False, None),
}


def layer_cases():
    return [(layer, mode) for layer in LAYERS for mode in MODES
            if mode != "list" or LAYERS[layer][0] == "BatchEnsembleWrapper"]


def _uniform(tag, shape, lo=-1.0, hi=1.0):
    import zlib

    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    return rng.uniform(lo, hi, size=tuple(shape)).astype(np.float32)


def layer_state(layer, n):
    """``mod.weight``, ``mod.bias`` and the member tables of a layer case (fp32)."""
    _, dim, cin, cout, _ = LAYERS[layer]
    wshape = (cout, cin) + (3,) * dim
    scale = 1.0 / np.sqrt(np.prod(wshape[1:]))
    return {"mod.weight": _uniform(layer + ":w", wshape, -2 * scale, 2 * scale),
            "mod.bias": _uniform(layer + ":b", (cout,), -0.5, 0.5),
            "all_weights.pre": _uniform(f"{layer}:{n}:pre", (n, cin), 0.6, 1.4),
            "all_weights.post": _uniform(f"{layer}:{n}:post", (n, cout), 0.6, 1.4)}


def layer_input(layer):
    return _uniform(layer + ":x", LAYERS[layer][4])


def layer_dy(layer, shape):
    return _uniform(layer + ":dy", shape)


# ---- networks ------------------------------------------------------------------------------------------
_RESNET = dict(spatial_dimensions=3, in_channels=1, resnet_structure=[(8, 8, 3, 2), (16, 16, 3, 2)],
               maxpool_structure=[(2, 2, 2), (2, 2, 2)], batch_ensemble=N)
# name: (class, constructor arguments, input shape, labels, weight decay of the step)
NETS = {
    "cat": ("CatNet", dict(_RESNET, n_classes=2), (4, 1, 16, 16, 8), [0, 1, 1, 0], 0.05),
    "ord": ("OrdNet", dict(_RESNET, n_classes=4, classification_structure=[16, 16, 16]),
            (6, 1, 16, 16, 8), [0, 1, 2, 3, 1, 2], 0.05),
}
STEP_SEED = 23                           # np.random.seed directly before the training step
BATCH_IDX = 1                            # the member of the ``batch_idx`` forward (CatNet)


def net_kwargs(name):
    kw = NETS[name][1]
    return {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}


def fill(state_dict, gain):
    """oracle.weights by key; the member tables around 1 (0.7 .. 1.3), where they are initialised."""
    import torch

    from oracle.weights import fill_state_dict, tensor_for

    out = fill_state_dict(state_dict, gain=gain, norm_weight_offset=1.0)
    for k, v in state_dict.items():
        if ".all_weights." in k:
            out[k] = torch.from_numpy(1.0 + tensor_for(k, v.shape, scale=0.3)).to(v.dtype)
    return out


def step_input(name, seed):
    shape = NETS[name][2]
    grids = np.meshgrid(*[np.arange(float(s)) for s in shape[2:]], indexing="ij")
    x = np.stack([np.stack([np.sin((b + 1) * 0.37 * grids[0] + c) * np.cos((b + 2) * 0.23 * grids[1])
                            * np.cos(0.45 * grids[2] + b) for c in range(shape[1])])
                  for b in range(shape[0])])
    return (x + 0.2 * _uniform(f"{name}:{seed}", shape, 0.0, 1.0)).astype(np.float32)


def signature_of(fn):
    """[name, kind, default] per parameter; a class default by its name."""
    import inspect

    out = []
    for p in inspect.signature(fn).parameters.values():
        d = p.default
        d = None if d is inspect.Parameter.empty else (d.__name__ if inspect.isclass(d) else repr(d))
        out.append([p.name, p.kind.name, d])
    return out


def bounds():
    with open(os.path.join(GOLD, "batch_ensemble_bounds.json")) as fh:
        return json.load(fh)


def layer_gold():
    return np.load(os.path.join(GOLD, "batch_ensemble_layers.npz"), allow_pickle=False)


def surface_gold():
    with open(os.path.join(GOLD, "batch_ensemble_surface.json")) as fh:
        return json.load(fh)


class StepGold:
    """The records of one network (``files`` and items: what cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, f"batch_ensemble_step_{name}.npz"), allow_pickle=False)
        self.files = list(self._g.files)

    def __getitem__(self, k):
        return self._g[k]
