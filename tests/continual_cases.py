"""Inputs shared by tools/make_continual_golden.py (which evaluates the reference on them) and the
continual-learning tests (which read tests/golden/continual.npz): everything is generated from names,
nothing is stored twice."""
import os
import zlib

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "continual.npz")

PS = (1, 2, 3, 1.5)
# named tensors of the penalty fixture: 1, 5 and 300 elements
SHAPES = {"scalar.weight": (1,), "vector.bias": (5,), "matrix.weight": (20, 15)}
STATES = ("untouched", "moved", "moved_back")


def draw(tag, shape, scale=1.0):
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    return (scale * rng.standard_normal(shape)).astype(np.float32)


class Named(torch.nn.Module):
    """A module whose ``named_parameters()`` are exactly ``tensors`` (dotted names nest modules)."""

    def __init__(self, tensors, dtype=torch.float32):
        super().__init__()
        for name, value in tensors.items():
            mod, parts = self, name.split(".")
            for part in parts[:-1]:
                if part not in mod._modules:
                    mod.add_module(part, torch.nn.Module())
                mod = mod._modules[part]
            mod.register_parameter(parts[-1], torch.nn.Parameter(torch.as_tensor(value).to(dtype).clone()))


def anchors():
    return {k: draw("anchor:" + k, s) for k, s in SHAPES.items()}


def state(name):
    """The live parameters of a state: the anchors themselves, every tensor moved (fp32 values), or
    moved with one element of every tensor put back exactly onto its anchor."""
    a = anchors()
    if name == "untouched":
        return {k: v.copy() for k, v in a.items()}
    out = {k: (v + draw("move:" + k, v.shape, 0.05)).astype(np.float32) for k, v in a.items()}
    if name == "moved_back":
        for k, v in out.items():
            if v.size > 1:                  # (a 1-element tensor put back would be "untouched")
                v.reshape(-1)[v.size // 2] = a[k].reshape(-1)[v.size // 2]
    return out


# ---- create_param_groups ----------------------------------------------------------------------------
def group_model():
    return torch.nn.Sequential(
        torch.nn.Linear(3, 4), torch.nn.ReLU(),
        torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.LayerNorm(4)), torch.nn.Linear(4, 2))


GROUP_CASES = {
    # exact names (one of them matches nothing), then a substring
    "exact": [["0.weight", "0.bias", "not.there"], "2.1"],
    "substring": ["weight", "3."],
    # "2." and "bias" overlap on 2.0.bias and 2.1.bias; the third group stays empty
    "overlap": ["2.", "bias", ["nothing"]],
}

# ---- EarlyStopper ---------------------------------------------------------------------------------
LOSSES = [1.0, 0.5, 0.75, 0.5, 0.625, 0.25, 0.375, 0.375, 0.5, 0.125, 1.0, 1.0, 1.0]
STOPPERS = {"p1": (1, 0.0), "p2": (2, 0.0), "p3_delta": (3, 0.1875)}
