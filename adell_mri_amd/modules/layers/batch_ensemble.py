"""Batch-ensemble layers on the HIP kernels (mirror of adell_mri/modules/layers/batch_ensemble.py,
arXiv:2002.06715): one shared body ``mod`` and ``n`` rank-1 members that scale the channels before
(``all_weights.pre`` [n, in_channels]) and after it (``all_weights.post`` [n, out_channels]).

Constructor arguments, attribute names, ``state_dict`` keys and the four forward modes are the
reference's:

* ``idx`` an int: that member for every item (one table row, broadcast inside the kernel);
* ``idx`` a list or tuple of one member per item (the wrapper only);
* training without ``idx``: ``np.random.randint(self.n, size=b)`` from numpy's global generator,
  one draw per layer per forward (the wrapper with ``n == 1`` draws nothing);
* eval without ``idx``: the mean over all members (the wrapper under ``no_grad``, as the reference).

The scales are ``functional.be_scale`` (the drawn members travel as one int32 upload, nothing is
gathered or read back); the eval mean takes one of two routes (``functional.be_route``, or the
``route=`` keyword): "batched" puts chunks of members side by side in one batch
(``be_members_expand``), runs ``mod`` once per chunk and reduces with ``be_members_mean``; "loop"
runs one member at a time and accumulates with ``be_members_mean``. ``spatial_dim=1`` raises
``NotImplementedError``: the package has no 1-D convolution.
"""
from typing import Callable

import numpy as np
import torch

from ... import functional as HF
from .conv import Conv2d, Conv3d
from .linear_blocks import Linear
from .res_blocks import ResidualBlock2d, ResidualBlock3d


def _member_tables(n: int, in_channels: int, out_channels: int) -> torch.nn.ParameterDict:
    """``pre`` then ``post`` from numpy's global generator, in the reference's order."""
    return torch.nn.ParameterDict({
        "pre": torch.nn.Parameter(torch.as_tensor(
            np.random.normal(1, 0.1, size=[n, in_channels]), dtype=torch.float32)),
        "post": torch.nn.Parameter(torch.as_tensor(
            np.random.normal(1, 0.1, size=[n, out_channels]), dtype=torch.float32))})


def _item_bytes(X: torch.Tensor) -> int:
    return X[0].numel() * X.element_size()


def members_mean(X, pre, post, n, mod, route=None):
    """mean over m of ``post[m] * mod(pre[m] * X)`` on the route asked for (None: ``be_route``)."""
    if route is None:
        route = HF.be_route(n, X.shape[0], _item_bytes(X), mod)
    if route not in HF.BE_ROUTES:
        raise ValueError(f"route must be one of {HF.BE_ROUTES}, got {route!r}")
    step = HF.be_chunk(n, X.shape[0], _item_bytes(X)) if route == "batched" else 1
    acc = None
    for m0 in range(0, n, step):
        m1 = min(n, m0 + step)
        acc = HF.be_members_mean(mod(HF.be_members_expand(X, pre, m0, m1)), post, m0, m1, n, acc)
    return acc


class BatchEnsemble(torch.nn.Module):
    """batch_ensemble.py:14-147: builds its own body, a ``Linear`` (``spatial_dim=0``), ``Conv2d`` /
    ``Conv3d`` or, with ``res_blocks=True``, a ``ResidualBlock2d`` / ``ResidualBlock3d``, from
    ``op_kwargs`` (default ``{"kernel_size": 3}``: no padding, as written). The eval mean is
    differentiable."""

    def __init__(self, spatial_dim: int, n: int, in_channels: int, out_channels: int,
                 adn_fn: Callable = torch.nn.Identity, op_kwargs: dict = None,
                 res_blocks: bool = False):
        super().__init__()
        self.spatial_dim = spatial_dim
        self.n = n
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.adn_fn = adn_fn
        self.op_kwargs = op_kwargs
        self.res_blocks = res_blocks

        self.correct_kwargs()
        self.initialize_layers()

    def correct_kwargs(self):
        if self.op_kwargs is None:
            self.op_kwargs = {} if self.spatial_dim == 0 else {"kernel_size": 3}

    def initialize_layers(self):
        if self.spatial_dim == 1:
            raise NotImplementedError("spatial_dim=1: the package has no 1-D convolution")
        if self.res_blocks is False:
            op = {0: Linear, 2: Conv2d, 3: Conv3d}[self.spatial_dim]
            self.mod = op(self.in_channels, self.out_channels, **self.op_kwargs)
        else:
            op = {2: ResidualBlock2d, 3: ResidualBlock3d}[self.spatial_dim]
            self.mod = op(in_channels=self.in_channels, out_channels=self.out_channels,
                          **self.op_kwargs)
        self.all_weights = _member_tables(self.n, self.in_channels, self.out_channels)
        self.adn_op = self.adn_fn(self.out_channels)

    def forward(self, X: torch.Tensor, idx: int = None, route: str = None):
        pre, post = self.all_weights["pre"], self.all_weights["post"]
        if idx is not None:
            # one row of each table (a view of the parameter), broadcast inside the kernel
            X = HF.be_scale(self.mod(HF.be_scale(X, pre[idx][None])), post[idx][None])
        elif self.training is True:
            idxs = HF.be_indices(np.random.randint(self.n, size=X.shape[0]), self.n, X.shape[0],
                                 X.device)
            X = HF.be_scale(self.mod(HF.be_scale(X, pre, idxs)), post, idxs)
        else:
            X = members_mean(X, pre, post, self.n, self.mod, route)
        return self.adn_op(X)


class BatchEnsembleWrapper(torch.nn.Module):
    """batch_ensemble.py:150-255: the member scales around a given module -- ``mod`` of the
    constructor or the one handed to ``forward`` (``ResNetBackbone`` hands each stage)."""

    def __init__(self, mod: torch.nn.Module, n: int, in_channels: int, out_channels: int,
                 adn_fn: Callable = torch.nn.Identity):
        super().__init__()
        self.mod = mod
        self.n = n
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.adn_fn = adn_fn

        self.initialize_layers()

    def initialize_layers(self):
        self.all_weights = _member_tables(self.n, self.in_channels, self.out_channels)
        self.adn_op = self.adn_fn(self.out_channels)

    def forward(self, X: torch.Tensor, idx: int = None, mod: torch.nn.Module = None, *args,
                route: str = None, **kwargs):
        if mod is None:
            mod = self.mod
        b = X.shape[0]
        pre, post = self.all_weights["pre"], self.all_weights["post"]
        if idx is not None:
            if isinstance(idx, int):
                X = HF.be_scale(mod(HF.be_scale(X, pre[idx][None]), *args, **kwargs),
                                post[idx][None])
            elif isinstance(idx, (list, tuple)):
                idxs = HF.be_indices(idx, self.n, b, X.device)
                X = HF.be_scale(mod(HF.be_scale(X, pre, idxs), *args, **kwargs), post, idxs)
            else:
                raise NotImplementedError("idx has to be int, list or tuple")
        elif self.training is True:
            # n == 1: member 0 for every item and nothing drawn
            idxs = (None if self.n == 1 else
                    HF.be_indices(np.random.randint(self.n, size=b), self.n, b, X.device))
            X = HF.be_scale(mod(HF.be_scale(X, pre, idxs), *args, **kwargs), post, idxs)
        else:
            with torch.no_grad():
                X = members_mean(X, pre, post, self.n, mod, route)
        return self.adn_op(X)
