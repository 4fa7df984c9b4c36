"""Whole-batch preprocessing of the classification wrappers (mirror of
adell_mri/utils/batch_preprocessing.py): label smoothing, mixup and partial mixup, and the
``BatchPreprocessing`` object a wrapper calls in ``training_step``.

The numpy draws come in the reference's order -- mixup: ``beta`` (batch size), then ``permutation``;
partial mixup: ``binomial``, ``beta`` (as many as were selected), ``permutation`` -- so a seed gives
the reference's factors and partners. The images go through one HIP launch (csrc/classify.hip:
two rows read, one written, the three operations rounded as torch rounds them); the [B] labels use
plain torch operations.

Deviations: ``partial_mixup`` returns new tensors (the reference assigns into its inputs), and an
item that is its own partner (a fixed point of the permutation) keeps its image as it is, where the
reference computes ``f x + (1 - f) x`` -- equal up to one rounding.
"""
from typing import Tuple

import numpy as np
import torch

from .. import functional as HF


def label_smoothing(y: torch.Tensor, smooth_factor: float) -> torch.Tensor:
    """batch_preprocessing.py:15-27: binary labels moved ``smooth_factor`` towards 0.5's side."""
    return torch.where(y < 0.5, y + smooth_factor, y - smooth_factor)


def _mix_labels(y, factor, partner):
    return y * factor + y[partner] * (1.0 - factor)


def mixup(x: torch.Tensor, y: torch.Tensor, mixup_alpha: float,
          g: np.random.Generator = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """batch_preprocessing.py:30-65: every item mixed with its partner under a permutation, factors
    from Beta(alpha, alpha)."""
    batch_size = y.shape[0]
    if g is None:
        g = np.random.default_rng()
    mixup_factor = torch.as_tensor(g.beta(mixup_alpha, mixup_alpha, batch_size), dtype=x.dtype,
                                   device=x.device)
    mixup_perm = g.permutation(batch_size)
    x = HF.mixup_rows(x.contiguous(), mixup_factor, mixup_perm)
    y = _mix_labels(y, mixup_factor, torch.as_tensor(mixup_perm, device=y.device))
    return x, y


def partial_mixup(x: torch.Tensor, y: torch.Tensor, mixup_alpha: float, mixup_fraction: float = 0.5,
                  g: np.random.Generator = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """batch_preprocessing.py:68-113: mixup of the items a Bernoulli(``mixup_fraction``) draw selects;
    the others are returned as they are (copied: the inputs are not written)."""
    batch_size = y.shape[0]
    if g is None:
        g = np.random.default_rng()
    mxu_i = g.binomial(1, mixup_fraction, batch_size).astype(bool)
    drawn = g.beta(mixup_alpha, mixup_alpha, mxu_i.sum())
    mixup_perm = g.permutation(batch_size)
    factor = np.ones(batch_size)
    factor[mxu_i] = drawn
    partner = np.where(mxu_i, mixup_perm, np.arange(batch_size))
    mixup_factor = torch.as_tensor(factor, dtype=x.dtype, device=x.device)
    x = HF.mixup_rows(x.contiguous(), mixup_factor, partner)
    selected = torch.as_tensor(mxu_i, device=y.device)
    mixed = _mix_labels(y, mixup_factor.to(y.device), torch.as_tensor(partner, device=y.device))
    return x, torch.where(selected, mixed, y)


class BatchPreprocessing:
    """batch_preprocessing.py:116-181. Labels are cast back to their initial dtype after mixup, as
    written: integer labels truncate."""

    def __init__(self, label_smoothing: float = None, mixup_alpha: float = None,
                 partial_mixup: float = None, seed: int = 42):
        self.label_smoothing = label_smoothing
        self.mixup_alpha = mixup_alpha
        self.partial_mixup = partial_mixup
        self.seed = seed
        if self.mixup_alpha is not None:
            self.g = np.random.default_rng(seed)

    def __call__(self, X: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.label_smoothing is not None:
            y = label_smoothing(y, self.label_smoothing)
        if self.mixup_alpha is not None:
            initial_y_dtype = y.dtype
            y = y.float()
            if self.partial_mixup is not None:
                X, y = partial_mixup(X, y, self.mixup_alpha, self.partial_mixup, self.g)
            else:
                X, y = mixup(X, y, self.mixup_alpha, self.g)
            y = y.to(initial_y_dtype)
        return X, y
