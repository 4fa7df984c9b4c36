"""Adaptive prediction sets (mirror of adell_mri/modules/conformal_prediction/conformal.py):
``AdaptivePredictionSets(alpha)`` with ``update`` / ``calculate`` / ``reset`` / ``forward`` and
``qhat`` as a non-trainable ``Parameter``.

On the GPU the cumulative probabilities come from one launch (``functional.aps_cumulative``, rows of at
most 64 classes): ``calculate`` reads each row's score from the kernel, no ``[N, C]`` gather. CPU
tensors and wider rows take the same rule in torch ops, so the class works without a GPU.

The rule, where the reference leaves it to ``argsort`` and ``cumsum``: the order is the stable
descending one (of equal probabilities the lower index first) and every prefix is an fp64 sum rounded
to fp32, the reference's CPU arithmetic. ``qhat = sorted(scores)[ceil(level (n - 1))]`` with ``level =
ceil((n + 1)(1 - alpha)) / n``, what ``torch.quantile(..., interpolation="higher")`` returns; a
``level > 1`` (too few calibration rows for ``alpha``) raises ``ValueError`` where the reference fails
inside ``torch.quantile``. A NaN score makes ``qhat`` NaN, as there.
"""
from math import ceil

import torch

from ... import functional as HF


class AdaptivePredictionSets(torch.nn.Module):
    def __init__(self, alpha: float):
        super().__init__()
        self.alpha = alpha

        self.y = []
        self.pred = []

    def update(self, y: torch.Tensor, pred: torch.Tensor):
        self.y.append(y)
        self.pred.append(pred)

    def calculate(self):
        y = torch.concatenate(self.y, 0)
        pred = torch.concatenate(self.pred, 0)
        n = y.shape[0]
        level = ceil((n + 1) * (1 - self.alpha)) / n if n > 0 else float("inf")
        if level > 1:
            raise ValueError(
                f"AdaptivePredictionSets: n = {n} calibration rows are too few for alpha = "
                f"{self.alpha}: the quantile level ceil((n + 1)(1 - alpha)) / n = {level} exceeds 1")
        scores = HF.aps_scores(pred, y)
        ordered = torch.sort(scores).values
        qhat = ordered[ceil(level * (n - 1))]
        qhat = torch.where(torch.isnan(scores).any(), torch.full_like(qhat, float("nan")), qhat)
        self.qhat = torch.nn.Parameter(qhat, requires_grad=False)

    def reset(self):
        self.y = []
        self.pred = []

    def forward(self, pred: torch.Tensor, logits: bool = False):
        if logits is True:
            pred = torch.softmax(pred, -1)
        pred_sets = HF.aps_sets(pred, self.qhat)
        return torch.concatenate([pred_sets.float(), pred], 1)
