"""Classification losses on the HIP kernels (csrc/classify.hip): the ordinal sigmoidal loss and the
relative order consistency of adell_mri/modules/classification/losses.py:9-129, and the two torch
classes the reference constructs for binary and multi-class networks
(entrypoints/classification/_utils.py:197-224), callable the same way.

Every loss is one launch forward and one backward, sums in a fixed order in fp64, bit-reproducible.
A label outside [0, K) is never used as an index: that item's loss and gradient are NaN (torch
raises; a device kernel cannot without a host synchronisation).
"""
import torch

from ... import functional as HF


class BCEWithLogitsLoss(torch.nn.Module):
    """``torch.nn.BCEWithLogitsLoss(weight)``: the mean over the items; ``weight`` (1 or B elements)
    multiplies the item loss -- torch's ``weight``, not ``pos_weight``, which is what
    ``configure_loss_fn`` passes. One logit per item; soft targets allowed."""

    def __init__(self, weight=None):
        super().__init__()
        self.weight = None if weight is None else torch.as_tensor(weight, dtype=torch.float32)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return HF.bce_with_logits(pred, target, self.weight)


class CrossEntropyLoss(torch.nn.Module):
    """``torch.nn.CrossEntropyLoss(weight)``: sum(w[y] l) / sum(w[y]) over logits [B, K] and int64
    labels [B]."""

    def __init__(self, weight=None):
        super().__init__()
        self.weight = None if weight is None else torch.as_tensor(weight, dtype=torch.float32)

    def forward(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return HF.cross_entropy(pred, target, self.weight)


def ordinal_sigmoidal_loss(pred: torch.Tensor, target: torch.Tensor, n_classes: int,
                           weight: torch.Tensor | None = None) -> torch.Tensor:
    """losses.py:9-62: the [B] vector of CORAL losses of pred [B, K - 1] against int64 labels."""
    return HF.ordinal_sigmoidal_loss(pred, target, n_classes, weight)


def relative_order_consistency(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """losses.py:65-79 on pred [B, 1] (the pre-bias output) and int64 labels [B]."""
    return HF.relative_order_consistency(pred, target)


class OrdinalSigmoidalLoss(torch.nn.Module):
    """losses.py:82-129: ``loss`` [B], or ``(loss, roc_loss)`` when ``pre_bias`` is passed."""

    def __init__(self, n_classes: int, weight: torch.Tensor | None = None):
        super().__init__()
        self.n_classes = n_classes
        self.weight = None if weight is None else torch.as_tensor(weight)

    def forward(self, pred: torch.Tensor, target: torch.Tensor,
                pre_bias: torch.Tensor | None = None):
        loss = ordinal_sigmoidal_loss(pred, target, self.n_classes, self.weight)
        if pre_bias is not None:
            return loss, relative_order_consistency(pre_bias, target)
        return loss


def configure_loss_fn(network_config, net_type, n_classes, class_weights=None):
    """entrypoints/classification/_utils.py:197-224: assigns ``network_config["loss_fn"]`` in place
    -- BCE with logits for two classes, the ordinal loss for ``net_type == "ord"``, else cross
    entropy."""
    if n_classes == 2:
        network_config["loss_fn"] = BCEWithLogitsLoss(class_weights)
    elif net_type == "ord":
        network_config["loss_fn"] = OrdinalSigmoidalLoss(n_classes, class_weights)
    else:
        network_config["loss_fn"] = CrossEntropyLoss(class_weights)
