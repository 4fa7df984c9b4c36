"""Semi-supervised U-Net of the reference (adell_mri/modules/semi_supervised_segmentation): the
U-Net that also returns its decoder features, the losses on them (local contrastive, with anchors,
nearest-neighbour, pseudo-label cross entropy) and the training wrapper that adds the contrastive
loss (weight 0.01) to the supervised step."""
from .losses import (AnatomicalContrastiveLoss, LocalContrastiveLoss,  # noqa: F401
                     LocalContrastiveLossWithAnchors, NearestNeighbourLoss, PseudoLabelCrossEntropy,
                     anchors_from_derangement, derangement, swap)
from .pl import UNetContrastiveSemiSL  # noqa: F401
from .unet import UNetSemiSL  # noqa: F401
