"""``complete_iou_loss`` (mirror of adell_mri/modules/object_detection/losses.py:7-83): IoU, centre
distance over enclosing-box diagonal, and the aspect-ratio term averaged over the dimension pairs,
for boxes ``[n, 2 ndim]`` whose sizes carry ``+ 1``. ``alpha = v / ((1 - iou) + v)`` is not detached.
This is the composite in plain torch ops; handed to ``YOLONet3dPL`` as ``reg_loss_fn`` (by identity)
it selects the fused step loss of csrc/detect.hip on the GPU, which computes the same three terms."""
from itertools import combinations
from typing import Tuple

import torch


def complete_iou_terms(a: torch.Tensor, b: torch.Tensor, a_center: torch.Tensor = None,
                       b_center: torch.Tensor = None,
                       ndim: int = 3) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(iou, cpd, ar) in the dtype of the boxes: ``complete_iou_loss`` in front of its closing
    ``iou.float()`` (what an fp64 oracle calls)."""
    a_tl, b_tl = a[:, :ndim], b[:, :ndim]
    a_br, b_br = a[:, ndim:], b[:, ndim:]
    inter_tl = torch.maximum(a_tl, b_tl)
    inter_br = torch.minimum(a_br, b_br)
    a_size = a_br - a_tl + 1
    b_size = b_br - b_tl + 1
    inter_size = inter_br - inter_tl + 1
    if a_center is None:
        a_center = (a_tl + a_br) / 2
    if b_center is None:
        b_center = (b_tl + b_br) / 2
    diag_tl = torch.minimum(a_tl, b_tl)
    diag_br = torch.maximum(a_br, b_br)
    inter_area = torch.prod(inter_size, axis=-1)
    union_area = torch.subtract(torch.prod(a_size, axis=-1) + torch.prod(b_size, axis=-1), inter_area)
    iou = torch.where(union_area > 0.0, inter_area / union_area, torch.zeros_like(union_area))
    center_distance = torch.square(a_center - b_center).sum(-1)
    bb_distance = torch.square(diag_br - diag_tl).sum(-1)
    cpd_component = center_distance / bb_distance
    pis = torch.pi ** 2
    ar_list = []
    for i, j in combinations(range(ndim), 2):
        ar_list.append(4 / pis * (torch.subtract(torch.arctan(a_size[:, i] / a_size[:, j]),
                                                 torch.arctan(b_size[:, i] / b_size[:, j]))) ** 2)
    v = sum(ar_list) / len(ar_list)
    alpha = v / ((1 - iou) + v)
    ar_component = v * alpha
    return iou, cpd_component, ar_component


def complete_iou_loss(a: torch.Tensor, b: torch.Tensor, a_center: torch.Tensor = None,
                      b_center: torch.Tensor = None,
                      ndim: int = 3) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    iou, cpd_component, ar_component = complete_iou_terms(a, b, a_center, b_center, ndim)
    return iou.float(), cpd_component, ar_component
