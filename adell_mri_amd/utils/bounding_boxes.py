"""``BBToAdjustedAnchors`` (mirror of adell_mri/utils/monai_transforms/bounding_boxes.py:12-195, without
the MONAI base class): bounding boxes in corner format (x1 y1 z1 x2 y2 z2, input voxels) to the anchor
map ``[1 + 7 A, *output_sh]`` the detection wrapper reads as ``label_key`` -- channel 0 the class, then
per anchor the objectness ("IoU"), three centre adjustments and three log size ratios. fp64, as the
reference. Mirrored as written: the "IoU" is ONE number per box and anchor (the smaller of box and
anchor size per axis, plus ``1 / rel_sh``, over the union of volumes), so it can exceed 1; boxes are the
outer loop and anchors the inner one, the strict ``iou > stored`` lets the first box win a tie, and the
class plane keeps the class of the last successful update; ``shape=`` rescales the boxes only, the
anchors stay as built from ``input_sh``.

``__call__`` is the numpy loop of the reference. ``batch`` is the device entry: padded boxes
``[B, N, 6]``, classes ``[B, N]`` and counts ``[B]`` -> ``[B, 1 + 7 A, *output_sh]`` in one launch of
csrc/detect.hip (one thread per output cell, fp64)."""
from itertools import product
from typing import Iterable

import numpy as np
import torch


class BBToAdjustedAnchors:
    def __init__(self, anchor_sizes, input_sh: Iterable, output_sh: Iterable, iou_thresh: float):
        self.anchor_sizes = [np.array(x) for x in anchor_sizes]
        self.input_sh = input_sh
        self.output_sh = np.array(output_sh)
        self.iou_thresh = iou_thresh
        self.setup_long_anchors()

    def setup_long_anchors(self):
        image_sh = np.array(self.input_sh)
        self.rel_sh = image_sh / self.output_sh
        long_coords = []
        for c in product(*[np.arange(x) for x in self.output_sh]):
            long_coords.append(c)
        self.long_coords = np.array(long_coords)
        rel_anchor_sizes = [x / self.rel_sh for x in self.anchor_sizes]
        self.long_anchors = []
        self.anchor_half = []
        for rel_anchor_size in rel_anchor_sizes:
            # adding 0.5 centres the bounding boxes in each cell
            anchor_h = rel_anchor_size / 2
            self.anchor_half.append(anchor_h)
            long_anchor_rel = [long_coords - anchor_h + 0.5, long_coords + anchor_h + 0.5]
            self.long_anchors.append(np.stack(long_anchor_rel, axis=-1))

    def __call__(self, bb_vertices: Iterable, classes: Iterable, shape: np.ndarray = None) -> np.ndarray:
        bb_vertices = np.array(bb_vertices)
        if len(bb_vertices.shape) < 2:
            bb_vertices = bb_vertices[np.newaxis, :]
        bb_vertices = np.stack([bb_vertices[:, :3], bb_vertices[:, 3:]], axis=-1)
        output = np.zeros([1 + 7 * len(self.long_anchors), *self.output_sh])
        # no vertices present
        if bb_vertices.shape[1] == 0:
            return output
        if shape is None:
            rel_sh = self.rel_sh
        else:
            rel_sh = shape / self.output_sh
        rel_bb_vert = bb_vertices / rel_sh[np.newaxis, :, np.newaxis]
        for i in range(rel_bb_vert.shape[0]):
            rel_bb_size = np.subtract(rel_bb_vert[i, :, 1], rel_bb_vert[i, :, 0])
            center = np.mean(rel_bb_vert[i, :, :], axis=-1)
            bb_vol = np.prod(rel_bb_size + 1 / rel_sh)
            cl = classes[i]
            for anchor_idx, long_anchor in enumerate(self.long_anchors):
                anchor_size = long_anchor[0, :, 1] - long_anchor[0, :, 0]
                rel_bb_size_adj = np.log(rel_bb_size / anchor_size)
                anchor_dim = long_anchor[0, :, 1] - long_anchor[0, :, 0]
                intersects = np.logical_and(
                    np.all(long_anchor[:, :, 1] > rel_bb_vert[i, :, 0], axis=1),
                    np.all(long_anchor[:, :, 0] < rel_bb_vert[i, :, 1], axis=1))
                inter_dim = np.minimum(rel_bb_size, anchor_dim)
                inter_vol = np.prod(inter_dim + 1 / rel_sh, axis=-1)
                anchor_vol = np.prod(anchor_dim, axis=-1)
                union_vol = anchor_vol + bb_vol - inter_vol
                iou = inter_vol / union_vol
                intersection_idx = np.logical_and(iou > self.iou_thresh, intersects)
                box_coords = self.long_coords[intersection_idx]
                center_adjustment = center - (box_coords + 0.5)
                distance_idx = np.all(np.abs(center_adjustment) < 1, axis=1)
                box_coords = box_coords[distance_idx]
                center_adjustment = center_adjustment[distance_idx]
                for j in range(box_coords.shape[0]):
                    idx = tuple([tuple([1 + k + anchor_idx * 7 for k in range(7)]), *box_coords[j]])
                    idx_cl = tuple([0, *box_coords[j]])
                    v = np.array([iou, *center_adjustment[j], *rel_bb_size_adj])
                    if iou > output[idx][0]:
                        output[idx] = v
                        output[idx_cl] = cl
        return output

    def batch(self, boxes: torch.Tensor, classes: torch.Tensor, counts: torch.Tensor,
              shape=None) -> torch.Tensor:
        """The maps of a batch on the device: ``boxes`` [B, N, 6] padded, ``classes`` [B, N],
        ``counts`` [B] boxes per item (0: an all-zero map) -> fp64 [B, 1 + 7 A, *output_sh]."""
        from .. import ops

        if len(self.output_sh) != 3:
            raise NotImplementedError("BBToAdjustedAnchors.batch: 3-D maps only")
        dev = boxes.device
        rel = self.rel_sh if shape is None else np.asarray(shape) / self.output_sh
        half = torch.from_numpy(np.stack(self.anchor_half).astype(np.float64)).to(dev)
        return ops.det_encode(boxes.to(torch.float64).contiguous(),
                              classes.to(torch.float64).contiguous(),
                              counts.to(torch.int32).contiguous(), half, rel, self.iou_thresh,
                              self.output_sh)

    def adjusted_anchors_to_bb_vertices(self, anchor_map: np.ndarray):
        top_left_output = []
        bottom_right_output = []
        for i in range(len(self.anchor_sizes)):
            anchor_size = self.anchor_sizes[i]
            rel_anchor_size = np.array(anchor_size)
            sam = anchor_map[(1 + i * 7):(1 + i * 7 + 7)]
            coords = np.where(sam[0] > 0)
            adj_anchors_long = np.zeros([len(coords[0]), 7])
            for j, coord in enumerate(zip(*coords)):
                center_idxs = tuple([tuple([k for k in range(7)]), *coord])
                v = sam[center_idxs]
                adj_anchors_long[j, :] = v
            correct_centers = np.add(adj_anchors_long[:, 1:4] + 0.5, np.stack(coords, axis=1))
            correct_centers = correct_centers * self.rel_sh
            correct_dims = np.multiply(adj_anchors_long[:, 4:], rel_anchor_size)
            top_left = correct_centers - correct_dims / 2
            bottom_right = correct_centers + correct_dims / 2
            top_left_output.append(top_left)
            bottom_right_output.append(bottom_right)
        return top_left_output, bottom_right_output
