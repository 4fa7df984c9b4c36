"""``YOLONet3d`` (mirror of adell_mri/modules/object_detection/nets.py:20-320): a ResNet backbone with
``maxpool_structure``, ADN -> atrous spatial pyramid -> ADN -> concurrent squeeze-and-excite -> ADN, and
four 1x1x1 heads: centre (tanh), size, objectness (sigmoid) and class (sigmoid for two classes, channel
softmax otherwise). Same constructor, attribute names and ``state_dict`` keys (``anchor_tensor`` first,
a frozen Parameter; ``classifiation_layer`` sic). Convolutions, ADN sites, pooling and the closing
activations are the HIP leaves; a head's ``torch.nn.Tanh`` / ``Sigmoid`` / ``Softmax`` module stays in
its ``Sequential`` for the key layout and is run as the fused activation kernel.

``recover_boxes`` / ``recover_boxes_batch`` keep the reference's behaviour, quirks included: without
NMS, more than 1000 candidates keep the INDICES below 1000 of the ascending score order (not the
thousand best); for ``n_classes == 2`` the "classes" are the objectness values; ``nms=True`` calls
``nms_nd(..., 0.7, 0.5)``, which as written suppresses nothing -- set ``self.nms_suppress = True`` for
the greedy suppression (``utils.nms_nd(suppress=True)``). ``recover_boxes_batch`` also takes the heads
as ``forward`` returns them (5-D, anchors still in the channels): on the GPU the candidates are then
tabulated and decoded in place by csrc/detect.hip (``functional.detection_decode``).

``backbone_str="convnext"`` (``ConvNeXtBackboneDetection``) is not built and ``CoarseDetector3d`` has no
behaviour to mirror (see its class text): both raise ``NotImplementedError``."""
from typing import List, Tuple

import numpy as np
import torch

from ... import functional as HF
from ..layers.adn_fn import ActDropNorm
from ..layers.conv import Conv3d
from ..layers.multi_resolution import AtrousSpatialPyramidPooling3d
from ..layers.res_net import ResNetBackbone
from ..layers.self_attention import ConcurrentSqueezeAndExcite3d
from .utils import maxpool_default, nms_nd, pyramid_default, resnet_default


def _head(seq, X):
    """A head's Sequential with its closing activation module run as the HIP kernel."""
    mods = list(seq)
    last = mods[-1]
    if isinstance(last, (torch.nn.Tanh, torch.nn.Sigmoid, torch.nn.Softmax)):
        mods = mods[:-1]
    for m in mods:
        X = m(X)
    if isinstance(last, torch.nn.Tanh):
        return HF.norm_drop_act(X, act="tanh")
    if isinstance(last, torch.nn.Sigmoid):
        return HF.norm_drop_act(X, act="sigmoid")
    if isinstance(last, torch.nn.Softmax):
        return HF.channel_softmax(X)
    return X


class YOLONet3d(torch.nn.Module):
    def __init__(self, backbone_str: str = "resnet", in_channels: int = 1, n_classes: int = 2,
                 anchor_sizes: List = np.ones([1, 6]), dev: str = "cuda",
                 resnet_structure: List[Tuple[int, int, int, int]] = resnet_default,
                 maxpool_structure: List[Tuple[int, int, int]] = maxpool_default,
                 pyramid_layers: List[Tuple[int, int, int]] = pyramid_default,
                 adn_fn: torch.nn.Module = lambda s: ActDropNorm(s, norm_fn=torch.nn.BatchNorm3d)):
        super().__init__()
        self.backbone_str = backbone_str
        self.in_channels = in_channels
        self.n_classes = n_classes
        self.anchor_sizes = anchor_sizes
        self.resnet_structure = resnet_structure
        self.maxpool_structure = maxpool_structure
        self.pyramid_layers = pyramid_layers
        self.adn_fn = adn_fn
        self.n_b = len(self.anchor_sizes)
        self.dev = dev

        self.init_anchor_tensors()
        self.init_layers()

    def init_anchor_tensors(self):
        self.anchor_tensor = [torch.reshape(torch.as_tensor(anchor_size), [3, 1, 1, 1])
                              for anchor_size in self.anchor_sizes]
        self.anchor_tensor = torch.cat(self.anchor_tensor, dim=0).to(self.dev)
        self.anchor_tensor = torch.nn.Parameter(self.anchor_tensor, requires_grad=False)

    def init_layers(self):
        if self.backbone_str == "resnet":
            self.res_net = ResNetBackbone(3, self.in_channels, self.resnet_structure,
                                          adn_fn=self.adn_fn,
                                          maxpool_structure=self.maxpool_structure)
        elif self.backbone_str == "convnext":
            raise NotImplementedError("YOLONet3d: backbone_str='convnext' (ConvNeXtBackboneDetection) "
                                      "is not built; 'resnet' is")
        self.feature_extraction = self.res_net
        last_size = self.resnet_structure[-1][0]

        pyramid = [self.adn_fn(last_size)]
        if self.pyramid_layers is not None and len(self.pyramid_layers) > 0:
            pyramid.extend([
                AtrousSpatialPyramidPooling3d(last_size, last_size, self.pyramid_layers,
                                              adn_fn=torch.nn.Identity),
                self.adn_fn(last_size)])
        pyramid.extend([ConcurrentSqueezeAndExcite3d(last_size), self.adn_fn(last_size)])
        self.pyramidal_feature_extraction = torch.nn.Sequential(*pyramid)

        self.bb_size_layer = torch.nn.Sequential(
            Conv3d(last_size, last_size, 1), self.adn_fn(last_size),
            Conv3d(last_size, self.n_b * 3, 1))
        self.bb_center_layer = torch.nn.Sequential(
            Conv3d(last_size, last_size, 1), self.adn_fn(last_size),
            Conv3d(last_size, self.n_b * 3, 1), torch.nn.Tanh())
        self.bb_objectness_layer = torch.nn.Sequential(
            Conv3d(last_size, last_size, 1), self.adn_fn(last_size),
            Conv3d(last_size, self.n_b, 1), torch.nn.Sigmoid())
        if self.n_classes == 2:
            self.classifiation_layer = torch.nn.Sequential(
                Conv3d(last_size, last_size, 1), self.adn_fn(last_size),
                Conv3d(last_size, 1, 1), torch.nn.Sigmoid())
        else:
            self.classifiation_layer = torch.nn.Sequential(
                Conv3d(last_size, last_size, 1), self.adn_fn(last_size),
                Conv3d(last_size, self.n_classes, 1), torch.nn.Softmax(dim=1))

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        features = self.feature_extraction(X)
        features = self.pyramidal_feature_extraction(features)
        bb_size_pred = _head(self.bb_size_layer, features)
        bb_center_pred = _head(self.bb_center_layer, features)
        bb_object_pred = _head(self.bb_objectness_layer, features)
        class_pred = _head(self.classifiation_layer, features)
        return bb_center_pred, bb_size_pred, bb_object_pred, class_pred

    def split(self, x, n_splits, dim):
        size = int(x.shape[dim] // n_splits)
        return torch.split(x, size, dim)

    def channels_to_anchors(self, prediction):
        prediction[:-1] = [torch.stack(self.split(x, self.n_b, 1), -1) for x in prediction[:-1]]
        return prediction

    def _tail(self, long_bb, object_scores, long_classes, nms):
        """The end of ``recover_boxes``: NMS, or the "top 1000" branch as written."""
        if nms is True:
            bb_idxs = nms_nd(long_bb, object_scores.reshape(-1), 0.7, 0.5,
                             suppress=getattr(self, "nms_suppress", False))
            return long_bb[bb_idxs], object_scores[bb_idxs], long_classes[bb_idxs]
        if len(object_scores.shape) > 0:
            if object_scores.shape[0] > 1000:
                top_1000 = torch.argsort(object_scores)
                top_1000 = top_1000[top_1000 < 1000]
                return long_bb[top_1000], object_scores[top_1000], long_classes[top_1000]
        return long_bb, object_scores, long_classes

    def recover_boxes(self, bb_center_pred: torch.Tensor, bb_size_pred: torch.Tensor,
                      bb_object_pred: torch.Tensor, class_pred: torch.Tensor, nms: bool = False,
                      correction_factor: torch.Tensor = None) -> torch.Tensor:
        """One image, anchors stacked last ([3, H, W, D, A], [3, ...], [1, ...], [C, H, W, D]) ->
        (boxes [n, 6] as (upper corner, lower corner), objectness scores [n], classes): the composite
        in torch ops, as the reference writes it."""
        c, h, w, d, a = bb_center_pred.shape
        dev = bb_center_pred.device
        mesh = torch.stack(torch.meshgrid([torch.arange(h), torch.arange(w), torch.arange(d)],
                                          indexing="ij")).to(dev)
        mesh = torch.stack([mesh for _ in self.anchor_sizes], -1)
        anc = torch.stack(torch.split(self.anchor_tensor, 3, 0), -1)
        bb_size_pred = anc * torch.exp(bb_size_pred)
        bb_center_pred = bb_center_pred + mesh
        c, x, y, z, a = torch.where(bb_object_pred > 0.5)
        object_scores = bb_object_pred[:, x, y, z, a].swapaxes(0, 1)
        long_sizes = bb_size_pred[:, x, y, z, a].swapaxes(0, 1)
        long_centers = bb_center_pred[:, x, y, z, a].swapaxes(0, 1)
        if correction_factor is not None:
            long_centers = long_centers * correction_factor.unsqueeze(0)
        if self.n_classes > 2:
            long_classes = class_pred[:, x, y, z].swapaxes(0, -1)
        else:
            long_classes = bb_object_pred[:, x, y, z, a].swapaxes(0, 1)
        long_classes = long_classes.squeeze()
        object_scores = object_scores.squeeze(1)
        upper_corner = long_centers - long_sizes / 2
        lower_corner = long_centers + long_sizes / 2
        long_bb = torch.cat([upper_corner, lower_corner], 1)
        return self._tail(long_bb, object_scores, long_classes, nms)

    def recover_boxes_batch(self, bb_size_pred: torch.Tensor, bb_center_pred: torch.Tensor,
                            bb_object_pred: torch.Tensor, class_pred: torch.Tensor, nms: bool = False,
                            correction_factor: torch.Tensor = None,
                            to_dict: bool = False) -> List[torch.Tensor]:
        """``recover_boxes`` per item. The first two arguments carry the reference's swapped names
        and are handed on positionally, so callers pass (centre, size, objectness, class) as
        ``forward`` returns them. 5-D heads on the GPU take the fused decode."""

        def convert_to_dict(x):
            return {"boxes": x[0], "scores": x[1], "labels": x[2]}

        if bb_object_pred.dim() == 5 and bb_object_pred.is_cuda:
            corr = None if correction_factor is None else [float(v) for v in correction_factor]
            decoded = HF.detection_decode(
                bb_size_pred.detach(), bb_center_pred.detach(), bb_object_pred.detach(),
                class_pred.detach() if self.n_classes > 2 else None, self.anchor_tensor, corr)
            per_item = [self._tail(bb, sc, cl.squeeze(), nms) for bb, sc, cl in decoded]
        else:
            if bb_object_pred.dim() == 5:
                bb_size_pred, bb_center_pred, bb_object_pred = (
                    torch.stack(self.split(x, self.n_b, 1), -1)
                    for x in (bb_size_pred, bb_center_pred, bb_object_pred))
            per_item = [self.recover_boxes(bb_size_pred[b], bb_center_pred[b], bb_object_pred[b],
                                           class_pred[b], nms=nms,
                                           correction_factor=correction_factor)
                        for b in range(bb_size_pred.shape[0])]
        output = []
        for o in per_item:
            if o[0].shape[0] == 1 and len(o[2].shape) == 1:
                o = o[0], o[1], o[2].unsqueeze(0)
            if to_dict is True:
                o = convert_to_dict(o)
            output.append(o)
        return output


class CoarseDetector3d(torch.nn.Module):
    """Not built: the reference's own forward cannot run. Its ADN after the pyramid is made for
    ``last_size * len(pyramid_layers)`` channels while ``AtrousSpatialPyramidPooling3d`` returns
    ``last_size`` (nets.py:383-393), so the first batch norm fails ("running_mean should contain
    16 elements not 48"): there is no behaviour to mirror."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        raise NotImplementedError(
            "CoarseDetector3d: the reference's forward fails -- the ADN after its pyramid is built "
            "for last_size * len(pyramid_layers) channels, the pyramid returns last_size "
            "(nets.py:383-393): no behaviour to mirror")
