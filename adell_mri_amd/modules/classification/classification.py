"""Classification networks on the HIP kernels (mirror of
adell_mri/modules/classification/classification/classification.py): ``CatNet`` (:264-442),
``OrdNet`` (:445-544) and ``ViTClassifier`` (:754-836), with ``label_to_ordinal`` /
``ordinal_prediction_to_class`` (:27-65) and ``GlobalPooling`` (layers/standard_blocks.py:10-37).

Module trees, attribute names and ``state_dict`` keys are the reference's (``res_net.*`` with
``feature_extraction`` the same module, ``classification_layer.0.op.*`` for ``CatNet`` and
``ViTClassifier``, ``classification_layer.op.*`` plus ``ordinal_bias`` / ``ordinal_bias_scale`` for
``OrdNet``). ``batch_ensemble=n`` (a member count) goes to the ResNet backbone, whose stages then
run inside ``BatchEnsembleWrapper``s; ``forward(X, batch_idx=...)`` picks the members. Not built,
each raising ``NotImplementedError`` that names the argument: the Gaussian-process head
(``gaussian_process=True``), a bare ``batch_ensemble=True`` (the reference's annotation says bool,
its layers need the member count and fail on a bool) and SeqPool (``use_class_token="seqpool"``).

One deviation: with a ``feature_extraction`` module given, ``CatNet`` reads the module's
``output_features`` when it has one, and otherwise runs the reference's probe tensor on the module's
own device under ``no_grad`` (the reference always probes on the CPU, where these modules cannot run).
"""
from typing import List, Tuple

import torch

from ... import functional as HF
from ..layers.adn_fn import ActDropNorm, get_adn_fn
from ..layers.linear_blocks import MLP
from ..layers.res_net import ResNetBackbone
from ..layers.vit import ViT

resnet_default = [(64, 128, 5, 2), (128, 256, 3, 5)]
maxpool_default = [(2, 2, 2), (2, 2, 2)]


def label_to_ordinal(label: torch.Tensor, n_classes: int, ignore_0: bool = True) -> torch.Tensor:
    """classification.py:27-52: for a label L in a [B, 1] tensor, the [B, n_classes] rows that are 1
    below index max(L - 1, 0) (``ignore_0``) or L, and 0 from there on. Host-side label
    preparation: plain torch."""
    label = torch.squeeze(label, 1)
    if ignore_0 is True:
        label = torch.clamp(label - 1, min=0)
    below = torch.arange(n_classes, device=label.device)[None, :] < label[:, None]
    return below.to(torch.int64)


def ordinal_prediction_to_class(x: torch.Tensor) -> torch.Tensor:
    """classification.py:55-65: the number of ordinal outputs above 0.5."""
    return (x > 0.5).sum(dim=1)


class GlobalPooling(torch.nn.Module):
    """standard_blocks.py:10-37: the maximum or the mean over everything behind the channel axis;
    2-D inputs pass through. "max" is the global max-pool ``ProjectionHead`` uses, "average" the
    row mean."""

    def __init__(self, mode: str = "max"):
        super().__init__()
        if mode not in ("average", "max"):
            raise ValueError("mode must be one of [average,max]")
        self.mode = mode

    def forward(self, X):
        if X.dim() <= 2:
            return X
        if self.mode == "average":
            return HF.row_mean(X.flatten(start_dim=2))
        while X.dim() < 5:      # [B, C, L] or a 2-D feature map: a volume with unit axes
            X = X.unsqueeze(2)
        if X.dim() > 5:
            X = X.flatten(start_dim=4)
        return HF.max_pool3d(X, tuple(X.shape[2:]), tuple(X.shape[2:]), 0).flatten(1)


def _probe_features(module, in_channels, spatial_dim):
    """The width of ``module``'s output: its ``output_features``, else the reference's probe
    (classification.py:363-367) on the module's own device."""
    if hasattr(module, "output_features"):
        return int(module.output_features)
    shape = [2, in_channels, 128, 128] + ([32] if spatial_dim == 3 else [])
    device = next((p.device for p in module.parameters()), torch.device("cpu"))
    with torch.no_grad():
        return int(module(torch.ones(shape, device=device)).shape[1])


class CatNet(torch.nn.Module):
    """Categorical classifier (classification.py:264-442): ResNet backbone (or the given feature
    extractor), global max-pool, an MLP head of three hidden layers with 1-D batch norm, GELU and a
    dropout of 0.1 (hard-coded, as in the reference). One logit for two classes."""

    def __init__(self, spatial_dimensions: int = 3, in_channels: int = 1, n_classes: int = 2,
                 feature_extraction: torch.nn.Module = None,
                 resnet_structure: List[Tuple[int, int, int, int]] = resnet_default,
                 maxpool_structure: List[Tuple[int, int, int]] = maxpool_default,
                 adn_fn: torch.nn.Module = None, res_type: str = "resnet",
                 classification_structure: List[int] = None, batch_ensemble: bool = False,
                 skip_last_activation: bool = False, gaussian_process: bool = False):
        super().__init__()
        if gaussian_process:
            raise NotImplementedError("gaussian_process=True: the Gaussian-process head is not built")
        if isinstance(batch_ensemble, bool) and batch_ensemble:
            raise NotImplementedError("batch_ensemble=True: give the number of members; the "
                                      "batch-ensemble layers cannot size their tables from a flag")
        if batch_ensemble and feature_extraction is not None:
            raise NotImplementedError("batch_ensemble with a given feature_extraction: the members "
                                      "live in the ResNet backbone this class builds")
        self.spatial_dim = spatial_dimensions
        self.in_channels = in_channels
        self.n_classes = n_classes
        self.feature_extraction = feature_extraction
        self.resnet_structure = resnet_structure
        self.maxpool_structure = maxpool_structure
        self.adn_fn = adn_fn
        self.res_type = res_type
        self.classification_structure = classification_structure
        self.batch_ensemble = batch_ensemble
        self.skip_last_activation = skip_last_activation
        self.gaussian_process = gaussian_process
        if self.adn_fn is None:
            norm = {2: torch.nn.BatchNorm2d, 3: torch.nn.BatchNorm3d}[self.spatial_dim]
            self.adn_fn = lambda s: ActDropNorm(s, norm_fn=norm)
        self.init_layers()
        self.init_classification_layer()

    def init_layers(self):
        if self.feature_extraction is None:
            self.res_net = ResNetBackbone(
                self.spatial_dim, self.in_channels, self.resnet_structure, adn_fn=self.adn_fn,
                maxpool_structure=self.maxpool_structure, res_type=self.res_type,
                batch_ensemble=int(self.batch_ensemble), skip_last_activation=self.skip_last_activation)
            self.feature_extraction = self.res_net
            self.last_size = self.resnet_structure[-1][0]
        else:
            self.last_size = _probe_features(self.feature_extraction, self.in_channels,
                                             self.spatial_dim)
        self.output_features = self.last_size

    def init_classification_layer(self):
        if self.n_classes == 2:
            final_n = 1
            self.last_act = torch.nn.Sigmoid()
        else:
            final_n = self.n_classes
            self.last_act = torch.nn.Softmax(1)
        if self.classification_structure is None:
            self.classification_structure = [self.last_size for _ in range(3)]
        self.gp = GlobalPooling()
        self.classification_layer = torch.nn.Sequential(
            MLP(self.last_size, final_n, self.classification_structure,
                adn_fn=get_adn_fn(1, "batch", "gelu", 0.1)))

    def forward_features(self, X: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        return self.forward(X, *args, **kwargs, return_features=True)

    def forward(self, X: torch.Tensor, return_features: bool = False, *args, **kwargs):
        features = self.gp(self.feature_extraction(X, *args, **kwargs))
        if return_features is True:
            return features
        return self.classification_layer(features)


class OrdNet(CatNet):
    """Ordinal classifier (classification.py:445-544): one pre-bias value per item from an MLP head
    (1-D batch norm, leaky ReLU, no dropout), repeated over the K - 1 thresholds and shifted by
    ``ordinal_bias * ordinal_bias_scale`` (CORAL). The last linear's bias is zeroed and stays
    trainable: the reference's ``bias.data.requires_grad = False`` acts on a temporary. Without a
    ``classification_structure`` the head takes ``CatNet``'s default of three layers (the reference
    fails there)."""

    def init_classification_layer(self):
        self.gp = GlobalPooling()
        if self.classification_structure is None:
            # CatNet's default; the reference hands None on to its MLP, which cannot take it
            self.classification_structure = [self.last_size for _ in range(3)]
        self.classification_layer = MLP(self.last_size, 1, self.classification_structure,
                                        adn_fn=get_adn_fn(1, "batch", "leaky_relu", 0.0))
        self.classification_layer.op[-1].bias.data.zero_()
        self.ordinal_bias = torch.nn.parameter.Parameter(
            torch.arange(self.n_classes - 1, 0, -1).float() - self.n_classes // 2,
            requires_grad=True)
        self.ordinal_bias_scale = torch.nn.parameter.Parameter(
            torch.tensor(1 / (self.n_classes - 1)), requires_grad=True)
        self.last_act = torch.nn.Sigmoid()

    def forward_features(self, X: torch.Tensor) -> torch.Tensor:
        return self.forward(X, return_features=True)

    def forward(self, X: torch.Tensor, return_features: bool = False,
                return_pre_bias: bool = False, return_only_pre_bias: bool = False):
        # (no batch_idx, as the reference's signature: an ordinal net draws or averages its members)
        features = self.gp(self.feature_extraction(X))
        if return_features is True:
            return features
        pre_bias = self.classification_layer(features)
        # [B, 1] + [K - 1]: the repeat over the thresholds and the shift (K - 1 numbers per item)
        p_ordinal = pre_bias + self.ordinal_bias * self.ordinal_bias_scale
        if return_pre_bias is True:
            return p_ordinal, pre_bias
        if return_only_pre_bias is True:
            return pre_bias
        return p_ordinal


class ViTClassifier(ViT):
    """ViT as a classifier (classification.py:754-836): the registers are dropped, the class token
    (``use_class_token=True``) or the mean over the tokens is the feature vector, the head is one
    hidden layer with layer norm and GELU. ``use_class_token="seqpool"`` raises
    ``NotImplementedError``."""

    def __init__(self, n_classes: int, use_class_token: bool = False, *args, **kwargs):
        if use_class_token == "seqpool":
            raise NotImplementedError("use_class_token='seqpool': SeqPool is not built")
        kwargs["use_class_token"] = use_class_token
        self.use_seq_pool = False
        super().__init__(*args, **kwargs)
        self.n_classes = n_classes
        nc = 1 if self.n_classes == 2 else self.n_classes
        self.classification_layer = torch.nn.Sequential(
            MLP(self.input_dim_primary, nc, [self.input_dim_primary for _ in range(1)],
                adn_fn=get_adn_fn(1, "layer", "gelu", 0.0)))
        self.output_features = self.input_dim_primary

    def forward_features(self, X: torch.Tensor) -> torch.Tensor:
        return self.forward(X, return_features=True)

    def forward(self, X: torch.Tensor, return_features: bool = False) -> torch.Tensor:
        embeded_X, _ = super().forward(X)
        if self.n_registers > 0:
            embeded_X = embeded_X[:, self.n_registers:]
        if self.use_class_token is True:
            embeded_X = embeded_X[:, 0].contiguous()
        else:
            embeded_X = HF.token_mean(embeded_X)
        if return_features is True:
            return embeded_X
        return self.classification_layer(embeded_X)
