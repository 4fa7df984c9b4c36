"""Deconfounded classification (mirror of
adell_mri/modules/classification/classification/deconfounded_classification.py):
``DeconfoundedNetGeneric`` (:141-341) and ``CategoricalConversion`` (:344-376).

A feature extractor with a ``forward_features`` method, a global max-pool, and on the pooled
features [B, F]: the classification MLP (1-D batch norm + GELU) and, on the first
``n_features_deconfounder`` columns, one small head per categorical confounder and one regression
head for the continuous ones. Constructor arguments, attribute names and ``state_dict`` keys are the
reference's (``feature_extraction_module.*``, ``confound_classifiers.{i}.op.*``,
``confound_regressions.op.*``, ``classification_layer.0.op.*``).

Deviations, on purpose:
  * ``feature_extraction_module="vgg"`` (the reference's default) and the VGG-based
    ``DeconfoundedNet`` raise ``NotImplementedError`` naming VGG, as ``ClassNetPL`` does; any other
    string raises ``ValueError`` (the reference formats a ``net_type`` attribute it never sets).
  * the feature width is the module's ``output_features`` when it has one, else a ``no_grad`` probe
    on the module's own device (the reference probes ``[1, C, 64, 64(, 16)]`` on the CPU).
  * ``CategoricalConversion.forward`` leaves its input list as it was (the reference writes the
    integer codes into it); an unseen category raises ``KeyError`` as there.

A column slice never reaches a kernel as a strided view: ``functional.split_columns`` makes the two
dense halves in one launch, and only when a consumer needs one (``exclude_surrogate_variables``, the
heads' own forward). ``forward(X, heads=False)`` skips the confounder heads: the wrapper's fused
loss (``functional.deconf_heads_loss``) reads the feature rows in place.
"""
from typing import List

import torch

from ... import functional as HF
from ..layers.adn_fn import get_adn_fn
from ..layers.linear_blocks import MLP
from .classification import CatNet, GlobalPooling


class DeconfoundedNet(torch.nn.Module):
    """deconfounded_classification.py:11-138 sits on the VGG classifier, which is not built."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError("DeconfoundedNet: the VGG classifier is not built; use "
                                  "DeconfoundedNetGeneric(feature_extraction_module='cat')")


class DeconfoundedNetGeneric(torch.nn.Module):
    """Feature deconfounder net over any module with ``forward_features`` (:141-341)."""

    def __init__(self, n_classes: int, in_channels: int = 1,
                 feature_extraction_module: torch.nn.Module | str = "vgg",
                 classification_structure: list[int] = [512, 512, 512], n_dim: int = 3,
                 n_features_deconfounder: int = None, n_cat_deconfounder: int | List[int] = None,
                 n_cont_deconfounder: int = None, exclude_surrogate_variables: bool = False,
                 deconfounder_structure: list[int] = None, *args, **kwargs):
        super().__init__()
        self.n_classes = n_classes
        self.feature_extraction_module = feature_extraction_module
        self.in_channels = in_channels
        self.classification_structure = classification_structure
        self.n_dim = n_dim
        self.n_features_deconfounder = n_features_deconfounder
        self.n_cat_deconfounder = n_cat_deconfounder
        self.n_cont_deconfounder = n_cont_deconfounder
        self.exclude_surrogate_variables = exclude_surrogate_variables
        self.deconfounder_structure = deconfounder_structure
        self.args = args
        self.kwargs = kwargs

        if self.n_features_deconfounder is None:
            self.n_features_deconfounder = 0
        if self.n_cat_deconfounder is None:
            self.n_cat_deconfounder = []
        if self.n_cont_deconfounder is None:
            self.n_cont_deconfounder = 0
        if self.deconfounder_structure is None:
            self.deconfounder_structure = []

        self.init_feature_extractor_if_necessary()
        self.get_output_feature_size()
        if not 0 <= self.n_features_deconfounder < self.n_output_features:
            raise ValueError(f"n_features_deconfounder must lie in [0, {self.n_output_features}), got "
                             f"{self.n_features_deconfounder}")
        self.init_deconfounding_layers()
        self.init_classification_layer()
        self.gp = GlobalPooling()

    def get_output_feature_size(self):
        module = self.feature_extraction_module
        if hasattr(module, "output_features"):
            self.n_output_features = int(module.output_features)
            return
        shape = [1, self.in_channels, 64, 64] + ([16] if self.n_dim == 3 else [])
        device = next((p.device for p in module.parameters()), torch.device("cpu"))
        with torch.no_grad():
            self.n_output_features = int(
                module.forward_features(torch.rand(shape, device=device)).shape[1])

    def init_feature_extractor_if_necessary(self):
        if isinstance(self.feature_extraction_module, str):
            if self.feature_extraction_module == "vgg":
                raise NotImplementedError(
                    "feature_extraction_module 'vgg': the VGG classifier is not built")
            elif self.feature_extraction_module == "cat":
                self.feature_extraction_module = CatNet(
                    *self.args, **self.kwargs, in_channels=self.in_channels, n_classes=self.n_classes)
            else:
                raise ValueError("feature_extraction_module '{}' not valid, has to be one of "
                                 "['cat', 'vgg']".format(self.feature_extraction_module))
        elif not hasattr(self.feature_extraction_module, "forward_features"):
            raise TypeError("feature_extraction_module needs a forward_features method")

    def init_deconfounding_layers(self):
        self.confound_classifiers = None
        self.confound_regressions = None
        if self.n_features_deconfounder > 0:
            self.confound_classifiers = torch.nn.ModuleList([])
            if len(self.n_cat_deconfounder) > 0:
                for n_class in self.n_cat_deconfounder:
                    self.confound_classifiers.append(
                        MLP(self.n_features_deconfounder, n_class, self.deconfounder_structure))
            if self.n_cont_deconfounder > 0:
                self.confound_regressions = MLP(
                    self.n_features_deconfounder, self.n_cont_deconfounder,
                    self.deconfounder_structure)

    def init_classification_layer(self):
        if self.exclude_surrogate_variables:
            n_out = self.n_output_features - self.n_features_deconfounder
        else:
            n_out = self.n_output_features
        n_classes = self.n_classes if self.n_classes > 2 else 1
        self.classification_layer = torch.nn.Sequential(
            MLP(n_out, n_classes, self.classification_structure,
                adn_fn=get_adn_fn(1, "batch", "gelu")))

    def linear_heads(self):
        """``([(W, b) per categorical head], (W, b) | None)`` when every confounder head is the
        default identity + ``Linear`` (empty ``deconfounder_structure``), else None."""
        if len(self.deconfounder_structure) > 0 or self.confound_classifiers is None:
            return None
        cat = [(m.op[-1].weight, m.op[-1].bias) for m in self.confound_classifiers]
        cont = None
        if self.confound_regressions is not None:
            cont = (self.confound_regressions.op[-1].weight, self.confound_regressions.op[-1].bias)
        return cat, cont

    def forward(self, X: torch.Tensor, return_features: bool = False, heads: bool = True):
        """``(classification, [confounder logits per categorical head] | None, regression | None,
        features)``, or the pooled features with ``return_features=True``. ``heads=False`` leaves the
        second and third entries None without running the confounder heads."""
        features = self.feature_extraction_module.forward_features(X)
        features = self.gp(features)
        if return_features is True:
            return features
        n_conf = self.n_features_deconfounder
        needs_conf = heads and (self.confound_classifiers is not None
                                or self.confound_regressions is not None)
        conf = rest = None
        if n_conf > 0 and (self.exclude_surrogate_variables or needs_conf):
            conf, rest = HF.split_columns(features, n_conf)
        if self.exclude_surrogate_variables:
            classification = self.classification_layer(rest if rest is not None else features)
        else:
            classification = self.classification_layer(features)
        confounder_classification = None
        confounder_regression = None
        if heads and self.confound_classifiers is not None:
            confounder_classification = [m(conf) for m in self.confound_classifiers]
        if heads and self.confound_regressions is not None:
            confounder_regression = self.confound_regressions(conf)
        return classification, confounder_classification, confounder_regression, features


class CategoricalConversion(torch.nn.Module):
    """Converts categorical variables into integer tensors (:344-376): ``key_lists[i]`` holds the
    categories of variable ``i`` in code order."""

    def __init__(self, key_lists: List[List[str]]):
        super().__init__()
        self.key_lists = key_lists
        self.init_conversion()

    def init_conversion(self):
        self.conversions = []
        for key_list in self.key_lists:
            self.conversions.append({str(key): i for i, key in enumerate(key_list)})

    def forward(self, X: List[str]) -> List[torch.Tensor]:
        assert len(X[0]) == len(self.key_lists)
        codes = [[conversion[x] for x, conversion in zip(item, self.conversions)] for item in X]
        return [torch.as_tensor([codes[j][i] for j in range(len(codes))]).long()
                for i in range(len(X[0]))]
