"""Ensemble classifiers (mirror of adell_mri/modules/classification/classification/ensemble.py):
``GenericEnsemble`` (:15-141) runs K encoders, max-pools each output over space, concatenates the
vectors and classifies them with an MLP head, optionally ending in a ``GaussianProcessLayer``;
``AveragingEnsemble`` (:144-187) averages the members' logits.

Kept: arguments, attributes and ``state_dict`` keys (``networks.*``, ``preproc_method.*``,
``prediction_head.*``, ``gaussian_process_head.*``), ``forward_features`` and
``forward(X, return_features)`` with a single tensor or a list repeated over the members, and the
reference's ``GaussianProcessLayer(head_structure[-1], nc, n_classes)`` with
``gaussian_process=True``: ``n_rff = nc``, ONE random feature for a binary problem. The package's
own keyword ``gp_n_rff`` builds ``GaussianProcessLayer(head_structure[-1], gp_n_rff, n_classes,
n_outputs=nc)`` instead.

On the device the K pooled vectors and their concatenation are one launch
(``functional.ensemble_pool``: no per-member pooled tensor, no ``cat``), the Gaussian-process head
is one launch (``functional.gp_phi``), and the averaging ensemble's mean and sigmoid / softmax are
one launch (``functional.ensemble_average``).

``EnsembleNet`` (:190-254) raises ``NotImplementedError``: the reference's own constructor cannot
run (it calls ``torch.nn.Modulelist`` and reads an attribute it never sets).
"""
from typing import Callable

import torch

from ... import functional as HF
from ..layers.gaussian_process import GaussianProcessLayer
from ..layers.linear_blocks import MLP
from ..layers.self_attention import ConcurrentSqueezeAndExcite2d, ConcurrentSqueezeAndExcite3d


class GenericEnsemble(torch.nn.Module):
    def __init__(self, spatial_dimensions: int, networks: list[torch.nn.Module],
                 n_features: list[int] | int, head_structure: list[int], n_classes: int,
                 head_adn_fn: Callable = None, sae: bool = False, gaussian_process: bool = False,
                 split_input: bool = False, gp_n_rff: int = None):
        super().__init__()
        self.spatial_dimensions = spatial_dimensions
        self.networks = torch.nn.ModuleList(networks)
        self.n_features = n_features
        self.head_structure = head_structure
        self.n_classes = n_classes
        self.head_adn_fn = head_adn_fn
        self.sae = sae
        self.gaussian_process = gaussian_process
        self.split_input = split_input
        self.gp_n_rff = gp_n_rff

        if isinstance(self.n_features, int):
            self.n_features = [self.n_features for _ in self.networks]
        self.n_features_final = sum(self.n_features)
        self.initialize_sae_if_necessary()
        self.initialize_head()

    def initialize_head(self):
        nc = 1 if self.n_classes == 2 else self.n_classes
        if self.gaussian_process is True:
            self.prediction_head = torch.nn.Sequential(
                self.head_adn_fn(self.n_features_final),
                MLP(self.n_features_final, self.head_structure[-1],
                    structure=self.head_structure[:-1], adn_fn=self.head_adn_fn))
            if self.gp_n_rff is None:
                # ensemble.py:81-83 as written: the second argument is n_rff
                self.gaussian_process_head = GaussianProcessLayer(self.head_structure[-1], nc,
                                                                  self.n_classes)
            else:
                self.gaussian_process_head = GaussianProcessLayer(
                    self.head_structure[-1], self.gp_n_rff, self.n_classes, n_outputs=nc)
        else:
            self.prediction_head = torch.nn.Sequential(
                self.head_adn_fn(self.n_features_final),
                MLP(self.n_features_final, nc, structure=self.head_structure,
                    adn_fn=self.head_adn_fn))

    def initialize_sae_if_necessary(self):
        if self.sae is True:
            if self.spatial_dimensions == 2:
                self.preproc_method = torch.nn.ModuleList(
                    [ConcurrentSqueezeAndExcite2d(f) for f in self.n_features])
            elif self.spatial_dimensions == 3:
                self.preproc_method = torch.nn.ModuleList(
                    [ConcurrentSqueezeAndExcite3d(f) for f in self.n_features])
        else:
            self.preproc_method = torch.nn.ModuleList([torch.nn.Identity() for _ in self.n_features])

    def forward_features(self, X: torch.Tensor | list[torch.Tensor]) -> torch.Tensor:
        return self.forward(X, return_features=True)

    def forward_head_features(self, X: torch.Tensor | list[torch.Tensor]) -> torch.Tensor:
        """The rows the Gaussian-process head reads: ``prediction_head(forward_features(X))``."""
        return self.prediction_head(self.forward_features(X))

    def forward(self, X: torch.Tensor | list[torch.Tensor],
                return_features: bool = False) -> torch.Tensor:
        if isinstance(X, torch.Tensor):
            X = [X]
        if len(X) == 1:
            X = [X[0] for _ in self.networks]
        outputs = []
        for x, network, pp in zip(X, self.networks, self.preproc_method):
            if hasattr(network, "forward_features"):
                out = network.forward_features(x)
            else:
                out = network(x)
            outputs.append(pp(out))
        outputs = HF.ensemble_pool(outputs)
        if return_features is True:
            return outputs
        output = self.prediction_head(outputs)
        if self.gaussian_process is True:
            output = self.gaussian_process_head(output)
        return output


class AveragingEnsemble(torch.nn.Module):
    def __init__(self, networks: list[torch.nn.Module], n_classes: int, idx: int = None):
        super().__init__()
        self.networks = torch.nn.ModuleList(networks)
        self.n_classes = n_classes
        self.idx = idx

    def forward(self, X: torch.Tensor | list[torch.Tensor]) -> torch.Tensor:
        if isinstance(X, torch.Tensor):
            X = [X]
        if len(X) == 1:
            X = [X[0] for _ in self.networks]
        output = []
        for x, network in zip(X, self.networks):
            out = network(x)
            if self.idx is not None:
                out = out[0]            # ensemble.py:179-180: element 0 whatever ``idx`` is
            output.append(out)
        return HF.ensemble_average(output)


class EnsembleNet(torch.nn.Module):
    def __init__(self, cat_net_args: dict[str, int] | list[dict[str, int]]):
        super().__init__()
        raise NotImplementedError(
            "EnsembleNet: the reference's own constructor cannot run (it calls "
            "torch.nn.Modulelist and reads self.input_structure, which it never sets); use "
            "GenericEnsemble or AveragingEnsemble")
