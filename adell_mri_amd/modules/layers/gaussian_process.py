"""Gaussian-process output layer on the HIP kernels (mirror of
adell_mri/modules/layers/gaussian_process.py; the SNGP head of arXiv:2006.10108): random Fourier
features phi = sqrt(2 / r) cos(b - W LayerNorm(x)), the mean phi weights^T, a precision matrix
fitted after training, and posterior variance and sampling at prediction.

Kept: the constructor arguments and attributes, the initialisation, and the ``state_dict`` keys
and shapes (``W`` [1, r, i], ``b`` [1, r], ``scaling_term`` [], ``inv_conv`` [1, r, r],
``input_norm.weight`` / ``.bias`` [i], ``weights`` [o, r]); ``cov`` is an attribute, not a buffer.

Deviations on purpose:
  * inputs are rows [N, i]; a higher-rank input raises ``NotImplementedError``;
  * ``get_cov`` (once per training) copies ``inv_conv`` to the host, inverts ``inv_conv + 1e-6 I``
    there in fp64 (``pinv`` of ``inv_conv`` when that fails) and stores ``cov`` as fp32 on the
    device: no device solver library;
  * ``get_parameters`` returns the reference's ``(mean [N, o], cov [N, o, o])``; the variance [N]
    is kept as ``last_variance`` and ``parameters_with_variance`` returns ``(mean, var)`` alone;
  * ``rsample(X, n_samples, generator=None, eps=None)`` draws ``eps`` with ``torch.randn`` on the
    device and returns ``mean + sqrt(var) eps``: the distribution of the reference's
    ``MultivariateNormal`` over its diagonal covariance, not its random stream. A variance that
    rounding made negative is used as 0 (the reference raises there).
"""
import math
from typing import Tuple

import numpy as np
import torch

from ... import functional as HF
from ... import ops
from .linear_blocks import LayerNorm


class GaussianProcessLayer(torch.nn.Module):
    def __init__(self, in_channels: int, n_rff: int, n_classes: int, n_outputs: int = None,
                 m: float = 0.999, ordinal: bool = False, normalize_input: bool = True):
        super().__init__()
        self.in_channels = in_channels
        self.n_rff = n_rff
        self.n_outputs = n_outputs if n_outputs is not None else n_rff
        self.out_channels = self.n_outputs
        self.m = m
        self.ordinal = ordinal
        self.n_classes = n_classes
        self.normalize_input = normalize_input
        self.initialize_params()

    def initialize_params(self):
        i, r, o = self.in_channels, self.n_rff, self.n_outputs
        W = torch.normal(torch.zeros([1, r, i]), torch.ones([1, r, i]) * math.sqrt(2.0 / i))
        self.register_buffer("scaling_term", torch.sqrt(torch.as_tensor(2.0 / r)))
        self.register_buffer("W", W.float())
        self.register_buffer("b", torch.rand([1, r]).float() * (2 * torch.pi))
        self.register_buffer("inv_conv", torch.eye(r, r).unsqueeze(0).float())
        self.input_norm = LayerNorm(i) if self.normalize_input else None
        self.weights = torch.nn.Parameter(torch.empty(o, r))
        torch.nn.init.kaiming_uniform_(self.weights, a=math.sqrt(5))
        # sqrt(2 / r) as the kernels take it: a host number, so no launch reads the buffer back
        self._scale = float(np.float32(np.sqrt(np.float32(2.0 / r))))

    def route(self, n: int) -> str:
        """The route ``forward_with_phi`` takes for ``n`` rows (functional.gp_route)."""
        return HF.gp_route(n, self.in_channels, self.n_rff)

    def _norm(self):
        if self.input_norm is None:
            return None, None, 1e-5
        return self.input_norm.weight, self.input_norm.bias, self.input_norm.eps

    def _rows(self, X):
        if X.dim() != 2:
            raise NotImplementedError(
                f"GaussianProcessLayer: rows [N, {self.in_channels}] expected, got "
                f"{tuple(X.shape)}: inputs of rank above 2 are not built")
        return X

    def calculate_phi(self, X: torch.Tensor) -> torch.Tensor:
        gamma, beta, eps = self._norm()
        if self.route(X.shape[0]) == "fused":
            return HF.gp_phi(self._rows(X), gamma, beta, self.W, self.b, None, self._scale, eps)[1]
        return self.forward_with_phi(X)[1]

    def forward_with_phi(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        gamma, beta, eps = self._norm()
        return HF.gp_phi(self._rows(X), gamma, beta, self.W, self.b, self.weights, self._scale, eps)

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return self.forward_with_phi(X)[0]

    @torch.no_grad()
    def update_inv_cov(self, X, probabilities, use_momentum: bool = False):
        self.update_inv_cov_from_phi(self.calculate_phi(X), probabilities, use_momentum)

    @torch.no_grad()
    def update_inv_cov_from_phi(self, phi, probabilities, use_momentum: bool = False):
        """One launch, in place, no host read; the curvature (p (1 - p), summed over the last axis
        for multi-class and ordinal heads) is computed in the kernel."""
        p = probabilities
        if not self.ordinal and self.n_classes == 2:
            p = p.reshape(-1, 1)
        ops.gp_precision_update(self.inv_conv, phi.contiguous(), p.contiguous(), use_momentum, self.m)

    @torch.no_grad()
    def reset_inv_cov(self):
        self.inv_conv.copy_(torch.eye(self.n_rff, dtype=self.inv_conv.dtype,
                                      device=self.inv_conv.device).unsqueeze(0))
        if hasattr(self, "cov"):
            del self.cov

    def get_cov(self):
        P = self.inv_conv.detach().to("cpu", torch.float64).numpy()
        try:
            cov = np.linalg.inv(P + 1e-6 * np.eye(P.shape[-1]))
        except np.linalg.LinAlgError:
            cov = np.linalg.pinv(P)
        self.cov = torch.from_numpy(cov.astype(np.float32)).to(self.inv_conv.device)

    def parameters_with_variance(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """(mean [N, o], var [N]): one launch for phi and the mean, one for the variance."""
        if hasattr(self, "cov") is False:
            raise Exception("self.get_cov() must be called before getting parameters")
        mean, phi = self.forward_with_phi(X)
        var = ops.gp_variance(phi.detach(), self.cov)
        self.last_variance = var
        return mean, var

    def get_parameters(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        mean, var = self.parameters_with_variance(X)
        return mean, torch.diag_embed(var.unsqueeze(-1).expand(-1, self.n_outputs))

    def rsample(self, X: torch.Tensor, n_samples: int, generator=None, eps=None) -> torch.Tensor:
        """[n_samples, N, o]; ``eps`` [n_samples, N, o]: the standard normal draws to use."""
        return self.sample_statistics(X, n_samples, generator, eps)[0]

    def sample_statistics(self, X, n_samples, generator=None, eps=None, parameters=None):
        """(samples [S, N, o], their mean [N, o], their unbiased std [N, o]) in one launch after
        the parameters (``parameters``: a ``(mean, var)`` already computed)."""
        mean, var = self.parameters_with_variance(X) if parameters is None else parameters
        mean = mean.detach()
        if eps is None:
            eps = torch.randn((n_samples, *mean.shape), device=mean.device, dtype=torch.float32,
                              generator=generator)
        return ops.gp_sample(mean.contiguous(), var, eps.contiguous())
