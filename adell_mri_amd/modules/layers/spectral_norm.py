"""Spectral normalisation as a weight parametrization: torch's ``_SpectralNorm`` (buffers ``_u`` /
``_v``, keys ``parametrizations.<name>.original`` / ``.0._u`` / ``.0._v``, normal draws and 15
power iterations at construction, the exact 1-D path) with the training-time power iteration and
``W / sigma`` on the fused kernels (``functional.spectral_normalize``) for fp32 device weights of
rank >= 2. CPU tensors, other dtypes and matrices beyond the fused limits take torch's own forward:
the "composed" route and the oracle of the fused ones. The class name is the one the reference's
callback excludes and its checkpoints carry."""
import torch
from torch.nn.utils import parametrize
from torch.nn.utils.parametrizations import _SpectralNorm as _TorchSpectralNorm

from ... import functional as HF
from ... import ops


class _SpectralNorm(_TorchSpectralNorm):
    def route(self, weight):
        """"block" / "grid" when ``forward(weight)`` runs the fused kernels, else "composed"."""
        if weight.ndim < 2 or not weight.is_cuda or weight.dtype != torch.float32 \
                or self._u.dtype != torch.float32 or 0 in weight.shape:
            return "composed"
        outer, h, inner = ops.spectral_norm_matrix(weight.shape, self.dim)
        return HF.spectral_norm_route(h, outer * inner)

    def forward(self, weight):
        if self.route(weight) == "composed":
            out = super().forward(weight)
        else:
            out = HF.spectral_normalize(weight, self._u, self._v, self.n_power_iterations, self.eps,
                                        self.dim, self.training)
        # a fresh tensor per access: its f16x3 packs live on it, not in the registry (functional._packed)
        out._adell_transient = True
        return out


def spectral_norm(module, name="weight", n_power_iterations=1, eps=1e-12, dim=None):
    """``torch.nn.utils.parametrizations.spectral_norm`` with this package's ``_SpectralNorm``: ``dim``
    defaults to 1 for ``ConvTranspose{1,2,3}d`` instances and 0 otherwise; ``n_power_iterations <= 0``
    raises torch's ``ValueError``."""
    weight = getattr(module, name, None)
    if not isinstance(weight, torch.Tensor):
        raise ValueError(f"Module '{module}' has no parameter or buffer with name '{name}'")
    if dim is None:
        transposed = (torch.nn.ConvTranspose1d, torch.nn.ConvTranspose2d, torch.nn.ConvTranspose3d)
        dim = 1 if isinstance(module, transposed) else 0
    parametrize.register_parametrization(module, name,
                                         _SpectralNorm(weight, n_power_iterations, dim, eps))
    return module
