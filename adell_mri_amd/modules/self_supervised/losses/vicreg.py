"""VICReg loss (mirror of adell_mri/modules/self_supervised/losses/vicreg.py:30-165).

``forward(X1, X2)`` returns ``(lam * inv, mu * var, nu * cov)`` like the reference; the
three terms and their gradients come from one HIP kernel each way (csrc/ssl.hip), which
uses the B x B Gram matrix of the centred embeddings instead of materialising the D x D
covariance matrix: sum(offdiag(C)^2) = ||Xc Xc^T||_F^2 / (B-1)^2 - sum(diag(C)^2).

``VICRegLocalLoss`` (vicreg.py:168-404, VICRegL) adds the local term on feature maps and boxes:
the top-gamma pair ranking and the row gather of csrc/vicregl.hip in front of the same kernels.
"""
from typing import Tuple

import torch

from .... import functional as HF


class VICRegLoss(torch.nn.Module):
    def __init__(self, min_var: float = 1.0, eps: float = 1e-4, lam: float = 25.0,
                 mu: float = 25.0, nu: float = 0.1):
        super().__init__()
        self.min_var = min_var
        self.eps = eps
        self.lam = lam
        self.mu = mu
        self.nu = nu

    def flatten_if_necessary(self, x):
        """[B, C, *spatial] feature maps -> [B, C] spatial means (vicreg.py:138-141), on the
        channel-statistics kernel."""
        if len(x.shape) > 2:
            if x.dim() == 5:
                return HF.channel_mean(x)
            if x.dim() == 4:
                return HF.channel_mean(x.unsqueeze(2))
            return HF.channel_mean(x.unsqueeze(2).unsqueeze(2))
        return x

    def vicreg_loss(self, X1: torch.Tensor, X2: torch.Tensor, adj: float = 1.0):
        """(var_loss, cov_loss, inv_loss), unweighted (vicreg.py:112-136)."""
        terms = HF.vicreg_terms(X1, X2, self.min_var, self.eps)
        return terms[1], terms[2] / adj, terms[0]

    def forward(self, X1: torch.Tensor, X2: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        var_loss, cov_loss, inv_loss = self.vicreg_loss(self.flatten_if_necessary(X1),
                                                        self.flatten_if_necessary(X2))
        return self.lam * inv_loss, self.mu * var_loss, self.nu * cov_loss


MAX_GAMMA = 64   # the candidate lists of the top-pairs kernel (csrc/vicregl.hip)


def _tokens(X: torch.Tensor) -> torch.Tensor:
    """[B, C, *spatial] -> [B, T, C] token rows: a view of the channels-last activation the
    backbones produce (no permute to NCDHW and back), a copy only for a channels-first input."""
    perm = (0,) + tuple(range(2, X.dim())) + (1,)
    return X.permute(*perm).reshape(X.shape[0], -1, X.shape[1])


class VICRegLocalLoss(VICRegLoss):
    """Local VICReg loss, VICRegL (mirror of adell_mri/modules/self_supervised/losses/
    vicreg.py:168-404), for [B, C, *spatial] feature maps of two views and their boxes
    [B, 2 * ndim] = (lo..., hi...).

    ``forward`` returns ``(lam * inv * alpha, mu * var * alpha, nu * cov * alpha, local)`` with
    ``alpha = 0.9``: the first three are the VICReg terms of the spatial means, ``local`` is
    ``short + long``, each ``(L(X1, X2) + L(X2, X1)) * (1 - alpha) / 2`` -- short ranks the distances
    between the token-grid coordinates mapped into each view's box (``grid * (hi - lo) + lo``),
    long the distances between the [T, C] token features.

    The reference is reproduced AS WRITTEN (like the notes in ``segmentation/losses.py``):
      * ``torch.topk`` on the flattened T x T matrix takes the gamma LARGEST distances, the most
        distant pairs, not the nearest;
      * of a selected pair (i, j) only the row index i ("column 0" of the unravelled index) is
        used, for BOTH views: rows i of Xa and rows i of Xb are gathered, j is dropped;
      * the B * gamma gathered rows of each view give ``(var + cov / gamma + inv) / gamma`` of
        ``vicreg_loss(f1, f2, adj=gamma)``, unweighted by lam / mu / nu.
    The indices carry no gradient; gradients flow through the gathered rows and the spatial means.

    On the device (csrc/vicregl.hip) the T x T matrices are never formed. The matrix of direction
    (X2, X1) is the transpose of that of (X1, X2), so ``forward`` ranks once per kind and takes the
    row indices for one direction and the column indices for the other. Ties are broken by
    (distance descending, flat index i * T + j of the (X1, X2) matrix ascending); the reference
    leaves them to ``torch.topk``. Differing view shapes make the reference index view 2 with
    view-1 indices (it fails for T2 < T1): ``X1.shape == X2.shape`` is required here, and
    ``1 <= gamma <= 64``, ``gamma <= T * T``; a ``ValueError`` otherwise.
    """

    def __init__(self, min_var: float = 1.0, eps: float = 1e-4, lam: float = 25.0,
                 mu: float = 25.0, nu: float = 0.1, gamma: int = 10):
        super().__init__(min_var=min_var, eps=eps, lam=lam, mu=mu, nu=nu)
        if not 1 <= int(gamma) <= MAX_GAMMA:
            raise ValueError(f"VICRegLocalLoss: 1 <= gamma <= {MAX_GAMMA} on the HIP path, got {gamma}")
        self.gamma = int(gamma)
        self.alpha = 0.9

    def _check(self, X1, X2):
        if X1.shape != X2.shape or X1.dim() not in (4, 5):
            raise ValueError(f"VICRegLocalLoss: two [B, C, *spatial] maps (2 or 3 spatial dimensions) "
                             f"of one shape, got {tuple(X1.shape)} and {tuple(X2.shape)}")
        T = 1
        for s in X1.shape[2:]:
            T *= int(s)
        if self.gamma > T * T:
            raise ValueError(f"VICRegLocalLoss: gamma {self.gamma} exceeds the {T * T} token pairs")

    def _local_from_pairs(self, Ta, Tb, pairs, col):
        """The local term from token rows [B, T, C] and ranked pairs: column ``col`` of the pairs
        indexes BOTH views."""
        g = self.gamma
        var_loss, cov_loss, inv_loss = self.vicreg_loss(HF.gather_rows(Ta, pairs, col),
                                                        HF.gather_rows(Tb, pairs, col), g)
        return (var_loss + cov_loss + inv_loss) / g

    def local_loss(self, X1: torch.Tensor, X2: torch.Tensor, all_dists: torch.Tensor):
        """Reference signature (vicreg.py:234-257), for a distance matrix [B, T, T] the caller has
        already formed: ``torch.topk`` ranks it (its tie order), the rows are gathered on the
        device. ``forward`` does not come here: it never forms the matrix."""
        self._check(X1, X2)
        T = all_dists.shape[-1]
        _, idxs = torch.topk(all_dists.detach().flatten(start_dim=1), self.gamma, 1)
        rows = torch.div(idxs, T, rounding_mode="floor")
        pairs = torch.stack([rows, idxs - rows * T], -1).to(torch.int32).contiguous()
        return self._local_from_pairs(_tokens(X1), _tokens(X2), pairs, 0)

    def location_local_loss(self, X1: torch.Tensor, X2: torch.Tensor, box_X1: torch.Tensor,
                            box_X2: torch.Tensor) -> torch.Tensor:
        """vicreg.py:259-288: the pairs of tokens most distant in the space of the two boxes."""
        self._check(X1, X2)
        pairs = HF.top_pairs_boxes(box_X1, box_X2, X1.shape[2:], self.gamma)
        return self._local_from_pairs(_tokens(X1), _tokens(X2), pairs, 0)

    def feature_local_loss(self, X1: torch.Tensor, X2: torch.Tensor):
        """vicreg.py:290-309: the pairs of tokens most distant in feature space."""
        self._check(X1, X2)
        T1, T2 = _tokens(X1), _tokens(X2)
        return self._local_from_pairs(T1, T2, HF.top_pairs(T1, T2, self.gamma), 0)

    def forward(self, X1: torch.Tensor, X2: torch.Tensor, box_X1: torch.Tensor,
                box_X2: torch.Tensor
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        self._check(X1, X2)
        var_loss, cov_loss, inv_loss = self.vicreg_loss(self.flatten_if_necessary(X1),
                                                        self.flatten_if_necessary(X2))
        T1, T2 = _tokens(X1), _tokens(X2)
        rem = 1 - self.alpha
        local = 0.0
        for pairs in (HF.top_pairs_boxes(box_X1, box_X2, X1.shape[2:], self.gamma),
                      HF.top_pairs(T1, T2, self.gamma)):
            # direction (X1, X2): the row indices; (X2, X1): the transposed matrix, the columns
            local = local + (self._local_from_pairs(T1, T2, pairs, 0) * rem
                             + self._local_from_pairs(T2, T1, pairs, 1) * rem) / 2
        return (self.lam * inv_loss * self.alpha, self.mu * var_loss * self.alpha,
                self.nu * cov_loss * self.alpha, local)
