"""Plain-torch restatement of iBOT's own arithmetic (the masker's index arithmetic, the mask-token
splice, ``reduce``, the per-view masked-token loss in either teacher mode, the centre sums),
evaluated in whatever dtype the inputs carry (the tests feed fp64). The DINO loss itself is
tests/dino_ref.py. Pinned to the reference by tests/golden/ibot_step.npz (tests/test_ibot.py); the
reference for shapes too large to store."""
from itertools import product

import numpy as np
import torch

import dino_ref as R


def patch_indices(coords, image_dimensions):
    """GenericTransformerMasker.retrieve_patch: token indices of the box [lower, upper) --
    c0 w + c1 in 2-D, c0 w + c1 + c2 w h in 3-D with h, w, d = image_dimensions."""
    n = len(image_dimensions)
    lower, upper = coords[:n], coords[n:]
    pts = np.array(list(product(*[range(int(lower[i]), int(upper[i])) for i in range(n)])))
    if n == 2:
        h, w = image_dimensions
        weights = np.array([w, 1])
    else:
        h, w, d = image_dimensions
        weights = np.array([w, 1, w * h])
    return (pts * weights[None, :]).sum(1)


class Masker:
    """The draws of GenericTransformerMasker: per patch one integer in [0, size - max) per axis,
    then one in [min, max) per axis."""

    def __init__(self, image_dimensions, min_patch_size, max_patch_size, seed=42):
        self.dims, self.lo, self.hi = image_dimensions, min_patch_size, max_patch_size
        self.rng = np.random.default_rng(seed)

    def draw(self, n_patches, skip_n=0):
        full = []
        for _ in range(n_patches):
            lower = np.array([self.rng.integers(0, s - m) for s, m in zip(self.dims, self.hi)])
            size = np.array([self.rng.integers(a, b) for a, b in zip(self.lo, self.hi)])
            full.append(patch_indices([*lower, *(lower + size)], self.dims))
        return np.unique(np.concatenate(full) + skip_n)


def splice(x, idx, token):
    """x [B, N, E] with the rows idx of every item replaced by token [E] (out of place)."""
    y = x.clone()
    y[:, torch.as_tensor(np.asarray(idx), dtype=torch.long)] = token.to(x)
    return y


def reduce(x, class_token, reduce_fn):
    """iBOT.reduce on the token logits [B, c + T, K]: (reduced, patch tokens)."""
    c = int(bool(class_token))
    patches = x[:, c:]
    return (x[:, 0] if reduce_fn == "cls" else patches.mean(1)), patches


def view(s, y, m, centers, t1, t2, class_token, reduce_fn, method="center"):
    """(s_red, loss_mask) of one view: the reduction of the student's logits and DinoLoss on the
    rows m of the PATCH tokens of student and teacher."""
    s_red, sp = reduce(s, class_token, reduce_fn)
    _, yp = reduce(y, class_token, reduce_fn)
    m = torch.as_tensor(np.asarray(m), dtype=torch.long)
    if int(m.max()) >= sp.shape[1]:
        raise IndexError(f"index {int(m.max())} is out of bounds for dimension 1 with size {sp.shape[1]}")
    return s_red, R.dino_loss(sp[:, m], yp[:, m].detach(), centers, t1, t2, method)


def token_sums(x, first=0, scale=1.0):
    return x[:, first:].sum(1) * scale


def mask_center_sum(y_1, y_2, class_token):
    """loss_mask.update_centers(cat[t_1, t_2]) on the teachers' PATCH tokens: ([1, K] sum, rows)."""
    c = int(bool(class_token))
    return R.center_sum(torch.cat([y_1[:, c:], y_2[:, c:]]))
