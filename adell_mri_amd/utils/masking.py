"""Block masker of transformer-style tensors (mirror of adell_mri/utils/masking.py:
``GenericTransformerMasker``, ``get_masker``, ``_check_patch_size``). Host numpy logic as in the
reference -- constructor, attributes, the order of the random draws and the returned coordinates are
the reference's -- with one difference on purpose: the mask vector is written by
``functional.mask_tokens`` (csrc/ibot.hip) into a NEW tensor, where the reference assigns into its
input in place.

Kept as written:
  * per patch the draws are one ``rng.integers(0, size - max)`` per axis for the lower corner, then
    one ``rng.integers(min, max)`` per axis for the extent (``np.random.default_rng(seed)``);
  * the token index of a coordinate is ``c0 * w + c1`` in 2-D and ``c0 * w + c1 + c2 * w * h`` in 3-D
    with ``h, w, d = image_dimensions`` -- the reference's expression, whatever order the embedding
    gives its tokens;
  * the result is ``np.unique(concatenate(patches) + skip_n)``; the same rows in every batch item;
  * ``n_features`` is stored and nothing is built from it (the generic masker has no positional
    embedding, hence no parameters).

The reference's other two maskers (``"transformer"``, ``"convolutional"``) are not mirrored:
``get_masker`` raises ``NotImplementedError`` for them.
"""
from itertools import product
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import functional as HF


def _check_patch_size(image_dimensions: Sequence[int], max_patch_size: Sequence[int]):
    if any([m >= s for s, m in zip(image_dimensions, max_patch_size)]):
        raise ValueError(
            "max_patch_size must be strictly smaller than image_dimensions in all dimensions. "
            f"image_dimensions: {image_dimensions}; max_patch_size: {max_patch_size}")


class GenericTransformerMasker(torch.nn.Module):
    def __init__(self, image_dimensions: List[int], min_patch_size: List[int],
                 max_patch_size: List[int], n_features: int = None, n_patches: int = 4,
                 seed: int = 42):
        super().__init__()
        self.image_dimensions = image_dimensions
        self.min_patch_size = min_patch_size
        self.max_patch_size = max_patch_size
        self.n_features = n_features
        self.n_patches = n_patches
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.n_dim = len(self.image_dimensions)
        assert self.n_dim in [2, 3]
        _check_patch_size(self.image_dimensions, self.max_patch_size)

    def sample_patch(self):
        upper_sampling_bound = [size - patch_size for size, patch_size in
                                zip(self.image_dimensions, self.max_patch_size)]
        lower_bound = np.array([self.rng.integers(0, i) for i in upper_sampling_bound])
        patch_size = np.array([self.rng.integers(m, M)
                               for m, M in zip(self.min_patch_size, self.max_patch_size)])
        upper_bound = lower_bound + patch_size
        return [*lower_bound, *upper_bound]

    def sample_patches(self, n_patches: int):
        return [self.sample_patch() for _ in range(n_patches)]

    def retrieve_patch(self, patch_coords: List[int]) -> np.ndarray:
        lower, upper = patch_coords[:self.n_dim], patch_coords[self.n_dim:]
        coords = np.array([c for c in product(*[range(lower[i], upper[i])
                                                for i in range(self.n_dim)])])
        if self.n_dim == 2:
            h, w = self.image_dimensions
            expression = np.array([w, 1])[None, :]
        else:
            h, w, d = self.image_dimensions
            expression = np.array([w, 1, w * h])[None, :]
        return np.sum(coords * expression, 1)

    def __call__(self, X: torch.Tensor, mask_vector: torch.Tensor = None, n_patches: int = None,
                 patch_coords=None, skip_n: int = 0) -> Tuple[torch.Tensor, np.ndarray]:
        """(masked X, coordinates). With a mask vector the coordinates are the sorted unique rows
        (``+ skip_n``) that were replaced; without one X comes back as it is and the coordinates
        are the list of per-patch index arrays, as in the reference. IndexError -- on the host,
        before any kernel -- for a row beyond the sequence."""
        if n_patches is None:
            n_patches = self.n_patches
        if patch_coords is None:
            patch_coords = self.sample_patches(n_patches)
        full_coords = [self.retrieve_patch(coords) for coords in patch_coords]
        if mask_vector is not None:
            full_coords = np.unique(np.concatenate(full_coords) + skip_n)
            X = HF.mask_tokens(X, full_coords, mask_vector)
        return X, full_coords


def get_masker(model_type: str, *args, **kwargs):
    if model_type == "generic_transformer":
        return GenericTransformerMasker(*args, **kwargs)
    if model_type in ("transformer", "convolutional"):
        raise NotImplementedError(f"masker {model_type!r} is not mirrored on the HIP path: only "
                                  "'generic_transformer' (what iBOT uses) is")
    raise NotImplementedError("model_type must be either 'transformer' or 'convolutional'")
