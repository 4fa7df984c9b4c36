"""iBOT network on the HIP kernels (mirror of adell_mri/modules/self_supervised/ibot.py): DINO's
``ViT`` encoder, ``MLP`` projection, L2 normalisation and weight-normalised Linear applied to EVERY
token, a block masker and a learnable mask token spliced into the embedded sequence
(functional.mask_tokens, csrc/ibot.hip). State keys are the reference's, in its order:
``mask_token_`` first (a 1-D parameter of ``n_encoder_features``; the masker holds none), then
``encoder_.*``, ``projection_.op.N.*`` and ``last_layer_.parametrizations.weight.original0 / 1``.

Kept as written:
  * ``forward_training`` embeds, masks (student only), runs the transformer blocks one by one, drops
    the registers, and applies the head to all remaining tokens; ``reduce`` splits the class row off
    first when there is one, "cls" returns it, "mean" the mean over the PATCH tokens.
  * the returned ``mask_coords`` keep the masker's ``+ skip_n`` offset (registers + class token)
    although they are then used on the patch tokens, where those rows are already gone: with
    ``skip_n > 0`` the masked-token loss reads rows shifted by ``skip_n`` and raises ``IndexError``
    when one reaches the number of patch tokens (iBOTPL.calculate_loss_mask).
  * ``extra_tokens`` is a one-element tuple.

Configurations the reference cannot run raise at construction (``_check_configuration``):
  * token width (``embedding_size``, else the patch's features) != ``attention_dim``: the projection
    reads ``attention_dim`` inputs and the forward fails with a shape error -> NotImplementedError;
  * ``n_encoder_features`` != token width: assigning the mask vector fails -> ValueError;
  * ``reduce_fn="cls"`` without a class token: an unbound local at the first forward -> ValueError;
  * ``reduce_fn="max"``: returns torch's (values, indices) pair, on which the loss fails ->
    NotImplementedError.
"""
from typing import Any

import torch

from ... import functional as HF
from ...utils.masking import get_masker
from ..layers.linear_blocks import MLP, WeightNormLinear
from ..layers.vit import ViT


class iBOT(torch.nn.Module):
    def __init__(self, backbone_args: dict[str, Any], projection_head_args: dict[str, Any],
                 out_dim: int, feature_map_dimensions: list[int], n_encoder_features: int,
                 min_patch_size: list[int], max_patch_size: list[int], n_patches: int = 4,
                 reduce_fn: str = "mean", seed: int = 42):
        super().__init__()
        self.backbone_args = backbone_args
        self.projection_head_args = projection_head_args
        self.out_dim = out_dim
        self.feature_map_dimensions = feature_map_dimensions
        self.n_encoder_features = n_encoder_features
        self.min_patch_size = min_patch_size
        self.max_patch_size = max_patch_size
        self.n_patches = n_patches
        self.reduce_fn = reduce_fn
        self.seed = seed
        self.initialize_masker()
        self.initialize_mask_token()
        self.initialize_encoder()
        self._check_configuration()
        self.initialize_projection()
        self.initialize_last_layer()

    def _check_configuration(self):
        width = self.encoder_.embedding.true_n_features
        if width != self.encoder_.attention_dim:
            raise NotImplementedError(
                f"iBOT applies a projection of attention_dim = {self.encoder_.attention_dim} inputs "
                f"to tokens of {width} features: the reference's forward fails with a shape error "
                f"(set embedding_size = attention_dim)")
        if self.n_encoder_features != width:
            raise ValueError(
                f"n_encoder_features = {self.n_encoder_features} but the encoder's tokens have "
                f"{width} features: the reference cannot assign the mask vector to them")
        if self.reduce_fn == "cls" and self.encoder_.use_class_token is not True:
            raise ValueError("reduce_fn='cls' needs use_class_token=True (the reference fails with "
                             "an unbound local at its first forward)")
        if self.reduce_fn == "max":
            raise NotImplementedError(
                "reduce_fn='max': the reference returns torch's (values, indices) pair, on which "
                "its loss fails; use 'mean' or 'cls'")
        if self.reduce_fn not in ("cls", "mean"):
            raise ValueError(f"reduce_fn {self.reduce_fn!r}: 'cls' or 'mean' (the reference "
                             "returns None for anything else)")

    def initialize_masker(self):
        self.patch_masker_ = get_masker(
            model_type="generic_transformer", image_dimensions=self.feature_map_dimensions,
            min_patch_size=self.min_patch_size, max_patch_size=self.max_patch_size,
            n_patches=self.n_patches, n_features=self.n_encoder_features, seed=self.seed)

    def initialize_encoder(self):
        self.encoder_ = ViT(**self.backbone_args)

    def initialize_projection(self):
        if "structure" not in self.projection_head_args:
            raise KeyError("`structure` must be specified in `projection_head_args`.")
        structure = list(self.projection_head_args["structure"])
        self.mlp_out_dim = structure[-1]
        projection_head_args = {**self.projection_head_args, "structure": structure[:-1]}
        self.projection_ = MLP(input_dim=self.encoder_.attention_dim,
                               output_dim=self.mlp_out_dim, **projection_head_args)

    def initialize_last_layer(self):
        self.last_layer_ = WeightNormLinear(self.mlp_out_dim, self.out_dim)
        pair = self.last_layer_.parametrizations.weight
        pair.original0.data.fill_(1)
        pair.original0.requires_grad = False

    def initialize_mask_token(self):
        self.mask_token_ = torch.nn.Parameter(torch.rand(self.n_encoder_features))

    @property
    def class_token(self) -> int:
        return int(self.encoder_.use_class_token is True)

    def reduce(self, X: torch.Tensor):
        """(reduced [B, K], patch tokens [B, T, K]) of the token logits [B, c + T, K]."""
        c = self.class_token
        patches = X[:, c:]
        if self.reduce_fn == "cls":
            return X[:, 0], patches
        return HF.token_mean(X, c), patches

    @property
    def extra_tokens(self):
        return (self.encoder_.n_registers + self.encoder_.use_class_token,)

    def token_logits(self, X: torch.Tensor, mask: bool = False):
        """The head's output on the class token (if any) and every patch token, [B, c + T, out_dim]
        -- what ``forward_training`` reduces and what the fused per-view loss reads in place; with
        ``mask`` also the masker's coordinates."""
        X = self.encoder_.embedding(X)
        mask_coords = None
        if mask is True:
            X, mask_coords = self.patch_masker_(X, mask_vector=self.mask_token_,
                                                n_patches=self.n_patches, skip_n=self.extra_tokens)
        for _, block in enumerate(self.encoder_.tbs.transformer_blocks):
            X = block(X)
        if self.encoder_.n_registers > 0:
            X = X[:, self.encoder_.n_registers:].contiguous()
        X = self.last_layer_(HF.l2_normalize(self.projection_(X)))
        return (X, mask_coords) if mask is True else X

    def forward_training(self, X: torch.Tensor, mask: bool = False):
        if mask is True:
            X, mask_coords = self.token_logits(X, mask=True)
            reduced_X, X = self.reduce(X)
            return reduced_X, X, mask_coords
        return self.reduce(self.token_logits(X))

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return self.forward_representation(X)

    def forward_representation(self, X: torch.Tensor) -> torch.Tensor:
        return self.encoder_(X)[0].permute(0, 2, 1)
