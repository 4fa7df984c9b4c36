"""ViT autoencoder and masked autoencoder on the HIP kernels (mirror of
adell_mri/modules/self_supervised/autoencoders.py): a linear patch embedding without class token
whose tokens are ``E = prod(patch_size) * in_channels`` wide, an encoder ``TransformerBlockStack``
that sees only the kept tokens of every item, a learnable mask token (times a learnable scale)
spliced in at the masked places, a decoder stack and a two-layer head back to ``prod(patch_size) *
in_channels`` values per token. State keys are the reference's, in its order: ``positional_embedding``,
``mask_token_scale``, ``mask_token``, then ``proj.*`` (``proj.positional_embedding`` is the SAME
Parameter as ``positional_embedding``: both keys are in the state, ``parameters()`` yields it once),
``encoder.*``, ``decoder.*``, ``decoder_pred.{0,2}.*``.

Kept as written:
  * ``len_keep = int(L * (1 - mask_ratio))``, the noise ``rng.uniform(size=[N, L])`` (float64) of the
    one ``np.random.default_rng(seed)``, drawn by EVERY forward, validation included; stable argsorts;
    the kept tokens per item and in shuffled order;
  * the positional embedding is added twice, inside ``proj`` and again after the un-shuffle;
  * the "image": ``pred.view(B, L, ph, pw, C).permute(0, 4, 1, 2, 3).contiguous().view(B, C, H, W)`` is
    not a spatial un-patchify -- element (b, c) holds pred[b, l, p C + c] at flat offset l P + p;
  * ``input_dim_size`` is stored and unused; ``mask`` is returned and unused by the loss.

What differs, in how it is computed and not in what:
  * the argsorts run on the host with numpy (``kind="stable"``; the noise is host data already) and
    the index tables go to the device in one copy (``ops.MaeShuffle``);
  * ``torch.gather`` / ``repeat`` / ``cat`` / ``gather`` / ``+`` are row kernels (csrc/mae.hip):
    ``functional.mae_keep_tokens`` and ``functional.mae_restore_tokens``;
  * ``forward_tokens`` returns ``(pred, mask)`` without the image copy: the wrapper takes the loss
    from it (``functional.mae_reconstruction_loss``);
  * the reference's ``ViTMaskedAutoEncoder.__init__`` builds every module twice (once in
    ``super().__init__``, once itself; the second set survives): here once, in the same order of keys;
  * ``ViTAutoEncoder.forward`` takes the output of each stack's ``(output, intermediates)`` pair;
    the reference adds the positional embedding to the pair itself and raises ``TypeError``;
  * two failures are raised at construction instead of in the first forward: an ``image_size`` that
    is not 2-D (the reference fails unpacking ``X.shape``) and a ``mask_fraction`` that keeps no token
    (the reference runs its encoder on an empty sequence) are ``ValueError``.
``ConvNeXtAutoEncoder`` is not mirrored (its ``forward`` is the identity and its backbone is not part
of this package).
"""
from typing import Any, Dict, Tuple

import numpy as np
import torch

from ... import functional as HF
from ... import ops
from ..layers.linear_blocks import Linear
from ..layers.vit import LinearEmbedding, TransformerBlockStack


class GELU(torch.nn.GELU):
    """torch.nn.GELU (exact) on the elementwise kernel."""

    def forward(self, X):
        return HF.elementwise(X, act="gelu")


def _shuffle(n: int, length: int, mask_ratio: float, rng: np.random.Generator, device):
    """The draw of ``random_masking`` as an ``ops.MaeShuffle``."""
    len_keep = int(length * (1 - mask_ratio))
    noise = rng.uniform(size=[n, length])        # noise in [0, 1]; small is keep, large is remove
    ids_shuffle = np.argsort(noise, axis=1, kind="stable")
    return ops.MaeShuffle(ids_shuffle, len_keep, device)


def random_masking(x: torch.Tensor, mask_ratio: float,
                   rng: np.random.Generator) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Per-sample random masking by per-sample shuffling (argsort of random noise).

    Args:
        x (torch.Tensor): tensor with shape [batch, n_tokens, embedding_size].
        mask_ratio (float): ratio of tokens to mask.
        rng (np.random.Generator): random number generator.

    Returns ``(x_masked [N, len_keep, D], mask [N, L] (0 keep, 1 remove), ids_restore [N, L] int64)``.
    """
    N, L, D = x.shape
    shuffle = _shuffle(N, L, mask_ratio, rng, x.device)
    return HF.mae_keep_tokens(x, shuffle), shuffle.mask, shuffle.restore.long()


class ViTAutoEncoder(torch.nn.Module):
    """ViT autoencoder."""

    def __init__(self, image_size, patch_size, in_channels: int, input_dim_size: int,
                 encoder_args: Dict[str, Any], decoder_args: Dict[str, Any],
                 embed_method: str = "linear", dropout_rate: float = 0.0,
                 decoder_pred_ratio: float = 4.0):
        super().__init__()
        self.image_size = image_size
        self.patch_size = patch_size
        self.in_channels = in_channels
        self.input_dim_size = input_dim_size
        self.encoder_args = encoder_args
        self.decoder_args = decoder_args
        self.embed_method = embed_method
        self.dropout_rate = dropout_rate
        self.decoder_pred_ratio = decoder_pred_ratio

        self.init_projection()
        self.init_encoder()
        self.init_positional_embedding()
        self.init_decoder()
        self.init_decoder_pred()

    def init_projection(self):
        self.proj = LinearEmbedding(self.image_size, self.patch_size, in_channels=self.in_channels,
                                    dropout_rate=self.dropout_rate, embed_method=self.embed_method,
                                    use_class_token=False)
        self.n_patches = self.proj.n_patches
        self.n_features = self.proj.true_n_features

    def _stack(self, args: Dict[str, Any]) -> TransformerBlockStack:
        return TransformerBlockStack(
            number_of_blocks=args["number_of_blocks"], input_dim_primary=self.n_features,
            attention_dim=self.n_features, hidden_dim=args["hidden_dim"], n_heads=args["n_heads"],
            mlp_structure=args["mlp_structure"], dropout_rate=args.get("dropout_rate", 0.0))

    def init_encoder(self):
        self.encoder = self._stack(self.encoder_args)

    def init_positional_embedding(self):
        """The positional embedding IS the embedding of the patching layer (one Parameter)."""
        self.positional_embedding = self.proj.positional_embedding

    def init_decoder(self):
        self.decoder = self._stack(self.decoder_args)

    def init_decoder_pred(self):
        dps = int(self.decoder_pred_ratio * self.n_features)
        self.decoder_pred = torch.nn.Sequential(
            Linear(self.n_features, dps), GELU(),
            Linear(dps, int(np.prod(self.patch_size)) * self.in_channels))

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        X = self.proj(X)
        X = HF.add_bcast(self.encoder(X)[0], self.positional_embedding)
        X = self.decoder(X)[0]
        return self.decoder_pred(X)


class ViTMaskedAutoEncoder(ViTAutoEncoder):
    """A ViT masked autoencoder (2-D images)."""

    def __init__(self, image_size, patch_size, in_channels: int, input_dim_size: int,
                 encoder_args: Dict[str, Any], decoder_args: Dict[str, Any],
                 embed_method: str = "linear", dropout_rate: float = 0.0,
                 decoder_pred_ratio: float = 4.0, mask_fraction: float = 0.3, seed: int = 42):
        if len(image_size) != 2 or len(patch_size) != 2:
            raise ValueError("ViTMaskedAutoEncoder takes 2-D images (its forward unpacks batch, "
                             f"channels, height, width); got image_size {list(image_size)} and "
                             f"patch_size {list(patch_size)}")
        super().__init__(image_size=image_size, patch_size=patch_size, in_channels=in_channels,
                         input_dim_size=input_dim_size, encoder_args=encoder_args,
                         decoder_args=decoder_args, embed_method=embed_method,
                         dropout_rate=dropout_rate, decoder_pred_ratio=decoder_pred_ratio)
        self.mask_fraction = mask_fraction
        self.seed = seed
        if int(self.n_patches * (1 - self.mask_fraction)) < 1:
            raise ValueError(f"mask_fraction {self.mask_fraction} keeps int({self.n_patches} * (1 - "
                             f"{self.mask_fraction})) = 0 of {self.n_patches} tokens: the encoder "
                             "would run on an empty sequence")
        self.init_mask_token()
        self.rng = np.random.default_rng(self.seed)

    def init_mask_token(self):
        self.mask_token_scale = torch.nn.Parameter(torch.ones(1))
        self.mask_token = torch.nn.Parameter(torch.randn(1, 1, self.n_features) * 0.02)

    @property
    def patch_elems(self) -> int:
        return int(np.prod(self.patch_size))

    def forward_tokens(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(pred [B, L, prod(patch_size) * in_channels], mask [B, L])``: the forward without the
        copy into the image layout."""
        batch_size, _, height, width = X.shape
        X_embed = self.proj(X)                                      # [B, L, E], positions included
        shuffle = _shuffle(X_embed.shape[0], X_embed.shape[1], self.mask_fraction, self.rng,
                           X_embed.device)
        X_encoded = self.encoder(HF.mae_keep_tokens(X_embed, shuffle))[0]     # [B, K, E]
        X_unshuffled = HF.mae_restore_tokens(X_encoded, self.mask_token, self.mask_token_scale,
                                             self.positional_embedding, shuffle)
        X_decoded = self.decoder(X_unshuffled)[0]
        return self.decoder_pred(X_decoded), shuffle.mask

    def forward(self, X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(reconstruction [B, C, H, W], mask [B, L])`` as the reference returns them."""
        pred, mask = self.forward_tokens(X)
        return HF.mae_to_image(pred, (pred.shape[0], self.in_channels, *X.shape[2:])), mask
