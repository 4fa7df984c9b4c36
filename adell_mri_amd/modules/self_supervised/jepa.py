"""I-JEPA network on the HIP kernels (mirror of adell_mri/modules/self_supervised/jepa.py): a
student ``ViT`` that encodes only the tokens of a few context blocks, a small transformer predictor
that fills in learnable mask tokens at the positions of each target block, and as target the
layer-normalised features of an EMA teacher that saw the whole image. State keys are the
reference's, in its order: ``encoder_.*``, then ``predictor_.predictor_pos_embed_``,
``predictor_.mask_token_``, ``predictor_.predictor_embed_.*``, ``predictor_.predictor_.*`` and
``predictor_.predictor_proj_.weight`` (the masker holds no parameters).

Kept as written:
  * every ``forward_training`` draws ``n_patches`` context blocks, then ``n_masked_patches`` target
    blocks from the one masker rng -- validation included; the context is ``np.unique`` of its
    blocks, each target is ``np.setdiff1d`` against the context, and empty targets are dropped;
  * the student runs the encoder's blocks on the context tokens only (no class token, no
    registers: ``embedded[:, skip_n:][:, context_idx]``);
  * the teacher is ``getattr(teacher_model, "shadow", teacher_model).encoder_`` (the module itself
    without a teacher), run under ``no_grad`` on the full input;
  * ``reduce_fn`` is stored and unused.

What differs, in how it is computed and not in what:
  * the indexing, ``cat`` and ``expand`` are row kernels (csrc/ijepa.hip): ``functional.gather_tokens``
    with the ``skip_n`` offset folded into the row table, ``functional.predictor_tokens`` for the
    predictor's input;
  * ``predictor_embed_(context)`` is the same for every target block, so ``forward_training``
    computes it ONCE and autograd sums the blocks' gradients; the reference recomputes it per block
    with the same value (``IJEPAPredictor.forward`` alone still computes it itself);
  * ``forward_blocks`` returns the predictions with the teacher's RAW output and the target row
    tables, from which ``functional.ijepa_block_loss`` takes the loss without writing the normalised
    features; ``forward_training`` builds the reference's ``(predictions, targets)`` from it.
If every target block is dropped the reference fails in ``torch.stack([])`` with a RuntimeError;
here ``RuntimeError`` is raised on the host, before any kernel runs.
"""
from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from ... import functional as HF
from ...utils.masking import get_masker
from ..layers.linear_blocks import Linear
from ..layers.vit import TransformerBlockStack, ViT

TensorList = List[torch.Tensor]
IJEPAOut = Tuple[TensorList, TensorList]


class IJEPAPredictor(torch.nn.Module):
    """Context tokens [B, nc, encoder_dim] -> predictions [B, nt, encoder_dim] for one target block:
    a Linear onto ``predictor_dim``, the positional embedding of the context rows, one mask token
    plus its positional embedding per target row appended, a ``TransformerBlockStack``
    (``input_dim_primary`` overridden by ``predictor_dim``), and a bias-free Linear back on the
    appended rows."""

    def __init__(self, encoder_dim: int, predictor_dim: int, block_stack_args: Dict[str, Any],
                 n_tokens: int):
        super().__init__()
        self.encoder_dim = encoder_dim
        self.predictor_dim = predictor_dim
        self.n_tokens = n_tokens
        self.predictor_embed_ = Linear(encoder_dim, predictor_dim, bias=True)
        self.predictor_pos_embed_ = torch.nn.Parameter(torch.rand(1, n_tokens, predictor_dim))
        self.mask_token_ = torch.nn.Parameter(torch.rand(1, 1, predictor_dim))
        block_stack_args = dict(block_stack_args)
        block_stack_args["input_dim_primary"] = predictor_dim
        self.predictor_ = TransformerBlockStack(**block_stack_args)
        self.predictor_proj_ = Linear(predictor_dim, encoder_dim, bias=False)

    def predict(self, embedded: torch.Tensor, context_idx, target_idx) -> torch.Tensor:
        """The predictor from the embedded context [B, nc, predictor_dim] on."""
        n_context, n_target = embedded.shape[1], len(target_idx)
        x = HF.predictor_tokens(embedded, self.predictor_pos_embed_, self.mask_token_, context_idx,
                                target_idx)
        x, _ = self.predictor_(x)
        # x[:, -n_target:] as a row gather: the slice is not dense
        tail = np.arange(n_context, n_context + n_target)
        return self.predictor_proj_(HF.gather_tokens(x, tail))

    def forward(self, context: torch.Tensor, context_idx: np.ndarray,
                target_idx: np.ndarray) -> torch.Tensor:
        return self.predict(self.predictor_embed_(context), context_idx, target_idx)


class IJEPA(torch.nn.Module):
    def __init__(self, backbone_args: Dict[str, Any], projection_head_args: Dict[str, Any],
                 feature_map_dimensions: List[int], n_encoder_features: int,
                 min_patch_size: List[int], max_patch_size: List[int], n_patches: int = 1,
                 n_masked_patches: int = 4, predictor_dim: Optional[int] = None,
                 encoder_architecture: str = "vit", predictor_architecture: str = "vit",
                 reduce_fn: str = "mean", seed: int = 42):
        super().__init__()
        self.backbone_args = backbone_args
        self.projection_head_args = projection_head_args
        self.feature_map_dimensions = feature_map_dimensions
        self.n_encoder_features = n_encoder_features
        self.min_patch_size = min_patch_size
        self.max_patch_size = max_patch_size
        self.n_patches = n_patches
        self.n_masked_patches = n_masked_patches
        self.predictor_dim = predictor_dim
        self.encoder_architecture = encoder_architecture
        self.predictor_architecture = predictor_architecture
        self.reduce_fn = reduce_fn
        self.seed = seed

        assert self.encoder_architecture == "vit", \
            "only 'vit' is supported as encoder architecture for I-JEPA"
        assert self.predictor_architecture == "vit", \
            "only 'vit' is supported as predictor architecture for I-JEPA"

        self.initialize_masker()
        self.initialize_encoder()
        self.initialize_predictor()

    @property
    def extra_tokens(self) -> int:
        """Class token and registers the embedding puts in front of the patch tokens."""
        return self.encoder_.n_registers + int(self.encoder_.use_class_token)

    def initialize_masker(self):
        self.patch_masker_ = get_masker(
            model_type="generic_transformer", image_dimensions=self.feature_map_dimensions,
            min_patch_size=self.min_patch_size, max_patch_size=self.max_patch_size,
            n_patches=self.n_patches, n_features=self.n_encoder_features, seed=self.seed)

    def initialize_encoder(self):
        self.encoder_ = ViT(**self.backbone_args)
        self.encoder_dim_ = self.encoder_.input_dim_primary

    def initialize_predictor(self):
        predictor_dim = self.predictor_dim if self.predictor_dim is not None else self.encoder_dim_
        n_tokens = int(np.prod(self.feature_map_dimensions))
        self.predictor_ = IJEPAPredictor(encoder_dim=self.encoder_dim_, predictor_dim=predictor_dim,
                                         block_stack_args=self.projection_head_args,
                                         n_tokens=n_tokens)

    def _get_teacher_encoder(self, teacher_model) -> torch.nn.Module:
        if teacher_model is None:
            teacher_model = self
        teacher = getattr(teacher_model, "shadow", teacher_model)
        return teacher.encoder_

    def _sample_mask_indices(self) -> Tuple[np.ndarray, List[np.ndarray]]:
        """(unique context token indices, one index array per target block that keeps a token
        outside the context)."""
        context_coords = self.patch_masker_.sample_patches(self.n_patches)
        context_idx = np.unique(np.concatenate(
            [self.patch_masker_.retrieve_patch(c) for c in context_coords])).astype(np.int64)
        target_coords = self.patch_masker_.sample_patches(self.n_masked_patches)
        target_idx = [np.setdiff1d(self.patch_masker_.retrieve_patch(c).astype(np.int64),
                                   context_idx) for c in target_coords]
        target_idx = [t for t in target_idx if len(t) > 0]
        return context_idx, target_idx

    def forward_blocks(self, X: torch.Tensor, teacher_model: torch.nn.Module = None):
        """(predictions, h, rows): one prediction [B, nt, E] per kept target block, the teacher's raw
        output h [B, skip_n + T, E] and per block the rows of h its target is read from (the
        block's token indices ``+ skip_n``)."""
        context_idx, target_idx = self._sample_mask_indices()
        if len(target_idx) == 0:
            raise RuntimeError(
                f"I-JEPA: all {self.n_masked_patches} target blocks lie inside the "
                f"{len(context_idx)} context tokens of this draw, so there is nothing to predict "
                "(the reference fails here in torch.stack of an empty list)")
        embedded = self.encoder_.embedding(X)
        skip_n = self.extra_tokens
        # student: the context tokens only
        context = HF.gather_tokens(embedded, context_idx + skip_n)
        for block in self.encoder_.tbs.transformer_blocks:
            context = block(context)
        e = self.predictor_.predictor_embed_(context)     # once for every target block
        predictions = [self.predictor_.predict(e, context_idx, t_idx) for t_idx in target_idx]
        teacher_encoder = self._get_teacher_encoder(teacher_model)
        with torch.no_grad():
            h = teacher_encoder(X)[0].detach()
        return predictions, h, [t_idx + skip_n for t_idx in target_idx]

    def forward_training(self, X: torch.Tensor, teacher_model: torch.nn.Module = None) -> IJEPAOut:
        """``(predictions, targets)``, one tensor [B, nt, E] per kept target block each, as in the
        reference: the targets are the rows of the layer-normalised teacher output."""
        predictions, h, rows = self.forward_blocks(X, teacher_model)
        with torch.no_grad():
            h = HF.layer_norm(h)
            targets = [HF.gather_tokens(h, r).detach() for r in rows]
        return predictions, targets

    def forward(self, X: torch.Tensor) -> IJEPAOut:
        return self.forward_representation(X)

    def forward_representation(self, X: torch.Tensor) -> torch.Tensor:
        return self.encoder_(X)[0].permute(0, 2, 1)
