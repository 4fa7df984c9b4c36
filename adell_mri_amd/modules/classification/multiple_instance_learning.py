"""Multiple-instance classifiers on the HIP kernels (mirror of
adell_mri/modules/classification/classification/multiple_instance_learning.py): ``MILAttention``
(:12-43), ``MultipleInstanceClassifier`` (:46-261) and ``TransformableTransformer`` (:264-482). A 2-D
``module`` runs on every slice of a volume [B, C, H, W, S]; the volume is classified from the stack of
slice vectors [B, S, V].

Constructor arguments, defaults, attribute names and ``state_dict`` keys are the reference's (``V``,
``U``, ``W``; ``module.*``, ``feature_extraction.*``, ``vocabulary_prediction.*``,
``final_prediction.*``, ``attention_op.*``, ``positional_embedding``; ``input_layer.*``, ``tbs.*``,
``classification_module.*``, ``class_token``), so its checkpoints load. On the kernels of
csrc/mil.hip: the slicing (``functional.volume_to_slices``), the gated-attention pooling
(``functional.mil_gated_pool``: attention, softmax over the slices and the pooling in one launch)
and the token rows of the slice transformer (``functional.slice_tokens``).

Mirrored as written:

* The slices are always taken along the LAST axis. ``dim`` is stored and asserted to be in
  {0, 1, 2}; only the reference's dead ``v_module_old`` reads it, which is not built.
* ``MultipleInstanceClassifier.v_module`` runs under ``no_grad``; ``TransformableTransformer``'s
  does not, so its module may train.
* ``extract_features`` flattens what lies behind the channel axis and reduces the last axis. For a
  module that already returns [B * S, V] the reference reduces over V itself, and its
  ``"(b s) v -> b s v"`` then cannot take the vector: here ``extract_features`` does the same and
  ``v_module`` raises a ``ValueError`` that names ``module``.

Raised on the host before any kernel, where the reference fails late or not at all: ``n_slices=None``
(its ``Rearrange(..., s=None)`` fails in the first forward with a ``TypeError``), a volume whose last
axis is not ``n_slices``, and a ``reduce_fn`` other than "mean" / "max" (the reference returns None).
"""
from typing import Callable, List

import torch

from ... import functional as HF
from ..layers.adn_fn import get_adn_fn
from ..layers.linear_blocks import MLP, LayerNorm, Linear
from ..layers.vit import TransformerBlockStack
from ..self_supervised.autoencoders import GELU


def _check_arguments(n_slices, reduce_fn):
    if n_slices is None or int(n_slices) != n_slices or int(n_slices) < 1:
        raise ValueError(f"n_slices must be the number of slices of the volumes (a positive "
                         f"integer), got {n_slices!r}: the slice vectors are regrouped per volume "
                         f"by it")
    if reduce_fn not in ("mean", "max"):
        raise ValueError(f"reduce_fn must be 'mean' or 'max', got {reduce_fn!r}")


def _extract_features(X: torch.Tensor, reduce_fn: str) -> torch.Tensor:
    """``X.flatten(start_dim=2)`` then the mean or the maximum over the last axis: [N, V, *spatial]
    -> [N, V]; a 2-D [N, V] is reduced over V itself, as in the reference."""
    if X.dim() <= 2:
        if reduce_fn == "mean":
            return HF.row_mean(X)
        rows = X.reshape(1, -1, 1, 1, X.shape[-1])      # [N, V] as one item of N channels
        return HF.channel_max(rows).reshape(X.shape[:-1])
    while X.dim() < 5:
        X = X.unsqueeze(2)
    if X.dim() > 5:
        X = X.flatten(start_dim=4)
    return HF.channel_mean(X) if reduce_fn == "mean" else HF.channel_max(X)


def _slice_vectors(self, X: torch.Tensor) -> torch.Tensor:
    """[B, C, H, W, S] -> [B, S, V]: the module on every slice, its output reduced."""
    if X.dim() != 5 or X.shape[-1] != self.n_slices:
        raise ValueError(f"X must be a volume [B, C, H, W, n_slices={self.n_slices}], got "
                         f"{tuple(X.shape)}")
    B = X.shape[0]
    X = HF.volume_to_slices(X)
    X = self.module(X)
    X = self.extract_features(X)
    if X.dim() != 2:
        raise ValueError(f"module must return [B * S, V, *spatial] for its slices: a "
                         f"{X.dim() + 1}-D output leaves {tuple(X.shape)} after extract_features, "
                         f"which cannot be regrouped as [B, S, V]")
    return X.reshape(B, self.n_slices, X.shape[-1])


class MILAttention(torch.nn.Module):
    """Gated attention for multiple-instance learning (:12-43, arXiv 1802.04712):
    ``A = softmax(W(tanh(V x) * sigmoid(U x)))`` over ``along_dim`` (-2: the instances)."""

    def __init__(self, n_dim: int, along_dim=-2):
        super().__init__()
        self.n_dim = n_dim
        self.along_dim = along_dim
        self.initialize_layers()

    def initialize_layers(self):
        self.V = Linear(self.n_dim, self.n_dim)
        self.U = Linear(self.n_dim, self.n_dim)
        self.W = Linear(self.n_dim, 1)

    def gate_inputs(self, X: torch.Tensor):
        """(V x, U x, the row of W, its bias): what ``functional.mil_gated_pool`` takes."""
        if X.dim() != 3 or self.along_dim not in (-2, 1):
            raise ValueError(f"MILAttention: X [B, S, n_dim] with along_dim=-2 expected, got "
                             f"{tuple(X.shape)} and along_dim={self.along_dim}")
        return self.V(X), self.U(X), self.W.weight, self.W.bias

    def calculate_attention(self, X: torch.Tensor) -> torch.Tensor:
        return HF.mil_attention(*self.gate_inputs(X))

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        attention = self.calculate_attention(X)
        return HF.scale_per_item_channel(X, attention.squeeze(-1))


class MultipleInstanceClassifier(torch.nn.Module):
    """Multiple-instance classifier for volumes (:46-261): slice vectors from ``module`` (under
    ``no_grad``), plus one positional scalar per slice, a feature MLP per slice, and a pooling over
    the slices weighted by A (the gated attention, or 1 / S): ``classification_mode`` "mean" (sum of
    feat A), "max" (maximum of feat A) or "vocabulary" (the mean composition of ``vocabulary_size``
    soft proxy classes); then an MLP. One logit for two classes."""

    def __init__(self, module: torch.nn.Module, module_out_dim: int, n_classes: int,
                 feat_extraction_structure: List[int], classification_structure: List[int],
                 adn_fn: Callable = get_adn_fn(1, "layer", "gelu", 0.1),
                 classification_adn_fn: Callable = get_adn_fn(1, "layer", "gelu", 0.1),
                 classification_mode: str = "mean", vocabulary_size: int = 10, n_slices: int = None,
                 use_positional_embedding: bool = True, dim: int = 2, attention: bool = False,
                 reduce_fn: str = "mean"):
        assert dim in [0, 1, 2], "dim must be one of [0,1,2]"
        assert classification_mode in ["mean", "max", "vocabulary"], \
            'classification has to be one of ["mean","max","vocabulary"]'
        _check_arguments(n_slices, reduce_fn)
        super().__init__()
        self.module = module
        self.module_out_dim = module_out_dim
        self.n_classes = n_classes
        self.feat_extraction_structure = feat_extraction_structure
        self.adn_fn = adn_fn
        self.classification_structure = classification_structure
        self.classification_adn_fn = classification_adn_fn
        self.classification_mode = classification_mode
        self.vocabulary_size = vocabulary_size
        self.n_slices = n_slices
        self.use_positional_embedding = use_positional_embedding
        self.dim = dim
        self.attention = attention
        self.reduce_fn = reduce_fn

        self.init_classification_module()
        self.init_positional_embedding()
        if self.attention is True:
            self.attention_op = MILAttention(self.module_out_dim)

    def init_positional_embedding(self):
        self.positional_embedding = None
        if self.n_slices is not None and self.use_positional_embedding is True:
            self.positional_embedding = torch.nn.Parameter(torch.zeros([1, self.n_slices, 1]))
            torch.nn.init.trunc_normal_(self.positional_embedding, mean=0.0, std=0.02, a=-2.0, b=2.0)

    def extract_features(self, X: torch.Tensor) -> torch.Tensor:
        return _extract_features(X, self.reduce_fn)

    @torch.no_grad()
    def v_module(self, X: torch.Tensor) -> torch.Tensor:
        return _slice_vectors(self, X)

    def init_classification_module(self):
        n_classes_out = 1 if self.n_classes == 2 else self.n_classes
        if len(self.feat_extraction_structure) > 0:
            self.feature_extraction = torch.nn.Sequential(
                LayerNorm(self.module_out_dim),
                MLP(self.module_out_dim, self.feat_extraction_structure[-1],
                    structure=self.feat_extraction_structure[:-1], adn_fn=self.adn_fn),
                LayerNorm(self.feat_extraction_structure[-1]),
                GELU())
            last_layer_value = self.feat_extraction_structure[-1]
        else:
            self.feature_extraction = torch.nn.Sequential(LayerNorm(self.module_out_dim), GELU())
            last_layer_value = self.module_out_dim
        if self.classification_mode in ["mean", "max"]:
            self.final_prediction = MLP(last_layer_value, n_classes_out,
                                        structure=self.classification_structure,
                                        adn_fn=self.classification_adn_fn)
        elif self.classification_mode == "vocabulary":
            self.vocabulary_prediction = MLP(last_layer_value, self.vocabulary_size, structure=[],
                                             adn_fn=self.classification_adn_fn)
            self.final_prediction = MLP(self.vocabulary_size, n_classes_out,
                                        structure=self.classification_structure,
                                        adn_fn=self.classification_adn_fn)

    def get_prediction(self, X: torch.Tensor):
        """(logits, A [B, S, 1]) from the slice vectors X [B, S, V]: attention, softmax over the
        slices and the pooling are one launch."""
        gate = self.attention_op.gate_inputs(X) if self.attention is True else ()
        out = self.feature_extraction(X)
        if self.classification_mode == "vocabulary":
            out = self.vocabulary_prediction(out)
        pooled, A = HF.mil_gated_pool(out, *gate, mode=self.classification_mode)
        return self.final_prediction(pooled), A

    def forward(self, X: torch.Tensor, return_attention: bool = False) -> torch.Tensor:
        ssl_representation = self.v_module(X)
        if self.positional_embedding is not None:
            ssl_representation = HF.slice_tokens(ssl_representation, self.positional_embedding)
        output, attention = self.get_prediction(ssl_representation)
        if return_attention is True:
            return output, attention
        return output


class TransformableTransformer(torch.nn.Module):
    """A transformer over the slice vectors of a volume (:264-482): ``module`` on every slice
    (gradients flow into it), ``input_layer`` (layer norm, or layer norm - Linear - layer norm when
    ``input_dim`` differs), one positional scalar per slice and a class token in front, a
    ``TransformerBlockStack`` (its arguments through ``*args, **kwargs``), then the class token or the
    mean over the tokens through layer norm, GELU and an MLP. ``return_attention=True`` also returns
    what the last block's attention produced."""

    def __init__(self, module: torch.nn.Module, module_out_dim: int, n_classes: int,
                 classification_structure: List[int], input_dim: int = None,
                 classification_adn_fn: Callable = get_adn_fn(1, "layer", "gelu", 0.1),
                 n_slices: int = None, use_positional_embedding: bool = True, dim: int = 2,
                 use_class_token: bool = True, reduce_fn: str = "mean", *args, **kwargs):
        assert dim in [0, 1, 2], "dim must be one of [0,1,2]"
        _check_arguments(n_slices, reduce_fn)
        super().__init__()
        self.module = module
        self.module_out_dim = module_out_dim
        self.n_classes = n_classes
        self.classification_structure = classification_structure
        self.input_dim = input_dim
        self.classification_adn_fn = classification_adn_fn
        self.n_slices = n_slices
        self.use_positional_embedding = use_positional_embedding
        self.dim = dim
        self.use_class_token = use_class_token
        self.reduce_fn = reduce_fn

        if input_dim is not None:
            self.transformer_input_dim = input_dim
            self.input_layer = torch.nn.Sequential(LayerNorm(module_out_dim),
                                                   Linear(module_out_dim, input_dim),
                                                   LayerNorm(input_dim))
        else:
            self.transformer_input_dim = module_out_dim
            self.input_layer = LayerNorm(module_out_dim)

        kwargs["input_dim_primary"] = self.transformer_input_dim
        kwargs["attention_dim"] = self.transformer_input_dim
        kwargs["hidden_dim"] = self.transformer_input_dim
        self.tbs = TransformerBlockStack(*args, **kwargs)
        self.classification_module = torch.nn.Sequential(
            LayerNorm(self.transformer_input_dim),
            GELU(),
            MLP(self.transformer_input_dim, 1 if self.n_classes == 2 else self.n_classes,
                structure=self.classification_structure, adn_fn=self.classification_adn_fn))
        self.initialize_classification_token()
        self.init_positional_embedding()

    def initialize_classification_token(self):
        if self.use_class_token is True:
            self.class_token = torch.nn.Parameter(torch.zeros([1, 1, self.transformer_input_dim]))

    def init_positional_embedding(self):
        self.positional_embedding = None
        if self.n_slices is not None and self.use_positional_embedding is True:
            self.positional_embedding = torch.nn.Parameter(torch.zeros([1, self.n_slices, 1]))
            torch.nn.init.trunc_normal_(self.positional_embedding, mean=0.0, std=0.02, a=-2.0, b=2.0)

    def extract_features(self, X: torch.Tensor) -> torch.Tensor:
        return _extract_features(X, self.reduce_fn)

    def v_module(self, X: torch.Tensor) -> torch.Tensor:
        return _slice_vectors(self, X)

    def forward(self, X: torch.Tensor, return_attention: bool = False) -> torch.Tensor:
        ssl_representation = self.v_module(X)
        ssl_representation = self.input_layer(ssl_representation)
        class_token = self.class_token if self.use_class_token is True else None
        if self.positional_embedding is not None or class_token is not None:
            ssl_representation = HF.slice_tokens(ssl_representation, self.positional_embedding,
                                                 class_token)
        transformer_output = self.tbs(ssl_representation, return_attention=return_attention)
        if return_attention is True:
            attention = transformer_output[-1][0]
        transformer_output = transformer_output[0]
        if self.use_class_token is True:
            transformer_output = transformer_output[:, 0, :].contiguous()
        else:
            transformer_output = HF.token_mean(transformer_output)
        output = self.classification_module(transformer_output)
        if return_attention is True:
            return output, attention
        return output
