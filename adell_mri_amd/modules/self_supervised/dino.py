"""DINO network on the HIP kernels (mirror of adell_mri/modules/self_supervised/dino.py): a ``ViT``
encoder, an ``MLP`` projection, an L2 normalisation and a weight-normalised bias-free Linear onto
``out_dim`` prototypes. State keys are the reference's: ``encoder_.*``, ``projection_.op.N.*`` and
``last_layer_.parametrizations.weight.original0`` / ``.original1``.

Kept as written: ``forward_encoder`` drops the registers, then takes token 0 with a class token and
otherwise ``out.mean(-1)`` -- the mean over the FEATURE axis, [B, tokens] -- while the projection
reads ``attention_dim`` inputs. Without a class token the reference's forward therefore runs only
when the number of tokens equals ``attention_dim`` (its own test configuration does: 32 x 32, patch
4, 64 wide); any other such configuration fails there with a shape error and raises
``NotImplementedError`` here, at construction.
"""
from typing import Any, Dict

import numpy as np
import torch

from ... import functional as HF
from ..layers.linear_blocks import MLP, WeightNormLinear
from ..layers.vit import ViT


class DINO(torch.nn.Module):
    def __init__(self, backbone_args: Dict[str, Any], projection_head_args: Dict[str, Any],
                 out_dim: int):
        super().__init__()
        self.backbone_args = backbone_args
        self.projection_head_args = projection_head_args
        self.out_dim = out_dim
        self._check_pooling()
        self.initialize_encoder()
        self.initialize_projection()
        self.initialize_last_layer()

    def _check_pooling(self):
        args = self.backbone_args
        if args.get("use_class_token", False) is True:
            return
        tokens = int(np.prod([int(s) // int(p) for s, p in zip(args["image_size"],
                                                               args["patch_size"])]))
        if args.get("channel_to_token", False):
            tokens *= int(args["in_channels"])
        if tokens != args["attention_dim"]:
            raise NotImplementedError(
                f"DINO without a class token pools with out.mean(-1), the mean over the feature "
                f"axis, and feeds the [B, {tokens}] result to a projection of attention_dim = "
                f"{args['attention_dim']} inputs: the reference's forward fails with a shape error "
                f"unless the two are equal (set use_class_token=True)")

    def forward_encoder(self, X: torch.Tensor) -> torch.Tensor:
        out = self.encoder_(X)[0]
        if self.encoder_.n_registers > 0:
            out = out[:, self.encoder_.n_registers:]
        if self.encoder_.use_class_token is True:
            return out[:, 0]
        return HF.row_mean(out)

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

    def forward(self, X: torch.Tensor) -> torch.Tensor:
        return self.last_layer_(HF.l2_normalize(self.projection_(self.forward_encoder(X))))

    def forward_representation(self, X: torch.Tensor) -> torch.Tensor:
        return self.forward_encoder(X)
