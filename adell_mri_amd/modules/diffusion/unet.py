"""``DiffusionUNet`` and ``get_timestep_embedding`` (mirror of adell_mri/modules/diffusion/unet.py):
the package's ``UNet`` with one timestep-conditioned channel gate
(``EfficientConditioningAttentionBlock``, ``op_type="linear"``) after every encoder level, link op and
decoder level -- ``3 L - 2`` sites for ``L`` levels -- and a head without sigmoid or softmax that
predicts the noise.

Mirrored as written: ``in_channels`` is required, ``n_classes = in_channels``,
``encoding_operations``, ``bottleneck_classification`` and ``feature_conditioning`` are forced off,
``embedding`` is ``None`` without guidance, the gate lists are ``encoder_eca``, ``decoder_eca``,
``link_eca``, the final layer is ``Sequential(conv 3, adn, conv 1 -> in_channels)``, ``cls`` without
guidance raises the reference's ``Exception``, and ``forward(X, t, cls=None)`` returns the raw head, or
``(head, deep_outputs)`` under deep supervision.

Underneath: the gate logits of all sites of a forward come from ONE ``functional.eca_gates`` launch in
front of the encoder loop (they all read the same embedding), and every gate is one
``functional.eca_apply`` launch on the channels-last activation the conv kernels leave. The forward
takes the plain route through the conv layers (no gradient carries, no split rows): a gated tensor is
a new value with more than one reader. The class embedding is a ``torch.nn.Embedding`` lookup of B
rows."""
import math

import numpy as np
import torch

from ... import functional as HF
from ..._lib import AdellHipError
from ..layers.class_attention import EfficientConditioningAttentionBlock
from ..layers.utils import crop_to_size
from ..segmentation.unet import UNet, _cat_channels, _DecoderOp


def get_timestep_embedding(t: torch.Tensor, channels: int, max_period: int = 10000) -> torch.Tensor:
    """The reference's sinusoidal embedding in torch ops, as written (fp32): ``t`` [G] -> [G,
    channels], cos half then sin half, zero pad for an odd ``channels``. The networks here do not
    call it: ``functional.eca_gates`` evaluates the same embedding inside its kernel."""
    exponent = -math.log(max_period) * torch.arange(start=0, end=channels // 2, dtype=torch.float32,
                                                    device=t.device)
    freqs = torch.exp(exponent / (channels // 2))

    args = t[:, None].float() * freqs[None, :]
    embedding = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)

    # zero pad
    if channels % 2 == 1:
        embedding = torch.nn.functional.pad(embedding, (0, 1, 0, 0))

    return embedding


def _plain_final(layer, X):
    """A deep-supervision head of ``UNet`` (conv, adn, conv, Sigmoid | Softmax) module by module, its
    last activation on the device kernels."""
    mods = list(layer)
    for mod in mods[:-1]:
        X = mod(X)
    if isinstance(mods[-1], torch.nn.Sigmoid):
        if X.dim() == 4:
            return HF.norm_drop_act(X.unsqueeze(2), act="sigmoid").squeeze(2)
        return HF.norm_drop_act(X, act="sigmoid")
    return HF.channel_softmax(X)


class DiffusionUNet(UNet):
    """U-Net for diffusion models."""

    def __init__(self, t_dim: int = 256, classifier_free_guidance: bool = False,
                 classifier_classes: int = 2, *args, **kwargs):
        if "in_channels" not in kwargs:
            raise Exception("in_channels must be defined")
        kwargs["n_classes"] = kwargs["in_channels"]
        kwargs["encoding_operations"] = None
        kwargs["bottleneck_classification"] = False
        kwargs["feature_conditioning"] = None
        super().__init__(*args, **kwargs)

        self.t_dim = t_dim
        self.classifier_free_guidance = classifier_free_guidance
        self.classifier_classes = classifier_classes

        self.init_eca()

    def init_eca(self):
        eca_op = EfficientConditioningAttentionBlock
        if self.classifier_free_guidance is True:
            # use this to map classes to self.t_dim vectors
            self.embedding = torch.nn.Embedding(self.classifier_classes, self.t_dim)
        else:
            self.embedding = None
        self.encoder_eca = torch.nn.ModuleList(
            [eca_op(self.t_dim, d, op_type="linear") for d in self.depth])
        self.decoder_eca = torch.nn.ModuleList(
            [eca_op(self.t_dim, d, op_type="linear") for d in self.depth[:-1][::-1]])
        self.link_eca = torch.nn.ModuleList(
            [eca_op(self.t_dim, d, op_type="linear") for d in self.depth[:-1][::-1]])

    def get_final_layer(self, d: int) -> torch.nn.Module:
        """conv 3 -> adn -> conv 1 back to ``in_channels``; no sigmoid, no softmax."""
        return torch.nn.Sequential(self._conv(d, d, 3, padding=1), self.adn_fn(d),
                                   self._conv(d, self.in_channels, 1))

    def forward(self, X: torch.Tensor, t: torch.Tensor, cls: torch.Tensor = None) -> torch.Tensor:
        """``X`` [B, in_channels, *spatial]; ``t`` [G] or [G, 1] with G in {1, B}, the timestep as a
        fraction (what ``Diffusion`` passes) or an integer; ``cls`` [B] class indices for guidance."""
        if cls is not None and self.classifier_free_guidance is False:
            raise Exception(
                "cls can only be defined if classifier_free_guidance is \
                        True in the constructor"
            )
        if not X.is_cuda:
            raise AdellHipError("adell_mri_amd.DiffusionUNet runs on MI355X only (no CPU fallback)")
        HF.clear_row_expectations()
        t = t.to(X.device)
        cls_embedding = None
        if cls is not None:
            cls_embedding = self.embedding(cls.long())
        # every gate of this forward reads the same embedding: one launch for all of them
        n_enc, n_dec = len(self.encoder_eca), len(self.decoder_eca)
        gates = HF.eca_gates(t, [*self.encoder_eca, *self.link_eca, *self.decoder_eca], cls_embedding)
        enc_gates, link_gates = gates[:n_enc], gates[n_enc:n_enc + n_dec]
        dec_gates = gates[n_enc + n_dec:]

        encoding_out = []
        curr = X
        for (op, op_ds), z in zip(self.encoding_operations, enc_gates):
            curr = op(curr)
            curr = HF.eca_apply(curr, z)
            encoding_out.append(curr)
            curr = op_ds(curr)

        deep_outputs = []
        for i in range(len(self.decoding_operations)):
            op = self.decoding_operations[i]
            link_op = self.link_ops[i]
            up = self.upscale_ops[i]
            link_op_input = encoding_out[-i - 2]
            encoded = HF.eca_apply(link_op(link_op_input), link_gates[i])
            curr = up(curr)
            sh = list(curr.shape)[2:]
            sh2 = list(encoded.shape)[2:]
            if np.prod(sh) < np.prod(sh2):
                encoded = crop_to_size(encoded, sh)
            if np.prod(sh) > np.prod(sh2):
                curr = crop_to_size(curr, sh2)
            # the concat is virtual: the decoder's first conv reads both tensors
            if isinstance(op, _DecoderOp):
                curr = op(curr, X_cat=encoded)
            else:
                curr = op(_cat_channels(curr, encoded))
            curr = HF.eca_apply(curr, dec_gates[i])
            deep_outputs.append(curr)

        curr = self.final_layer(curr)

        if self.deep_supervision is True:
            for i in range(len(deep_outputs)):
                deep_outputs[i] = _plain_final(self.deep_supervision_ops[i], deep_outputs[i])
            return curr, deep_outputs

        return curr
