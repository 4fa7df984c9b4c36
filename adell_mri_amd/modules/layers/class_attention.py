"""``EfficientConditioningAttentionBlock`` (mirror of adell_mri/modules/layers/class_attention.py):
a conditioning vector is mapped to one sigmoid gate per channel of an activation. Constructor
arguments, attribute names and ``state_dict`` keys (``class_to_channels.*``, ``op.1.*``, ``op.2.*``,
``op.4.*``) are the reference's.

``op_type="linear"`` (what ``DiffusionUNet`` builds) runs on the device: the gate logits come from
``functional.eca_gates`` (one launch; a network asks for all of its sites at once) and
``functional.eca_apply`` multiplies the activation by their sigmoid in one launch. The ``torch.nn``
children hold the parameters and are never called. ``op_type="conv"``, the class default that
``DiffusionUNet`` never uses, raises ``NotImplementedError`` at construction."""
from typing import Union

import torch

from ... import functional as HF


class EfficientConditioningAttentionBlock(torch.nn.Module):
    def __init__(self, class_dimension: int, input_channels: int, gamma: float = 2, b: float = 1,
                 op_type: str = "conv"):
        super().__init__()
        self.class_dimension = class_dimension
        self.input_channels = input_channels
        self.gamma = gamma
        self.b = b
        self.op_type = op_type

        self.initialize_layers()

    def odd(self, i: Union[int, float]) -> int:
        i = int(i)
        if i % 2 == 0:
            i = i + 1
        return i

    def initialize_layers(self):
        if self.op_type == "conv":
            raise NotImplementedError(
                'EfficientConditioningAttentionBlock(op_type="conv") is outside the HIP path: '
                'DiffusionUNet builds op_type="linear"')
        if self.op_type != "linear":
            return      # as the reference: no ``op``; forward has nothing to run
        self.class_to_channels = torch.nn.Linear(self.class_dimension, self.input_channels)
        self.op = torch.nn.Sequential(
            torch.nn.SiLU(),
            torch.nn.Linear(self.input_channels, self.input_channels),
            torch.nn.LayerNorm(self.input_channels),
            torch.nn.SiLU(),
            torch.nn.Linear(self.input_channels, self.input_channels),
        )

    def forward(self, X: torch.Tensor, cls: torch.Tensor) -> torch.Tensor:
        """``X`` [B, C, *spatial] times the gates of the conditioning vectors ``cls`` ([G, 1,
        class_dimension] or [G, class_dimension], G in {1, B})."""
        z = HF.eca_gates(None, [self], cls.reshape(-1, self.class_dimension))[0]
        return HF.eca_apply(X, z)
