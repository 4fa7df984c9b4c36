"""What the multiple-instance tests share: the six fixture networks of tests/golden/mil_step_<net>.npz
(tools/make_mil_golden.py), how either side builds them, and a view of one network's records.

The 2-D module is a small ``ResNetBackbone`` (two stages, ``get_adn_fn(2, "batch", "swish", 0.0)``) in
``eval()`` mode: [B * S, 1, 16, 16] -> [B * S, 16, 2, 2]. Volumes are [4, 1, 16, 16, 8]. A frozen module
has ``requires_grad=False`` on every parameter; ``tt_mean_train`` leaves them trainable (still in
``eval()`` mode: batch norm uses its running statistics)."""
import os

import numpy as np

from classification_cases import STEP_EPS, STEP_LR, fill, step_groups, zero_dropout  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETS = ("mil_mean_att", "mil_max_att", "mil_vocab_att", "mil_mean_plain", "tt_cls", "tt_mean_train")
SHAPE = (4, 1, 16, 16, 8)
MODULE = dict(spatial_dim=2, in_channels=1, structure=[(8, 16, 3, 2), (16, 32, 3, 2)],
              maxpool_structure=[(2, 2), (2, 2)])
MODULE_OUT = 16

_MIL = dict(module_out_dim=MODULE_OUT, n_slices=SHAPE[-1], classification_structure=[16])
_TT = dict(module_out_dim=MODULE_OUT, n_slices=SHAPE[-1], classification_structure=[16], n_heads=2)
# name: (class, constructor arguments without ``module``, labels, weight decay of the step,
#        whether the module's parameters train)
CONFIGS = {
    "mil_mean_att": ("MultipleInstanceClassifier",
                     dict(_MIL, n_classes=2, feat_extraction_structure=[16, 16],
                          classification_mode="mean", attention=True), [0, 1, 1, 0], 0.05, False),
    "mil_max_att": ("MultipleInstanceClassifier",
                    dict(_MIL, n_classes=3, feat_extraction_structure=[16, 16],
                         classification_mode="max", attention=True), [0, 2, 1, 2], 0.05, False),
    "mil_vocab_att": ("MultipleInstanceClassifier",
                      dict(_MIL, n_classes=2, feat_extraction_structure=[16],
                           classification_mode="vocabulary", vocabulary_size=6, attention=True),
                      [0, 1, 1, 0], (0.05, 0.1), False),
    "mil_mean_plain": ("MultipleInstanceClassifier",
                       dict(_MIL, n_classes=3, feat_extraction_structure=[],
                            classification_mode="mean", attention=False), [0, 2, 1, 2], 0.05, False),
    "tt_cls": ("TransformableTransformer",
               dict(_TT, n_classes=3, input_dim=32, use_class_token=True, number_of_blocks=2,
                    mlp_structure=[32]), [0, 2, 1, 2], (0.05, 0.1), False),
    "tt_mean_train": ("TransformableTransformer",
                      dict(_TT, n_classes=2, input_dim=None, use_class_token=False,
                           number_of_blocks=2, mlp_structure=[16]), [0, 1, 1, 0], 0.05, True),
}


def net_kwargs(name):
    """Constructor arguments (copied) without ``module``."""
    return {k: (list(v) if isinstance(v, list) else v) for k, v in CONFIGS[name][1].items()}


def build_net(name, classes, backbone_cls, get_adn_fn, **extra):
    """The network ``name`` from one side's classes: ``classes`` holds ``MultipleInstanceClassifier``
    and ``TransformableTransformer`` (or their wrappers under those names), ``backbone_cls`` that
    side's ``ResNetBackbone``. Dropout rates zeroed, the module in ``eval()`` mode and frozen
    unless the network trains it. Returns (net, the rates that were zeroed)."""
    cls, _, _, _, trains = CONFIGS[name]
    module = backbone_cls(MODULE["spatial_dim"], MODULE["in_channels"], list(MODULE["structure"]),
                          list(MODULE["maxpool_structure"]),
                          adn_fn=get_adn_fn(2, "batch", "swish", 0.0))
    if not trains:
        module.requires_grad_(False)
    net = getattr(classes, cls)(module=module, **net_kwargs(name), **extra)
    rates = zero_dropout(net)
    return net, rates


def set_step_mode(net):
    """``train()`` with the 2-D module in ``eval()`` mode (a pretrained encoder: running
    statistics)."""
    net.train()
    net.module.eval()
    return net


class StepGold:
    """The records of one network (``files`` and items: what cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, f"mil_step_{name}.npz"), allow_pickle=False)
        self.files = list(self._g.files)

    def __getitem__(self, k):
        return self._g[k]
