"""What the classification tests share: the fixture networks of
tests/golden/classification_step_<net>.npz (tools/make_classification_golden.py; the loss cases,
draws and tables are in classification_step_cases.npz), the weights both sides
load, and a view of one network's records."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETS = ("cat2", "cat3", "ord4", "vit_cls", "vit_mean")
# ``learning_rate`` and ``optimizer_eps`` of the fixture steps (constructor arguments of the wrappers).
# AdamW's first step moves a parameter by lr g / (|g| + eps): an error d in g moves it by up to
# lr d / eps. Batch norm over four items makes gradients of order 1 whose fp32 error is of order 1e-5,
# and a conv bias in front of a batch norm has a gradient that is rounding noise only; with the
# defaults (1e-3, 1e-8) the reference's own fp32 step misses its fp64 step by 300 parameter
# tolerances. lr / eps = 1e-2 keeps that below a quarter of one, and the step (1e-4) at 50 of them.
STEP_LR, STEP_EPS = 1e-4, 1e-2

_RESNET = dict(spatial_dimensions=3, in_channels=2, resnet_structure=[(8, 16, 3, 2), (16, 32, 3, 2)],
               maxpool_structure=[(2, 2, 2), (2, 2, 2)])
_VIT = dict(image_size=[8, 16], patch_size=[4, 4], in_channels=2, number_of_blocks=2, attention_dim=32,
            hidden_dim=32, n_heads=2, mlp_structure=[32], n_registers=2)
# name: (class, constructor arguments, input shape, labels, class weights, weight decay of the step)
CONFIGS = {
    "cat2": ("CatNet", dict(_RESNET, n_classes=2), (4, 2, 16, 16, 8), [0, 1, 1, 0], None, 0.05),
    "cat3": ("CatNet", dict(_RESNET, n_classes=3), (4, 2, 16, 16, 8), [0, 2, 1, 2], [0.5, 1.0, 2.0],
             (0.05, 0.1)),
    "ord4": ("OrdNet", dict(_RESNET, n_classes=4, classification_structure=[16, 16, 16]),
             (6, 2, 16, 16, 8), [0, 1, 2, 3, 1, 2], None, 0.05),
    "vit_cls": ("ViTClassifier", dict(_VIT, n_classes=3, use_class_token=True), (4, 2, 8, 16),
                [0, 2, 1, 2], None, 0.05),
    "vit_mean": ("ViTClassifier", dict(_VIT, n_classes=2, use_class_token=False), (4, 2, 8, 16),
                 [0, 1, 1, 0], None, (0.05, 0.1)),
}


def net_kwargs(name):
    """Constructor arguments (copied) without ``adn_fn``: the ResNets take
    ``get_adn_fn(3, "batch", "swish", 0.0)`` of the side that builds them."""
    kw = CONFIGS[name][1]
    return {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}


def fill(state_dict, gain):
    from oracle.weights import fill_state_dict

    return fill_state_dict(state_dict, gain=gain, norm_weight_offset=1.0)


def zero_dropout(net):
    """Every ``torch.nn.Dropout`` to p = 0 (the heads' 0.1 is hard-coded and would make the step
    random); returns what the rates were."""
    import torch

    rates = []
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout):
            rates.append(m.p)
            m.p = 0.0
    return rates


def step_groups(named_parameters, weight_decay):
    """The parameter groups of ``ClassPLABC.configure_optimizers`` as (names, weight decay) and
    the base weight decay, restated on parameter names."""
    names = [n for n, p in named_parameters if p.requires_grad]
    reduced = [n for n in names if "ordinal_bias" in n]
    rest = [n for n in names if "ordinal_bias" not in n]
    if isinstance(weight_decay, (list, tuple)):
        wd_body, wd_head = weight_decay
        head = [n for n in rest if "classification" in n]
        body = [n for n in rest if "classification" not in n]
        return [([], 0), (reduced, wd_body / 100), (head, wd_head), (body, wd_body)], wd_body / 100
    wd = float(weight_decay)
    return [([], 0), (reduced, wd / 100), (rest, wd)], wd / 100


class StepGold:
    """The records of one network, keys without the ``<net>:`` prefix (``files`` and items: what
    cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, f"classification_step_{name}.npz"), allow_pickle=False)
        self._p = name + ":"
        self.files = [k[len(self._p):] for k in self._g.files if k.startswith(self._p)]

    def __getitem__(self, k):
        return self._g[self._p + k]


def case_gold():
    """The loss cases, the recorded draws and the tables."""
    return np.load(os.path.join(GOLD, "classification_step_cases.npz"), allow_pickle=False)
