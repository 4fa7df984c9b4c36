"""What the masked-autoencoder tests share: the two networks of tests/golden/mae_step.npz
(tools/make_mae_golden.py), the weights both sides load, and a view of one network's records."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETS = ("c1", "c2")
B = 3

# name: (constructor arguments, tokens L, width E, kept tokens K)
_STACK = dict(number_of_blocks=2, hidden_dim=32, mlp_structure=[32])
CONFIGS = {
    # one channel: the "image" is a view of the predictions
    "c1": (dict(image_size=[16, 16], patch_size=[4, 4], in_channels=1, input_dim_size=96,
                encoder_args=dict(_STACK, n_heads=2), decoder_args=dict(_STACK, n_heads=2),
                mask_fraction=0.75), 16, 16, 4),
    # non-square, two interleaved channels; int(12 * (1 - 0.6)) = int(4.8) = 4: the truncation
    "c2": (dict(image_size=[16, 24], patch_size=[4, 8], in_channels=2, input_dim_size=96,
                encoder_args=dict(_STACK, n_heads=4), decoder_args=dict(_STACK, n_heads=4),
                mask_fraction=0.6), 12, 64, 4),
}


def step_config(name):
    cfg = CONFIGS[name][0]
    return {k: (dict(v) if isinstance(v, dict) else v) for k, v in cfg.items()}


def fill(state_dict, gain):
    """The weights of a fixture network: ``oracle.weights.fill_state_dict``, with the positional
    embedding -- one Parameter under two state keys -- given the values of its first key."""
    from oracle.weights import fill_state_dict

    sd = fill_state_dict(state_dict, gain=gain)
    sd["proj.positional_embedding"] = sd["positional_embedding"].clone()
    return sd


class StepGold:
    """The records of one network, keys without the ``<net>:`` prefix (``files`` and items: what
    cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, "mae_step.npz"), allow_pickle=False)
        self._p = name + ":"
        self.files = [k[len(self._p):] for k in self._g.files if k.startswith(self._p)]
        self.top = self._g

    def __getitem__(self, k):
        return self._g[self._p + k]
