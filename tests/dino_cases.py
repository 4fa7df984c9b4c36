"""What the DINO tests share: the two networks of tests/golden/ssl_dino_step.npz
(tools/make_dino_golden.py::step_nets) and a view of one network's records."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NETS = ("net2d", "net3d")


def step_config(name):
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn

    adn = get_adn_fn(1, "identity", "gelu", 0.0)
    if name == "net2d":   # no class token: the feature-mean path (64 tokens, 64 wide)
        return dict(backbone_args=dict(image_size=[32, 32], patch_size=[4, 4], in_channels=1,
                                       number_of_blocks=2, attention_dim=64, hidden_dim=64,
                                       n_heads=4, mlp_structure=[64], adn_fn=adn,
                                       use_class_token=False),
                    projection_head_args=dict(structure=[64, 32], adn_fn=adn), out_dim=48)
    return dict(backbone_args=dict(image_size=[16, 16, 8], patch_size=[4, 4, 4], in_channels=2,
                                   number_of_blocks=2, attention_dim=32, hidden_dim=32,
                                   embedding_size=32, n_heads=4, mlp_structure=[64], adn_fn=adn,
                                   use_class_token=True, n_registers=2),
                projection_head_args=dict(structure=[48, 24], adn_fn=adn), out_dim=40)


class StepGold:
    """The records of one network, keys without the ``<net>:`` prefix (``files`` and items: what
    cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, "ssl_dino_step.npz"), allow_pickle=False)
        self._p = name + ":"
        self.files = [k[len(self._p):] for k in self._g.files if k.startswith(self._p)]
        self.top = self._g

    def __getitem__(self, k):
        return self._g[self._p + k]
