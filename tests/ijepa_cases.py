"""What the I-JEPA tests share: the two networks of tests/golden/ijepa_step.npz
(tools/make_ijepa_golden.py::step_nets -- the two ViTs of dino_cases.py with an I-JEPA predictor and
masker), the configuration whose first draw leaves no target token, the token counts the reference's
masker draws for them, and a view of one network's records."""
import os

import numpy as np

from dino_cases import GOLD, NETS, step_config as dino_config  # noqa: F401

# context tokens and target tokens (after the set difference, dropped blocks as 0) of the first and
# the second draw -- what tools/make_ijepa_golden.py asserts of the reference's own masker
DRAWS = {
    "net2d": [(12, [6, 0, 4, 4]), (10, [7, 3, 2, 3])],
    "net3d": [(4, [7, 2, 3]), (7, [3, 1, 6])],
    "empty": [(16, [0, 0])],
}


def step_config(name):
    cfg = dino_config(name)
    del cfg["out_dim"]
    ba, adn = cfg["backbone_args"], cfg["backbone_args"]["adn_fn"]
    if name == "net2d":   # no class token: 8 x 8 patch tokens of 64 features, predictor 32 wide
        ba["embedding_size"] = 64
        cfg.update(projection_head_args=dict(number_of_blocks=2, attention_dim=32, hidden_dim=32,
                                             n_heads=4, mlp_structure=[64], adn_fn=adn),
                   feature_map_dimensions=[8, 8], n_encoder_features=64, min_patch_size=[2, 2],
                   max_patch_size=[4, 4], n_patches=2, n_masked_patches=4, predictor_dim=32,
                   seed=48)
    else:                 # class token + 2 registers: 6 x 6 x 4 patch tokens of 32 features
        ba["image_size"] = [24, 24, 16]
        cfg.update(projection_head_args=dict(number_of_blocks=2, attention_dim=32, hidden_dim=32,
                                             n_heads=4, mlp_structure=[64], adn_fn=adn),
                   feature_map_dimensions=[6, 6, 4], n_encoder_features=32,
                   min_patch_size=[1, 1, 1], max_patch_size=[3, 3, 3], n_patches=2,
                   n_masked_patches=3, predictor_dim=None, seed=42)
    return cfg


def empty_config():
    """net2d with three context and two target blocks and seed 1: the first draw puts both targets
    inside the 16 context tokens."""
    cfg = step_config("net2d")
    cfg.update(n_patches=3, n_masked_patches=2, seed=1)
    return cfg


class StepGold:
    """The records of one network, keys without the ``<net>:`` prefix (``files`` and items: what
    cases.grad_rel_err reads); the parameters and the EMA after the step (``step1:*``, ``ema1:*``)
    come from tests/golden/ijepa_step_params.npz and ijepa_step_ema.npz."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, "ijepa_step.npz"), allow_pickle=False)
        self._after = [np.load(os.path.join(GOLD, f), allow_pickle=False)
                       for f in ("ijepa_step_params.npz", "ijepa_step_ema.npz")]
        self._p = name + ":"
        self.files = [k[len(self._p):] for f in [self._g] + self._after for k in f.files
                      if k.startswith(self._p)]
        self.top = self._g

    def __getitem__(self, k):
        k = self._p + k
        for f in self._after:
            if k in f.files:
                return f[k]
        return self._g[k]

    def draw(self, i):
        """(context indices, [target indices per kept block]) of draw ``i``."""
        blocks = int(self[f"draw{i}:blocks"])
        return self[f"draw{i}:context"], [self[f"draw{i}:target{j}"] for j in range(blocks)]
