"""What the iBOT tests share: the two networks of tests/golden/ibot_step.npz
(tools/make_ibot_golden.py::step_nets -- the two of dino_cases.py with a masker added) and a view of
one network's records, which reads the parameters and the EMA after the step (``step1:*``,
``ema1:*``) from tests/golden/ibot_step_params.npz."""
import os

import numpy as np

from dino_cases import GOLD, NETS, step_config as dino_config  # noqa: F401

MASK_SEED = 42


def step_config(name):
    cfg = dino_config(name)
    ba = cfg["backbone_args"]
    if name == "net2d":   # no class token, "mean": 8 x 8 patch tokens of 64 features
        ba["embedding_size"] = 64
        cfg.update(feature_map_dimensions=[8, 8], n_encoder_features=64, min_patch_size=[2, 2],
                   max_patch_size=[4, 4], n_patches=3, reduce_fn="mean", seed=MASK_SEED)
    else:                 # class token + 2 registers, "cls": 4 x 4 x 3 patch tokens of 32 features
        ba["image_size"] = [16, 16, 12]
        cfg.update(feature_map_dimensions=[4, 4, 3], n_encoder_features=32,
                   min_patch_size=[1, 1, 1], max_patch_size=[3, 3, 2], n_patches=2,
                   reduce_fn="cls", seed=MASK_SEED)
    return cfg


class StepGold:
    """The records of one network, keys without the ``<net>:`` prefix (``files`` and items: what
    cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, "ibot_step.npz"), allow_pickle=False)
        self._after = np.load(os.path.join(GOLD, "ibot_step_params.npz"), allow_pickle=False)
        self._p = name + ":"
        self.files = [k[len(self._p):] for k in self._g.files + self._after.files
                      if k.startswith(self._p)]
        self.top = self._g

    def __getitem__(self, k):
        k = self._p + k
        return self._after[k] if k in self._after.files else self._g[k]
