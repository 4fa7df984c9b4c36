"""What the deconfounded-classification tests and tools/make_deconfounded_golden.py share: the kernel
cases of tests/golden/deconfounded_kernels.npz, the two fixture networks of
tests/golden/deconfounded_step_<net>.npz, their inputs and the bounds
(tests/golden/deconfounded_bounds.json)."""
import json
import os
import zlib

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUM_BOUND = 5e-5
# the step tolerances of tests/test_classification_gpu.py and tests/test_batch_ensemble_gpu.py
TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6))
STEP_LR, STEP_EPS = 1e-4, 1e-2          # tests/classification_cases.py says why
STEP_WD = 0.05                          # non-zero: Adam and AdamW differ in the step

# ---- kernel cases ----------------------------------------------------------------------------------------
# (B, F, n_conf) of the correlation loss; with F >= 24, column 1 and column n_conf + 1 are exactly 0
CORR_CASES = [(3, 7, 1), (5, 9, 8), (5, 24, 8), (7, 130, 3), (70, 40, 17), (33, 512, 64),
              (4, 2048, 64)]
CORR_EDGE = (2, 6, 2)                   # two items: every r is +-1, on the clamp's edge
CORR_DUP = (6, 12, 3)                   # column n_conf is a copy of column 0: r = 1, forward only

# the fused limits of deconf_heads_loss (functional.deconf_route)
MAX_HEADS, MAX_CLASSES, MAX_CONT, MAX_CONF = 8, 64, 64, 1024
# heads: (categorical class counts, regression outputs)
HEADS = {"one": ((3,), 0), "two": ((2, 5), 0), "both": ((2, 5), 2), "cont": ((), 2)}
HEAD_B = (3, 5, 70)
HEAD_NCONF = (1, 8, 65)
# just beyond each fused limit: (n_conf, class counts, n_cont); the composed route
HEADS_BEYOND = {
    "heads": (4, (2,) * (MAX_HEADS + 1), 0),
    "classes": (4, (MAX_CLASSES + 1,), 0),
    "cont": (4, (), MAX_CONT + 1),
    "conf": (MAX_CONF + 1, (3,), 1),
}
SPLIT_CASES = [(3, 7, 1), (5, 9, 8), (70, 130, 65), (4, 2048, 64)]


def uniform(tag, shape, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    return rng.uniform(lo, hi, size=tuple(shape)).astype(np.float32)


def corr_input(B, F, n, zero_columns=None):
    """Uniform in (-1, 1); with F >= 24 (or on request) column 1 and column n + 1 are exactly 0."""
    x = uniform(f"corr:{B}:{F}:{n}", (B, F))
    if (F >= 24) if zero_columns is None else zero_columns:
        x[:, 1] = 0.0
        x[:, n + 1] = 0.0
    return x


def corr_zero_columns(B, F, n):
    return [1, n + 1] if F >= 24 else []


def dup_input():
    B, F, n = CORR_DUP
    x = uniform("corr:dup", (B, F))
    x[:, n] = x[:, 0]
    return x


def heads_case(B, F, n, classes, n_cont, tag=""):
    """features, [(W, b)] per categorical head, labels int64 [H, B], (Wc, bc), regression target."""
    t = f"heads:{B}:{F}:{n}:{classes}:{n_cont}:{tag}"
    s = 1.0 / np.sqrt(n)
    cat = [(uniform(f"{t}:W{h}", (K, n), -2 * s, 2 * s), uniform(f"{t}:b{h}", (K,), -0.5, 0.5))
           for h, K in enumerate(classes)]
    rng = np.random.default_rng(zlib.crc32((t + ":y").encode()))
    labels = np.stack([rng.integers(0, K, size=B) for K in classes]).astype(np.int64) \
        if classes else np.zeros((0, B), dtype=np.int64)
    cont = (uniform(f"{t}:Wc", (n_cont, n), -2 * s, 2 * s), uniform(f"{t}:bc", (n_cont,), -0.5, 0.5)) \
        if n_cont else None
    target = uniform(f"{t}:yc", (B, n_cont)) if n_cont else None
    return uniform(f"{t}:x", (B, F)), cat, labels, cont, target


# ---- networks --------------------------------------------------------------------------------------------
CAT_VARS = {"a": [["s1", "s2", "s3"], ["m", "f"]], "b": [["s1", "s2", "s3"]]}
# name: constructor arguments of DeconfoundedNetGeneric (without adn_fn), input shape, labels, the
# categorical confounders per item, the continuous ones (None: no such key), multi-class loss
NETS = {
    "a": (dict(n_classes=2, in_channels=1, feature_extraction_module="cat",
               classification_structure=[16, 16], n_dim=3, n_features_deconfounder=6,
               n_cat_deconfounder=[3, 2], n_cont_deconfounder=2, spatial_dimensions=3,
               resnet_structure=[(8, 8, 3, 2), (16, 16, 3, 2)],
               maxpool_structure=[(2, 2, 2), (2, 2, 2)]),
          (4, 1, 16, 16, 8), [0, 1, 1, 0],
          [["s2", "m"], ["s1", "f"], ["s3", "f"], ["s2", "m"]],
          [[0.3, -1.2], [1.1, 0.4], [-0.7, 0.9], [0.2, -0.1]]),
    "b": (dict(n_classes=3, in_channels=1, feature_extraction_module="cat",
               classification_structure=[16, 16], n_dim=2, n_features_deconfounder=5,
               n_cat_deconfounder=[3], exclude_surrogate_variables=True,
               deconfounder_structure=[8], spatial_dimensions=2,
               resnet_structure=[(8, 8, 3, 2), (16, 16, 3, 2)], maxpool_structure=[(2, 2), (2, 2)]),
          (4, 1, 16, 16), [0, 2, 1, 2],
          [["s3"], ["s1"], ["s2"], ["s1"]], None),
}


def net_kwargs(name):
    kw = NETS[name][0]
    return {k: (list(v) if isinstance(v, list) else v) for k, v in kw.items()}


def cat_table(name):
    """The int64 [n_heads, B] codes of the network's categorical confounders."""
    maps = [{k: i for i, k in enumerate(keys)} for keys in CAT_VARS[name]]
    return np.array([[maps[h][item[h]] for item in NETS[name][3]] for h in range(len(maps))],
                    dtype=np.int64)


def fill(state_dict, gain):
    from oracle.weights import fill_state_dict

    return fill_state_dict(state_dict, gain=gain, norm_weight_offset=1.0)


def step_input(name, seed):
    shape = NETS[name][1]
    grids = np.meshgrid(*[np.arange(float(s)) for s in shape[2:]], indexing="ij")
    z = np.cos(0.45 * grids[2]) if len(grids) > 2 else 1.0
    x = np.stack([np.stack([np.sin((b + 1) * 0.37 * grids[0] + c) * np.cos((b + 2) * 0.23 * grids[1])
                            * z + 0.1 * b for c in range(shape[1])]) for b in range(shape[0])])
    return (x + 0.2 * uniform(f"deconf:{name}:{seed}", shape, 0.0, 1.0)).astype(np.float32)


def signature_of(fn):
    """[name, kind, default] per parameter; a class default by its name."""
    import inspect

    out = []
    for p in inspect.signature(fn).parameters.values():
        d = p.default
        d = None if d is inspect.Parameter.empty else (d.__name__ if inspect.isclass(d) else repr(d))
        out.append([p.name, p.kind.name, d])
    return out


def bounds():
    with open(os.path.join(GOLD, "deconfounded_bounds.json")) as fh:
        return json.load(fh)


def surface_gold():
    with open(os.path.join(GOLD, "deconfounded_surface.json")) as fh:
        return json.load(fh)


def kernel_gold():
    return np.load(os.path.join(GOLD, "deconfounded_kernels.npz"), allow_pickle=False)


class StepGold:
    """The records of one network (``files`` and items: what cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, f"deconfounded_step_{name}.npz"), allow_pickle=False)
        self.files = list(self._g.files)

    def __getitem__(self, k):
        return self._g[k]
