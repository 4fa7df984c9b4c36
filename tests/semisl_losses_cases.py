"""Cases of the semi-supervised loss tests, shared by tools/make_semisl_losses_golden.py (which runs the
real reference on them) and by tests/test_semisl_losses*.py. Inputs that would make a fixture large
are not stored: they are a pure function of a name and a shape (oracle/weights.tensor_for), as the
networks' weights are everywhere else in the suite."""
import json
import os

import numpy as np

from oracle.weights import tensor_for

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the project's tolerances for fused losses (tests/test_semisl_gpu.py): rtol 2e-5 / atol 2e-6 on values,
# 2e-4 of the largest magnitude on gradients
VALUE_RTOL, VALUE_ATOL, GRAD_REL = 2e-5, 2e-6, 2e-4

# tag -> shape, temperature, how the anchors come about ("given", or the derangement seed of the module
# with anchors_1 given or drawn as well), whether given anchors take a gradient
ANCHOR_CASES = {
    "a": dict(shape=(3, 8, 3, 5, 7), temperature=0.1, anchors="given", anchor_grad=True),
    "b": dict(shape=(2, 4, 17, 16, 16), temperature=0.1, anchors="given", anchor_grad=True),
    "c": dict(shape=(2, 20, 9, 11, 13), temperature=0.2, anchors="given", anchor_grad=True),
    "d": dict(shape=(2, 8, 6, 10), temperature=0.1, anchors="given", anchor_grad=True),
    "e": dict(shape=(3, 8, 3, 5, 7), temperature=0.1, anchors="drawn", seed=42),
    "f": dict(shape=(4, 8, 6, 10), temperature=0.15, anchors="second drawn", seed=7),
}
GRAD_SAMPLE_STRIDE = 13     # cases with more than GRAD_FULL_LIMIT elements store every 13th gradient element
GRAD_FULL_LIMIT = 4096


def anchor_inputs(tag):
    """(x, a1, a2, r) as fp32 numpy arrays: anchors correlated with x, r the weights of the items."""
    shape = ANCHOR_CASES[tag]["shape"]
    x = tensor_for(f"semisl_anchor:{tag}:x", shape, 1.0)
    a1 = 0.5 * x + tensor_for(f"semisl_anchor:{tag}:a1", shape, 1.0)
    a2 = tensor_for(f"semisl_anchor:{tag}:a2", shape, 1.0) - 0.25 * x
    r = 0.5 + np.abs(tensor_for(f"semisl_anchor:{tag}:r", (shape[0],), 1.0))
    return x, a1.astype(np.float32), a2.astype(np.float32), r.astype(np.float32)


def grad_sample(g):
    """What the fixture keeps of a gradient: all of it, or every GRAD_SAMPLE_STRIDE-th element."""
    g = np.asarray(g).reshape(-1)
    return g if g.size <= GRAD_FULL_LIMIT else g[::GRAD_SAMPLE_STRIDE]


# ---- nearest-neighbour script ---------------------------------------------------------------------------
NN_ARGS = dict(maxsize=16, n_classes=3, max_elements_per_batch=6, n_samples_per_class=2,
               temperature=0.1, seed=42)
NN_SHAPE = (2, 8, 3, 5, 7)       # 105 voxels: odd
NN_PUTS = 3


def nn_put_inputs(i):
    """(X, y) of put call i: class 0 overflows max_elements_per_batch, class 1 stays under it (four
    voxels, in both items), class 2 is never present."""
    B, C = NN_SHAPE[:2]
    sp = NN_SHAPE[2:]
    X = tensor_for(f"semisl_nn:put{i}:X", NN_SHAPE, 1.0)
    y = np.zeros((B, NN_ARGS["n_classes"]) + sp, dtype=np.float32)
    y[:, 0] = (tensor_for(f"semisl_nn:put{i}:y0", (B,) + sp, 1.0) > 0.0)
    V = int(np.prod(sp))
    for b, where in ((0, [3 + i, 50]), (1, [7, V - 1 - i])):
        plane = np.zeros(V, dtype=np.float32)
        plane[where] = 1.0
        y[b, 1] = plane.reshape(sp)
    return X, y


def nn_forward_inputs():
    """(X, y) of the forward: multi-hot float labels, as the reference's own tests use."""
    X = tensor_for("semisl_nn:fwd:X", NN_SHAPE, 1.0)
    y = (tensor_for("semisl_nn:fwd:y", (NN_SHAPE[0], NN_ARGS["n_classes"]) + NN_SHAPE[2:], 1.0)
         > 0.0).astype(np.float32)
    return X, y


# ---- pseudo-label cases ---------------------------------------------------------------------------------
PL_SHAPE = (2, 3, 5, 7, 3)
PL_THRESHOLD = 0.7
PL_CASES = {
    "plain": dict(),
    "weight": dict(weight=[0.2, 1.0, 3.0]),
    "smooth": dict(label_smoothing=0.1),
    "sum": dict(reduction="sum"),
    "all": dict(weight=[0.2, 1.0, 3.0], label_smoothing=0.1, reduction="sum"),
}


def pl_inputs():
    """(pred, proba): a tenth of the probabilities are exactly fp32(PL_THRESHOLD) (not above it)."""
    pred = 3.0 * tensor_for("semisl_pl:pred", PL_SHAPE, 1.0)
    proba = 0.5 + 0.5 * tensor_for("semisl_pl:proba", PL_SHAPE, 1.0)
    at = tensor_for("semisl_pl:at", PL_SHAPE, 1.0) > 0.8
    proba[at] = np.float32(PL_THRESHOLD)
    return pred.astype(np.float32), proba.astype(np.float32)


# ---- tolerances -----------------------------------------------------------------------------------------
def bounds():
    with open(os.path.join(GOLD, "semisl_losses_bounds.json")) as fh:
        return json.load(fh)


def value_tol(key, ref, table=None):
    """Allowed absolute error of a value: the project's, or four times the reference's own fp32 error
    where the bounds file records one for ``key``."""
    tol = VALUE_ATOL + VALUE_RTOL * np.abs(np.asarray(ref, dtype=np.float64))
    extra = (table if table is not None else bounds()).get(key, {}).get("tol")
    return np.maximum(tol, extra) if extra is not None else tol


def grad_tol(key, ref, table=None):
    """Allowed absolute error of a gradient element, likewise."""
    tol = GRAD_REL * float(np.abs(np.asarray(ref, dtype=np.float64)).max())
    extra = (table if table is not None else bounds()).get(key, {}).get("tol")
    return max(tol, extra) if extra is not None else tol
