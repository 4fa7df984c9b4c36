"""Inputs of the uncertainty tests (bootstrap AUC intervals, adaptive prediction sets): shared by
tools/make_uncertainty_golden.py, which records the reference's results for them in
tests/golden/uncertainty.npz, and by the tests, which read the recorded inputs from that file."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALPHA = 0.2

# (n, C) of the adaptive-prediction-set cases; (33, 2) is CPU-only ground
APS_CASES = [(4, 2), (9, 3), (37, 5), (64, 17), (200, 64)]
APS_CPU_CASES = APS_CASES + [(33, 2)]

# name -> (n, classes (2: binary scores [n]), resamples, sample_size, seed of bootstrap_metric)
BOOT_CASES = {"bin": (301, 2, 100, 0.5, 42), "mc": (200, 3, 40, 0.5, 7)}


def aps_key(n, C):
    return f"aps_{n}_{C}"


def aps_inputs(n, C):
    """fp32 probabilities [n, C] (a softmax in fp64, rounded) and int64 labels [n]."""
    rng = np.random.RandomState(1000 * n + C)
    z = rng.randn(n, C) * 2.0
    e = np.exp(z - z.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32), rng.randint(0, C, n).astype(np.int64)


def aps_tied_inputs(n, C, seed=5):
    """Rows with many equal probabilities: multiples of 1 / 16 that sum to 1 exactly."""
    rng = np.random.RandomState(seed)
    p = np.zeros((n, C), dtype=np.float32)
    for i in range(n):
        for c in rng.randint(0, C, 16):
            p[i, c] += 1.0 / 16.0
    return p, rng.randint(0, C, n).astype(np.int64)


def boot_inputs(name):
    """(scores fp32 [n] or [n, C], labels int64 [n]): informative scores with ties (two decimals)."""
    n, C, _, _, seed = BOOT_CASES[name]
    rng = np.random.RandomState(seed)
    y = rng.randint(0, C, n).astype(np.int64)
    if C == 2:
        s = np.clip(0.5 + 0.2 * (2 * y - 1) + 0.25 * rng.randn(n), 0, 1)
        return np.round(s, 2).astype(np.float32), y
    z = rng.randn(n, C) + 1.5 * np.eye(C)[y]
    e = np.exp(z - z.max(1, keepdims=True))
    return np.round(e / e.sum(1, keepdims=True), 2).astype(np.float32), y


def pair_case(n, kind="ties", seed=0, classes=2):
    """Scores and labels of a pair-count case. kind: "ties" (one decimal: tie groups cross the
    32-bit words), "equal" (one score), "nopos" (no positive at all)."""
    rng = np.random.RandomState(seed + 17 * n)
    y = rng.randint(0, classes, n).astype(np.int64)
    if classes == 2:
        s = np.round(rng.rand(n), 1).astype(np.float32)
    else:
        s = np.round(rng.rand(n, classes), 1).astype(np.float32)
    if kind == "equal":
        s[...] = 0.5
    if kind == "nopos":
        y[...] = 0
    return s, y


def resample_rows(n, R, m, seed=0):
    """int32 [R, m]: distinct indices per row."""
    rng = np.random.RandomState(seed + n + 31 * R)
    return np.stack([rng.permutation(n)[:m] for _ in range(R)]).astype(np.int32)


def golden():
    return np.load(os.path.join(GOLD, "uncertainty.npz"))


def surface():
    with open(os.path.join(GOLD, "uncertainty_surface.json")) as fh:
        return json.load(fh)


def signature_of(fn):
    """[name, kind, default] per parameter; a class default by its name."""
    import inspect

    out = []
    for p in inspect.signature(fn).parameters.values():
        d = p.default
        d = None if d is inspect.Parameter.empty else (d.__name__ if inspect.isclass(d) else repr(d))
        out.append([p.name, p.kind.name, d])
    return out
