"""fp64 / numpy restatements for the uncertainty tests: the AUC by counting pairs, the bootstrap's
mean and quantiles, and adaptive prediction sets by the rule the package documents (stable descending
order, every prefix an fp64 sum rounded to fp32)."""
from math import ceil

import numpy as np


# ---- AUC -------------------------------------------------------------------------------------------------
def pair_counts(scores, labels):
    """(2 #{pos > neg} + #{pos == neg}, positives, negatives) as Python ints, pair by pair; labels
    other than 0 and 1 are skipped."""
    scores = np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels)
    sp, sn = scores[labels == 1], scores[labels == 0]
    gt = int((sp[:, None] > sn[None, :]).sum())
    eq = int((sp[:, None] == sn[None, :]).sum())
    return 2 * gt + eq, int(sp.size), int(sn.size)


def pair_counts_sorted(scores, labels):
    """The same three numbers from two binary searches per positive (for sizes at which the pair
    table does not fit); tests pin it to ``pair_counts``."""
    scores = np.asarray(scores, dtype=np.float64)
    labels = np.asarray(labels)
    sp, sn = scores[labels == 1], np.sort(scores[labels == 0])
    below = np.searchsorted(sn, sp, side="left").astype(np.int64)
    upto = np.searchsorted(sn, sp, side="right").astype(np.int64)
    return int((below + upto).sum()), int(sp.size), int(sn.size)


def one_vs_rest(labels, c, n_classes):
    labels = np.asarray(labels)
    return np.where((labels >= 0) & (labels < n_classes), (labels == c).astype(np.int64), -1)


def auc(scores, labels):
    """fp64; NaN without a positive or a negative."""
    num, P, N = pair_counts(scores, labels)
    return num / (2.0 * P * N) if P * N > 0 else float("nan")


def macro_auc(scores, labels, n_classes):
    """One-vs-rest over the classes that have both a positive and a negative; NaN when none has."""
    vals = [auc(scores[:, c], one_vs_rest(labels, c, n_classes)) for c in range(n_classes)]
    vals = [v for v in vals if v == v]
    return sum(vals) / len(vals) if vals else float("nan")


def metric_value(scores, labels, n_classes):
    return auc(scores, labels) if n_classes == 2 else macro_auc(scores, labels, n_classes)


def quantile(values, q):
    """``torch.quantile`` (linear interpolation) of fp64 values; NaN when any value is."""
    v = np.sort(np.asarray(values, dtype=np.float64))
    if np.isnan(v).any():
        return float("nan")
    rank = q * (v.size - 1)
    lo, hi = int(np.floor(rank)), int(np.ceil(rank))
    w = rank - lo
    return v[lo] + w * (v[hi] - v[lo]) if w < 0.5 else v[hi] - (v[hi] - v[lo]) * (1 - w)


def bootstrap(scores, labels, n_classes, rows, interval=0.95):
    """(values [R], mean, [lower, upper] quantiles), all fp64. The two levels are rounded to fp32
    first: the reference builds them with ``torch.as_tensor([lower, upper])``, an fp32 tensor."""
    vals = np.array([metric_value(scores[r], labels[r], n_classes) for r in rows], dtype=np.float64)
    lower = (1 - interval) / 2
    levels = [float(np.float32(lower)), float(np.float32(interval + lower))]
    return vals, vals.mean(), np.array([quantile(vals, q) for q in levels])


# ---- adaptive prediction sets ------------------------------------------------------------------------------
def aps_cumulative(p):
    """fp32 [N, C]: the cumulative probability at each class's own rank."""
    p = np.asarray(p, dtype=np.float32)
    order = np.argsort(-p, axis=1, kind="stable")          # of equal values the lower index first
    prefix = np.cumsum(np.take_along_axis(p, order, 1).astype(np.float64), axis=1).astype(np.float32)
    cum = np.empty_like(prefix)
    np.put_along_axis(cum, order, prefix, 1)
    return cum


def aps_scores(p, y):
    return aps_cumulative(p)[np.arange(len(y)), np.asarray(y)]


def aps_level(n, alpha):
    return ceil((n + 1) * (1 - alpha)) / n


def aps_qhat(p, y, alpha):
    n = len(y)
    return np.sort(aps_scores(p, y))[ceil(aps_level(n, alpha) * (n - 1))]


def aps_sets(p, qhat):
    sets = aps_cumulative(p) <= np.float32(qhat)
    sets[np.arange(p.shape[0]), np.argmax(p, 1)] = True
    return sets
