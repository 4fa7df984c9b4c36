"""fp64 restatements of what csrc/classify.hip and adell_mri_amd/classification_metrics.py compute:
the three losses on logits with their gradients, the relative order consistency, mixup, and every
classification metric. tests/test_classification.py pins them to the recorded results of the real
reference (tests/golden/classification_step_cases.npz) and, where present, to scikit-learn and scipy;
the GPU tests compare the kernels against them."""
import numpy as np


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _softplus_neg_abs(x):
    return np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    x = _f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def log_sigmoid(x):
    x = _f64(x)
    return np.minimum(x, 0) - _softplus_neg_abs(x)


def bce_items(x, t):
    x, t = _f64(x), _f64(t)
    return np.maximum(x, 0) - x * t + _softplus_neg_abs(x)


def loss(kind, x, y, w=None, n_classes=None, g=None):
    """(item [B], reduced, dx) in fp64. ``g``: None for the gradient of the reduced value, else the
    per-item incoming gradient [B]. kind "bce": x [B] or [B, 1], soft targets y, w of 1 or B
    elements, reduced = mean; "ce": x [B, K], class weights, reduced = sum / sum(w[y]); "ordinal":
    x [B, K - 1], class weights, reduced = mean."""
    x = _f64(x)
    B = x.shape[0]
    if kind == "bce":
        xv = x.reshape(B)
        wt = np.ones(B) if w is None else np.broadcast_to(_f64(w).reshape(-1), (B,))
        raw = bce_items(xv, y)
        draw = (sigmoid(xv) - _f64(y)).reshape(x.shape)
        wt_x = wt.reshape((B,) + (1,) * (x.ndim - 1))
        denom = float(B)
    else:
        y = np.asarray(y, dtype=np.int64)
        wt = np.ones(B) if w is None else _f64(w)[y]
        wt_x = wt[:, None]
        if kind == "ce":
            m = x.max(1, keepdims=True)
            lse = m[:, 0] + np.log(np.exp(x - m).sum(1))
            raw = lse - x[np.arange(B), y]
            draw = np.exp(x - lse[:, None])
            draw[np.arange(B), y] -= 1
            denom = float(wt.sum())
        else:
            t = (y[:, None] >= np.arange(1, n_classes)[None, :]).astype(np.float64)
            ls = log_sigmoid(x)
            raw = -(ls * t + (ls - x) * (1 - t)).sum(1)
            draw = sigmoid(x) - t
            denom = float(B)
    item = wt * raw
    coef = np.full(B, 1.0 / denom) if g is None else _f64(g)
    dx = coef.reshape((B,) + (1,) * (x.ndim - 1)) * wt_x * draw
    return item, item.sum() / denom, dx


def roc(p, y):
    """(loss, dp, M) of the relative order consistency; NaN loss and gradient when M = 0."""
    p, y = _f64(p).reshape(-1), np.asarray(y, dtype=np.int64)
    d = p[:, None] - p[None, :]
    differ = y[:, None] != y[None, :]
    t = (y[:, None] > y[None, :]).astype(np.float64)
    M = int(differ.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        value = np.float64(np.where(differ, bce_items(d, t), 0.0).sum()) / np.float64(M)
        s = np.where(differ, sigmoid(d) - t, 0.0)
        dp = (s.sum(1) - s.sum(0)) / np.float64(M)
    return value, dp, M


def mixup_rows(x, factor, partner):
    """torch's expression in fp32, row by row; a row that is its own partner is copied."""
    import torch

    x = torch.as_tensor(x)
    f = torch.as_tensor(factor, dtype=torch.float32)
    out = x.clone()
    for b, pb in enumerate(np.asarray(partner).tolist()):
        if pb != b:
            out[b] = x[b] * f[b] + x[pb] * (1.0 - f[b])
    return out


# ---- metrics ---------------------------------------------------------------------------------------
def argmax_nan_wins(scores):
    """The first maximal index of every row; a NaN wins (torch.argmax)."""
    scores = np.asarray(scores)
    out = np.zeros(scores.shape[0], dtype=np.int64)
    for n, row in enumerate(scores):
        nan = np.flatnonzero(np.isnan(row))
        out[n] = nan[0] if nan.size else int(np.argmax(row))
    return out


def classes_of(preds, C):
    preds = np.asarray(preds)
    if preds.ndim == 2:
        return argmax_nan_wins(preds)
    if np.issubdtype(preds.dtype, np.integer):
        return preds.astype(np.int64)
    assert C == 2
    return (preds > 0.5).astype(np.int64)


def confusion(preds, labels, C):
    """([C, C] counts, row = label, column = prediction; the number of bad samples)."""
    pred, labels = classes_of(preds, C), np.asarray(labels, dtype=np.int64)
    bad = (labels < 0) | (labels >= C) | (pred < 0) | (pred >= C)
    M = np.zeros((C, C), dtype=np.int64)
    np.add.at(M, (labels[~bad], pred[~bad]), 1)
    return M, int(bad.sum())


def _ratio(num, den):
    num, den = _f64(num), _f64(den)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def per_class(M, kind, beta=1.0):
    M = _f64(M)
    tp = np.diag(M)
    fp, fn = M.sum(0) - tp, M.sum(1) - tp
    tn = M.sum() - tp - fp - fn
    b2 = beta * beta
    return {"recall": _ratio(tp, tp + fn), "specificity": _ratio(tn, tn + fp),
            "precision": _ratio(tp, tp + fp),
            "fbeta": _ratio((1 + b2) * tp, (1 + b2) * tp + b2 * fn + fp)}[kind]


def macro(M, kind, beta=1.0):
    M = _f64(M)
    tp = np.diag(M)
    seen = (M.sum(0) + M.sum(1) - tp) > 0
    return float(per_class(M, kind, beta)[seen].mean()) if seen.any() else 0.0


def auroc(scores, labels):
    """The Mann-Whitney statistic; NaN without a positive or a negative."""
    scores, labels = _f64(scores), np.asarray(labels)
    pos, neg = scores[labels == 1], scores[labels == 0]
    if pos.size == 0 or neg.size == 0:
        return float("nan")
    gt = (pos[:, None] > neg[None, :]).sum()
    eq = (pos[:, None] == neg[None, :]).sum()
    return float((2 * gt + eq) / (2.0 * pos.size * neg.size))


def auroc_pairs(scores, labels):
    scores, labels = np.asarray(scores), np.asarray(labels)
    pos, neg = scores[labels == 1], scores[labels == 0]
    return (int(2 * (pos[:, None] > neg[None, :]).sum() + (pos[:, None] == neg[None, :]).sum()),
            int(pos.size), int(neg.size))


def multiclass_auroc(scores, labels, C):
    labels = np.asarray(labels)
    values = [auroc(np.asarray(scores)[:, c], (labels == c).astype(np.int64)) for c in range(C)]
    values = [v for v in values if not np.isnan(v)]
    return float(np.mean(values)) if values else float("nan")


def _expand(M):
    """(labels, predictions) of the samples M counts."""
    M = np.asarray(M, dtype=np.int64)
    l, p = np.nonzero(M)
    reps = M[l, p]
    return np.repeat(l, reps).astype(np.float64), np.repeat(p, reps).astype(np.float64)


def mse(M):
    l, p = _expand(M)
    return float(((p - l) ** 2).mean())


def pearson(M):
    l, p = _expand(M)
    dl, dp = l - l.mean(), p - p.mean()
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64((dl * dp).sum()) / np.sqrt(np.float64((dl * dl).sum() * (dp * dp).sum())))


def _ranks(v):
    """Average ranks (1-based)."""
    order = np.argsort(v, kind="stable")
    ranks = np.empty(len(v))
    sv = v[order]
    i = 0
    while i < len(v):
        j = i
        while j + 1 < len(v) and sv[j + 1] == sv[i]:
            j += 1
        ranks[order[i:j + 1]] = (i + j) / 2 + 1
        i = j + 1
    return ranks


def spearman(M):
    l, p = _expand(M)
    rl, rp = _ranks(l), _ranks(p)
    dl, dp = rl - rl.mean(), rp - rp.mean()
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64((dl * dp).sum()) / np.sqrt(np.float64((dl * dl).sum() * (dp * dp).sum())))


def kappa_quadratic(M):
    M = _f64(M)
    C = M.shape[0]
    c = np.arange(C, dtype=np.float64)
    w = (c[:, None] - c[None, :]) ** 2 / (C - 1) ** 2
    expected = np.outer(M.sum(1), M.sum(0)) / M.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(1 - (w * M).sum() / np.float64((w * expected).sum()))
