"""fp64 / numpy restatement of the segmentation metrics of adell_mri_amd.metrics (the yardstick of
tests/test_seg_metrics*.py; not a test module). Written from the definitions in the metrics module
docstring, not from any implementation."""
import numpy as np

KINDS = ("iou", "precision", "fbeta", "dice")


def _target_classes(target, n):
    """Class index per voxel (-1: outside [0, n)) after round-half-even of float targets."""
    t = np.asarray(target)
    if t.dtype == np.bool_:
        t = t.astype(np.int64)
    if np.issubdtype(t.dtype, np.floating):
        with np.errstate(invalid="ignore"):
            r = np.rint(t.astype(np.float32))
        ok = (r >= 0) & (r < n)                       # NaN compares false
        return np.where(ok, np.nan_to_num(r), -1).astype(np.int64)
    t = t.astype(np.int64)
    return np.where((t >= 0) & (t < n), t, -1)


def counts(pred, target):
    """(counts int64 [C][3] = (tp, fp, fn), bad-target flag) of ONE update; pred [B, C, ...] fp32,
    target [B, ...] or [B, 1, ...]."""
    pred = np.asarray(pred, dtype=np.float32)
    C = pred.shape[1]
    if C == 1:
        p = pred.reshape(-1)
        tc = _target_classes(target, 2).reshape(-1)
        with np.errstate(invalid="ignore", over="ignore"):
            out_of_range = bool(np.any(~((p >= 0) & (p <= 1))))
            if out_of_range:
                s = np.float32(1) / (np.float32(1) + np.exp(-p))     # fp32 sigmoid
                m = s > np.float32(0.5)
            else:
                m = p > np.float32(0.5)
        t = tc == 1
        c = np.array([[np.sum(m & t), np.sum(m & ~t), np.sum(~m & t)]], dtype=np.int64)
        return c, bool(np.any(tc < 0))
    B = pred.shape[0]
    p = pred.reshape(B, C, -1)
    pc = np.argmax(p, axis=1).reshape(-1)        # first maximum; numpy's argmax returns the first NaN
    tc = _target_classes(target, C).reshape(-1)
    c = np.zeros((C, 3), dtype=np.int64)
    for k in range(C):
        c[k] = (np.sum((pc == k) & (tc == k)), np.sum((pc == k) & (tc != k)),
                np.sum((tc == k) & (pc != k)))
    return c, bool(np.any(tc < 0))


def value(c, kind, beta=1.0):
    """The metric of accumulated counts [C][3], fp64, macro over the classes that occur."""
    b = float(np.float32(beta))
    b2 = b * b
    vals = []
    for tp, fp, fn in np.asarray(c, dtype=np.int64):
        if tp + fp + fn == 0:
            continue
        tp, fp, fn = float(tp), float(fp), float(fn)
        if kind == "iou":
            num, den = tp, tp + fp + fn
        elif kind == "precision":
            num, den = tp, tp + fp
        elif kind == "fbeta":
            num, den = (1.0 + b2) * tp, (1.0 + b2) * tp + b2 * fn + fp
        else:
            num, den = 2.0 * tp, 2.0 * tp + fp + fn
        vals.append(num / den if den > 0 else 0.0)
    return sum(vals) / len(vals) if vals else 0.0


def within_one_ulp(got, want):
    w = np.float32(want)
    return abs(np.float32(got) - w) <= np.spacing(np.abs(w)) or np.float32(got) == w
