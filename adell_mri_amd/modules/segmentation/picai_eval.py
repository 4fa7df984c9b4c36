"""PI-CAI lesion-level evaluation on the device: the reference's ``picai_eval.evaluate`` as its
segmentation wrappers call it at the end of every validation / test epoch
(adell_mri/modules/segmentation/pl.py:609-652: ``evaluate(y_det=all_pred, y_true=all_true,
y_det_postprocess_func=get_lesions)``, every other argument at its default).

The device part (``ops.picai_tables``, csrc/components.hip) labels the detection map
``pred > 0.1`` (``get_lesions``, pl.py:75-97) and the target ``astype(int32) != 0`` with the
26-connected structure of ``scipy.ndimage.label``, counts every component's voxels, takes every
candidate's confidence (the maximum of the detection map over it: 1 for the thresholded map) and
keeps the (GT lesion, candidate, intersection) triples whose IoU can reach 0.1. Only these tables
reach the host, one packed record per case; nothing proportional to the voxel count does.

The host part is small numpy fp64 (``evaluate_case``, picai_eval/eval.py:51-251, and ``Metrics``,
picai_eval/metrics.py:114-404): IoU ``(inter + 1e-8) / (union + 1e-8)``, entries below
``min_overlap`` dropped, the rest + 1, a maximising rectangular assignment on the rows and columns
that keep an entry, then the (is_lesion, confidence, overlap) lists. AP, AUROC and score restate
scikit-learn's ``precision_recall_curve`` / ``roc_curve`` / ``auc`` (mergesort tie order, unit sample
weights). NaN for one-class sets (all benign, or no benign case) is part of the contract. scipy and
scikit-learn are not dependencies. Where the assignment has ties the matched pair may differ from
scipy's; AP, score and AUROC cannot (the counts they use do not depend on the choice).
"""
import numpy as np
import torch

from ... import ops

_EPS = 1e-8


# ---- host numerics ------------------------------------------------------------------------
def linear_sum_assignment_max(matrix):
    """Rows and columns of a maximum-weight assignment of a rectangular matrix (scipy's
    ``linear_sum_assignment(matrix, maximize=True)``; shortest augmenting paths). Rows ascending."""
    a = np.asarray(matrix, dtype=np.float64)
    if a.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    transposed = a.shape[0] > a.shape[1]
    cost = -(a.T if transposed else a)
    n, m = cost.shape
    u = np.zeros(n + 1)
    v = np.zeros(m + 1)
    p = np.zeros(m + 1, np.int64)        # p[j]: 1-based row on column j (0: none)
    way = np.zeros(m + 1, np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(m + 1, np.inf)
        used = np.zeros(m + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used
            free[0] = False
            cur = cost[i0 - 1] - u[i0] - v[1:]
            upd = free[1:] & (cur < minv[1:])
            minv[1:][upd] = cur[upd]
            way[1:][upd] = j0
            cand = np.where(free, minv, np.inf)
            j1 = int(np.argmin(cand))
            delta = cand[j1]
            u[p[used]] += delta
            v[used] -= delta
            minv[free] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    cols = np.nonzero(p[1:])[0]
    rows = p[1:][cols] - 1
    if transposed:
        rows, cols = cols, rows
    order = np.argsort(rows, kind="stable")
    return rows[order].astype(np.int64), cols[order].astype(np.int64)


def _binary_clf_curve(y_true, y_score):
    y_true = np.asarray(y_true, dtype=np.float64) == 1
    y_score = np.asarray(y_score, dtype=np.float64)
    desc = np.argsort(y_score, kind="mergesort")[::-1]
    y_score = y_score[desc]
    y_true = y_true[desc]
    distinct = np.where(np.diff(y_score))[0]
    thr_idx = np.r_[distinct, y_true.size - 1]
    tps = np.cumsum(y_true * 1.0, dtype=np.float64)[thr_idx]
    fps = np.cumsum((1.0 - y_true) * 1.0, dtype=np.float64)[thr_idx]
    return fps, tps, y_score[thr_idx]


def precision_recall_curve(y_true, y_score):
    """scikit-learn's ``precision_recall_curve`` (unit weights, ``drop_intermediate=False``)."""
    fps, tps, thresholds = _binary_clf_curve(y_true, y_score)
    ps = tps + fps
    precision = np.zeros_like(tps)
    np.divide(tps, ps, out=precision, where=ps != 0)
    recall = np.ones_like(tps) if tps[-1] == 0 else tps / tps[-1]
    return np.hstack((precision[::-1], 1)), np.hstack((recall[::-1], 0)), thresholds[::-1]


def roc_curve(y_true, y_score):
    """scikit-learn's ``roc_curve`` (unit weights, ``drop_intermediate=True``); NaN rates for a
    missing class."""
    fps, tps, thresholds = _binary_clf_curve(y_true, y_score)
    if len(fps) > 2:
        keep = np.where(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thresholds = fps[keep], tps[keep], thresholds[keep]
    tps = np.r_[0, tps]
    fps = np.r_[0, fps]
    thresholds = np.r_[np.inf, thresholds]
    fpr = np.repeat(np.nan, fps.shape) if fps[-1] <= 0 else fps / fps[-1]
    tpr = np.repeat(np.nan, tps.shape) if tps[-1] <= 0 else tps / tps[-1]
    return fpr, tpr, thresholds


def auc(x, y):
    """scikit-learn's ``auc``: trapezoidal area under a monotone curve."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if x.shape[0] < 2:
        raise ValueError(f"At least 2 points are needed to compute area under curve, got {x.shape[0]}")
    direction = 1
    dx = np.diff(x)
    if np.any(dx < 0):
        if np.all(dx <= 0):
            direction = -1
        else:
            raise ValueError(f"x is neither increasing nor decreasing : {x}.")
    return direction * float(np.sum(dx * (y[1:] + y[:-1]) / 2.0))


def average_precision(y_true, y_score):
    """picai_eval's AP (metrics.py:336-372): precision set to 0 at threshold 0, then
    ``-sum(diff(recall) * precision[:-1])``."""
    precision, recall, thresholds = precision_recall_curve(y_true, y_score)
    precision[:-1][thresholds == 0] = 0
    return float(-np.sum(np.diff(recall) * np.array(precision)[:-1]))


class Metrics:
    """The reference's ``Metrics`` reduced to what the wrappers log: ``AP``, ``auroc``, ``score``
    from ``lesion_results`` ({case: [(is_lesion, confidence, overlap)]}), ``case_target`` and
    ``case_pred`` ({case: value}); cases in sorted order."""

    def __init__(self, lesion_results, case_target, case_pred):
        self.subject_list = sorted(lesion_results)
        self.lesion_results = {k: lesion_results[k] for k in self.subject_list}
        self.case_target = {k: case_target[k] for k in self.subject_list}
        self.case_pred = {k: case_pred[k] for k in self.subject_list}

    @property
    def lesion_results_flat(self):
        return [r for k in self.subject_list for r in self.lesion_results[k]]

    @property
    def AP(self):
        flat = self.lesion_results_flat
        return average_precision([r[0] for r in flat], [r[1] for r in flat])

    @property
    def auroc(self):
        fpr, tpr, _ = roc_curve([self.case_target[k] for k in self.subject_list],
                                [self.case_pred[k] for k in self.subject_list])
        return auc(fpr, tpr)

    @property
    def score(self):
        return (self.auroc + self.AP) / 2

    @property
    def num_cases(self):
        return len(self.subject_list)


# ---- one case from its packed record ------------------------------------------------------
def case_from_record(rec, n_voxels, min_overlap=0.1):
    """(y_list, case confidence, case target) of one case (eval.py:51-251) from its record
    [N_cand, N_gt, n_pairs, gt counts, cand counts, cand confidences (fp32 bits), pairs x 3]."""
    rec = np.asarray(rec, dtype=np.int32)
    nc, ng, npairs = (int(v) for v in rec[:3])
    o = 3
    gcnt = rec[o:o + ng].astype(np.int64)
    o += ng
    ccnt = rec[o:o + nc].astype(np.int64)
    o += nc
    conf = rec[o:o + nc].view(np.float32).astype(np.float64)
    o += nc
    pairs = rec[o:o + 3 * npairs].reshape(npairs, 3).astype(np.int64)
    y_list = []
    if ng == 0:
        y_list = [(0, float(conf[c]), 0.0) for c in range(nc)]
    else:
        g, c, inter = pairs[:, 0] - 1, pairs[:, 1] - 1, pairs[:, 2]
        union = gcnt[g] + ccnt[c] - inter
        iou = (inter + _EPS) / (union + _EPS)
        keep = ~(iou < min_overlap)
        g, c, iou = g[keep], c[keep], iou[keep]
        rows, rinv = np.unique(g, return_inverse=True)
        cols, cinv = np.unique(c, return_inverse=True)
        sub = np.zeros((len(rows), len(cols)))
        sub[rinv, cinv] = iou
        sub[sub > 0] += 1
        mr, mc = linear_sum_assignment_max(sub)
        ok = sub[mr, mc] > 0
        mr, mc = mr[ok], mc[ok]
        for r, k in zip(mr, mc):
            y_list.append((1, float(conf[cols[k]]), float(sub[r, k] - 1)))
        y_list += [(1, 0.0, 0.0)] * (ng - len(mr))
        sufficient = set(cols.tolist())
        y_list += [(0, float(conf[k]), 0.0) for k in range(nc) if k not in sufficient]
    # np.max(y_det): the largest confidence, or 0 from a background voxel
    case_conf = float(conf.max()) if nc else -np.inf
    if ccnt.sum() < n_voxels:
        case_conf = max(case_conf, 0.0)
    case_target = max((r[0] for r in y_list), default=0)
    return y_list, case_conf, int(case_target)


def _cases(x, name):
    """A list / tuple of device tensors, or a batch tensor, as one [B, D, H, W] tensor."""
    if isinstance(x, (list, tuple)):
        x = torch.stack([torch.as_tensor(t) for t in x]) if len(x) else None
    if x is None:
        raise ValueError(f"{name}: no cases")
    if x.dim() != 4:
        raise NotImplementedError(
            f"{name}: every case must be one 3-D volume, got a batch of shape {tuple(x.shape)}; the "
            "reference labels with a 3x3x3 structure, which scipy rejects on any other rank "
            "('structure and input must have equal rank')")
    return x


class PicaiEval:
    """Accumulator of the PI-CAI evaluation of an epoch: ``update(pred, y)`` per micro-batch,
    ``compute()`` at the end, ``reset()`` after. ``pred`` and ``y`` are [B, 1, D, H, W] or
    [B, D, H, W] device tensors, raw (the prediction is thresholded at ``threshold`` on the device;
    ``threshold=None`` takes it as a detection map). Each update is one launch sequence and ONE host
    synchronisation (the record sizes); the records themselves are copied asynchronously into pinned
    host memory, and ``compute`` waits for them. State: plain attributes (no buffers).

    ``extract_lesions=True`` is the reference's other route (``get_lesions(x, threshold,
    extract_lesions=True)``, pl.py:76-97, and entrypoints/segmentation/test.py:361-399): every
    prediction goes through ``ops.lesion_candidates`` first (``threshold`` a number, ``"dynamic"`` or
    ``"dynamic-fast"``; the other keywords are those of ``extract_lesion_candidates``) and the
    resulting detection map, whose components carry their peak probability, is evaluated as it is.
    The dynamic mode adds its own synchronisations (one per round plus one)."""

    def __init__(self, min_overlap=0.1, threshold=0.1, extract_lesions=False,
                 min_voxels_detection=10, num_lesions_to_extract=5, dynamic_threshold_factor=2.5,
                 max_prob_round_decimals=None, remove_adjacent_lesion_candidates=True):
        if not 0.1 <= float(min_overlap) <= 1.0:
            raise ValueError(f"PicaiEval: min_overlap must lie in [0.1, 1], got {min_overlap}: the "
                             "device keeps only the (lesion, candidate) pairs with IoU >= 0.1")
        self.min_overlap = float(min_overlap)
        self.threshold = threshold
        self.extract_lesions = bool(extract_lesions)
        self.extract_kwargs = dict(
            min_voxels_detection=min_voxels_detection, num_lesions_to_extract=num_lesions_to_extract,
            dynamic_threshold_factor=dynamic_threshold_factor,
            max_prob_round_decimals=max_prob_round_decimals,
            remove_adjacent_lesion_candidates=remove_adjacent_lesion_candidates)
        if isinstance(threshold, str) and not self.extract_lesions:
            raise ValueError(f"PicaiEval: threshold {threshold!r} needs extract_lesions=True")
        self.reset()

    def reset(self):
        self.records = []        # (pinned int32 record words, sizes, voxels per case)
        self._event = None

    def __len__(self):
        return sum(len(sizes) for _, sizes, _ in self.records)

    def update(self, pred, y):
        pred = pred.detach()
        y = y.detach()
        if pred.dim() == 5 and pred.shape[1] == 1:
            pred = pred.squeeze(1)
        if y.dim() == 5 and y.shape[1] == 1:
            y = y.squeeze(1)
        pred = _cases(pred, "PicaiEval.update")
        y = _cases(y, "PicaiEval.update")
        if pred.shape != y.shape:
            raise ValueError(f"PicaiEval.update: prediction {tuple(pred.shape)} and target "
                             f"{tuple(y.shape)} differ")
        if self.extract_lesions:
            hard_blobs = ops.lesion_candidates(pred, self.threshold, **self.extract_kwargs)[0]
            hdr, out = ops.picai_tables(hard_blobs, y, threshold=None)
        else:
            hdr, out = ops.picai_tables(pred, y, self.threshold)
        h = hdr.cpu().numpy().astype(np.int64)       # the one host synchronisation
        sizes = 3 + h[:, 1] + 2 * h[:, 0] + 3 * h[:, 2]
        total = int(sizes.sum())
        host = torch.empty(total, dtype=torch.int32, pin_memory=True)
        host.copy_(out[:total], non_blocking=True)
        self._event = torch.cuda.Event()
        self._event.record()
        self.records.append((host, sizes, int(np.prod(pred.shape[1:]))))

    def metrics(self):
        """The ``Metrics`` of every case since the last ``reset`` (cases numbered in update order)."""
        if self._event is not None:
            self._event.synchronize()
        lesion_results, case_target, case_pred = {}, {}, {}
        idx = 0
        for host, sizes, nvox in self.records:
            words = host.numpy()
            off = 0
            for s in sizes:
                y_list, conf, target = case_from_record(words[off:off + s], nvox, self.min_overlap)
                lesion_results[idx], case_pred[idx], case_target[idx] = y_list, conf, target
                off += int(s)
                idx += 1
        return Metrics(lesion_results, case_target, case_pred)

    def compute(self):
        """{'AP', 'R' (score), 'AUC'} as floats; with more than one rank, the mean of every rank's
        value (Lightning's ``sync_dist``). ValueError when there is no case (on every rank when any
        rank has none: all of them take part in the reduction first)."""
        empty = len(self) == 0
        vals = [float("nan")] * 3
        if not empty:
            with np.errstate(invalid="ignore", divide="ignore"):
                m = self.metrics()
                vals = [m.AP, m.score, m.auroc]
        dist = torch.distributed
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dev = torch.device("cuda", torch.cuda.current_device())
            t = torch.tensor(vals + [float(empty)], dtype=torch.float64, device=dev)
            dist.all_reduce(t)
            t = t.cpu()
            empty = bool(t[3] > 0)
            vals = (t[:3] / dist.get_world_size()).tolist()
        if empty:
            raise ValueError("PicaiEval.compute: no case was evaluated since the last reset() (on "
                             "this rank or another one)")
        return {"AP": float(vals[0]), "R": float(vals[1]), "AUC": float(vals[2])}


def evaluate(y_det, y_true, min_overlap=0.1, threshold=0.1, extract_lesions=False,
             **extract_kwargs):
    """``picai_eval.evaluate(y_det, y_true, y_det_postprocess_func=get_lesions)`` over lists or
    batches of device tensors (one 3-D volume per case; the cases of a list may differ in shape).
    Returns a ``Metrics``; ValueError for ``min_overlap`` below 0.1. With ``extract_lesions`` it is
    ``evaluate(y_det=[extract_lesion_candidates(p, threshold, ...)[0] for p in y_det], y_true,
    y_det_postprocess_func=None)`` (``extract_kwargs``: see ``PicaiEval``)."""
    acc = PicaiEval(min_overlap=min_overlap, threshold=threshold, extract_lesions=extract_lesions,
                    **extract_kwargs)
    if isinstance(y_det, (list, tuple)) or isinstance(y_true, (list, tuple)):
        dets, trues = list(y_det), list(y_true)
        if len(dets) != len(trues):
            raise ValueError(f"evaluate: {len(dets)} detection maps and {len(trues)} targets")
        k = 0
        while k < len(dets):     # one update per run of consecutive cases of one shape
            e = k + 1
            while (e < len(dets) and dets[e].shape == dets[k].shape
                   and trues[e].shape == trues[k].shape):
                e += 1
            acc.update(_cases(dets[k:e], "evaluate"), _cases(trues[k:e], "evaluate"))
            k = e
    else:
        acc.update(_cases(y_det, "evaluate"), _cases(y_true, "evaluate"))
    return acc.metrics()
