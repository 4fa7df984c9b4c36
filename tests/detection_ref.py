"""fp64 restatements of the detection arithmetic, written from the formulas and not from the package:
the step loss and its gradients (torch autograd in fp64 over plain index arithmetic), box decoding, NMS
in both modes, the mAP matching, average precision and the anchor map (numpy loops). tests/test_detection.py
pins them to the fixtures recorded from the reference; the GPU tests compare the kernels with them."""
import itertools

import numpy as np
import torch


def positives_of(target, n_anchors, threshold):
    """Rows (b, h, w, d, a) with map objectness > threshold, ordered b, h, w, d, a."""
    obj = np.stack([target[:, 1 + 7 * a] for a in range(n_anchors)], -1)      # [B, H, W, D, A]
    return np.argwhere(obj > threshold)


def ciou(pc, ps, tc, ts):
    """(iou, cpd, ar) of boxes pc -+ ps against tc -+ ts ([n, 3] fp64 torch), sizes with + 1."""
    a_tl, a_br, b_tl, b_br = pc - ps, pc + ps, tc - ts, tc + ts
    a_size, b_size = a_br - a_tl + 1, b_br - b_tl + 1
    inter = (torch.minimum(a_br, b_br) - torch.maximum(a_tl, b_tl) + 1).prod(-1)
    union = a_size.prod(-1) + b_size.prod(-1) - inter
    iou = torch.where(union > 0, inter / union, torch.zeros_like(union))
    cpd = ((pc - tc) ** 2).sum(-1) / ((torch.maximum(a_br, b_br) - torch.minimum(a_tl, b_tl)) ** 2).sum(-1)
    v = 0
    for i, j in itertools.combinations(range(3), 2):
        v = v + 4 / np.pi ** 2 * (torch.atan(a_size[:, i] / a_size[:, j])
                                  - torch.atan(b_size[:, i] / b_size[:, j])) ** 2
    v = v / 3
    return iou, cpd, v * (v / ((1 - iou) + v))


def step_loss(centre, size, obj, target, anchors, corr, threshold=0.5, cut_target=False):
    """The loss of the detection step in fp64 with its gradients. Inputs: numpy arrays in the heads'
    layout. Returns a dict: loss, bce, m_iou (mean(1 - iou)), m_cpd, m_ar, iou, cpd, ar (per positive,
    table order), rows, dcentre, dsize, dobj."""
    A = obj.shape[1]
    rows = positives_of(target, A, threshold)
    c = torch.tensor(centre, dtype=torch.float64, requires_grad=True)
    s = torch.tensor(size, dtype=torch.float64, requires_grad=True)
    o = torch.tensor(obj, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(target, dtype=torch.float64)
    anc = torch.tensor(anchors, dtype=torch.float64).reshape(A, 3)
    cf = torch.tensor(corr, dtype=torch.float64)
    b, h, w, d, a = (torch.from_numpy(rows[:, i]) for i in range(5))
    cell = torch.stack([h, w, d], 1).double()
    k = torch.arange(3)
    pc = (c[b[:, None], 3 * a[:, None] + k, h[:, None], w[:, None], d[:, None]] + cell) * cf
    ps = torch.exp(s[b[:, None], 3 * a[:, None] + k, h[:, None], w[:, None], d[:, None]]) * anc[a] / 2
    tc = (t[b[:, None], 1 + 7 * a[:, None] + 1 + k, h[:, None], w[:, None], d[:, None]] + cell) * cf
    ts = torch.exp(t[b[:, None], 1 + 7 * a[:, None] + 4 + k, h[:, None], w[:, None], d[:, None]]) * anc[a] / 2
    iou, cpd, ar = ciou(pc, ps, tc, ts)
    y = torch.zeros_like(o)
    y[b, a, h, w, d] = iou.detach() if cut_target else iou
    log_p = torch.clamp(torch.log(o), min=-100)
    log_1p = torch.clamp(torch.log1p(-o), min=-100)
    bce = (-(y * log_p + (1 - y) * log_1p)).mean()
    m_iou, m_cpd, m_ar = (1 - iou).mean(), cpd.mean(), ar.mean()
    loss = bce + 0.1 * (m_iou + m_cpd + m_ar)
    # the cross-entropy's own derivative by the objectness is torch's (p - y) / max((1 - p) p, 1e-12) / n
    # wherever the logs are not clamped; autograd of the expression above gives the same there
    gc, gs, go = torch.autograd.grad(loss, [c, s, o], allow_unused=True)
    loss, bce, m_iou, m_cpd, m_ar = (v.detach() for v in (loss, bce, m_iou, m_cpd, m_ar))
    zero = lambda g, ref: np.zeros(ref.shape) if g is None else g.numpy()   # noqa: E731
    return dict(loss=float(loss), bce=float(bce), m_iou=float(m_iou), m_cpd=float(m_cpd), m_ar=float(m_ar),
                iou=iou.detach().numpy(), cpd=cpd.detach().numpy(), ar=ar.detach().numpy(), rows=rows,
                dcentre=zero(gc, centre), dsize=zero(gs, size), dobj=zero(go, obj))


def decode(centre, size, obj, cls, anchors, corr=None):
    """Per image (boxes [n, 6], scores [n], classes [n, C] or [n]) of the cells with objectness > 0.5
    in (h, w, d, a) order, fp64."""
    B, A = obj.shape[:2]
    anchors = np.asarray(anchors, np.float64).reshape(A, 3)
    corr = np.ones(3) if corr is None else np.asarray(corr, np.float64)
    out = []
    for b in range(B):
        o = np.stack([obj[b, a] for a in range(A)], -1)
        rows = np.argwhere(o > 0.5)
        boxes, scores, classes = [], [], []
        for h, w, d, a in rows:
            sz = anchors[a] * np.exp(size[b, 3 * a:3 * a + 3, h, w, d].astype(np.float64))
            c = (centre[b, 3 * a:3 * a + 3, h, w, d].astype(np.float64) + np.array([h, w, d])) * corr
            boxes.append(np.concatenate([c - sz / 2, c + sz / 2]))
            scores.append(float(obj[b, a, h, w, d]))
            classes.append(float(obj[b, a, h, w, d]) if cls is None else cls[b, :, h, w, d].astype(np.float64))
        out.append((np.array(boxes).reshape(-1, 6), np.array(scores), np.array(classes)))
    return out


def overlap(a, b):
    """check_overlap(a [6], b [n, 6])."""
    return np.logical_and((a[3:] > b[:, :3]).any(1), (a[:3] < b[:, 3:]).any(1))


def iou_of(a, b):
    inter = np.prod(np.minimum(a[3:], b[:, 3:]) - np.maximum(a[:3], b[:, :3]) + 1, axis=1)
    union = np.prod(a[3:] - a[:3] + 1) + np.prod(b[:, 3:] - b[:, :3] + 1, axis=1) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


def nms(boxes, scores, score_threshold, iou_threshold=0.5, suppress=False):
    """Indices kept, in descending score order. ``suppress=False``: the reference as written (nothing
    is suppressed); True: the greedy sweep."""
    boxes, scores = np.asarray(boxes, np.float64), np.asarray(scores, np.float64)
    idx = np.nonzero(scores > score_threshold)[0]
    idx = idx[np.argsort(scores[idx], kind="stable")[::-1]]
    if not suppress:
        return idx
    gone = np.zeros(idx.size, bool)
    for i in range(idx.size):
        if gone[i]:
            continue
        rest = np.arange(i + 1, idx.size)
        rest = rest[~gone[rest]]
        if rest.size == 0:
            continue
        a, b = boxes[idx[i]], boxes[idx[rest]]
        gone[rest[overlap(a, b) & (iou_of(a, b) > iou_threshold)]] = True
    return idx[~gone]


def match(pred_boxes, pred_scores, target_boxes, score_threshold=0.5):
    """(best [T], iou [T], any overlap, order): per target box the best of the predictions above the
    score threshold in ascending score order (``order``: their original indices), lowest index on a
    tie; predictions that do not overlap count as IoU 0."""
    pred_boxes = np.asarray(pred_boxes, np.float64)
    pred_scores = np.asarray(pred_scores, np.float64)
    order = np.nonzero(pred_scores > score_threshold)[0]
    order = order[np.argsort(pred_scores[order], kind="stable")]
    pb = pred_boxes[order]
    T = len(target_boxes)
    arr = np.zeros((T, len(pb)))
    any_hit = False
    for i in range(T):
        a = np.asarray(target_boxes[i], np.float64)
        if len(pb):
            ov = overlap(a, pb)
            arr[i, ov] = iou_of(a, pb[ov])
            any_hit = any_hit or bool(ov.any())
    if len(pb) == 0:
        return np.full(T, -1), np.zeros(T), False, order
    best = arr.argmax(1)
    return best, arr[np.arange(T), best], any_hit, order


def average_precision(scores, labels):
    """Binary AP: sum over the distinct thresholds (descending) of (R_n - R_{n-1}) P_n."""
    scores, labels = np.asarray(scores, np.float64), np.asarray(labels).astype(bool)
    P = labels.sum()
    if P == 0:
        return float("nan")
    ap, prev_r = 0.0, 0.0
    for thr in sorted(set(scores.tolist()), reverse=True):
        sel = scores >= thr
        tp = (labels & sel).sum()
        r, p = tp / P, tp / sel.sum()
        ap += (r - prev_r) * p
        prev_r = r
    return float(ap)


def average_precision_multiclass(scores, labels, C):
    labels = np.asarray(labels)
    vals = [average_precision(np.asarray(scores)[:, c], labels == c) for c in range(C) if (labels == c).any()]
    return float(np.mean(vals)) if vals else float("nan")


def anchor_map(anchor_sizes, input_sh, output_sh, thresh, boxes, classes, shape=None):
    """The anchor map [1 + 7 A, *output_sh] cell by cell."""
    anchor_sizes = [np.asarray(a, np.float64) for a in anchor_sizes]
    output_sh = np.asarray(output_sh)
    rel_anchor = np.asarray(input_sh) / output_sh
    rel = rel_anchor if shape is None else np.asarray(shape) / output_sh
    out = np.zeros([1 + 7 * len(anchor_sizes), *output_sh])
    boxes = np.asarray(boxes, np.float64).reshape(-1, 6)
    for i in range(boxes.shape[0]):
        lo, hi = boxes[i, :3] / rel, boxes[i, 3:] / rel
        sz, ctr = hi - lo, (lo + hi) / 2
        bb_vol = np.prod(sz + 1 / rel)
        for ai, anc in enumerate(anchor_sizes):
            hf = anc / rel_anchor / 2
            adim = (0 + hf + 0.5) - (0 - hf + 0.5)
            inter = np.prod(np.minimum(sz, adim) + 1 / rel)
            iou = inter / (np.prod(adim) + bb_vol - inter)
            if not iou > thresh:
                continue
            for cell in itertools.product(*[range(s) for s in output_sh]):
                c = np.array(cell, np.float64)
                if not (np.all(c + hf + 0.5 > lo) and np.all(c - hf + 0.5 < hi)):
                    continue
                adj = ctr - (c + 0.5)
                if not np.all(np.abs(adj) < 1):
                    continue
                if iou > out[(1 + 7 * ai,) + cell]:
                    out[(slice(1 + 7 * ai, 8 + 7 * ai),) + cell] = np.concatenate([[iou], adj, np.log(sz / adim)])
                    out[(0,) + cell] = classes[i]
    return out
