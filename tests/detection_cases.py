"""What the detection tests share: builders of the head-level loss cases, the NMS and matching cases,
the anchor-map cases and the two fixture networks of tests/golden/detection_*.npz
(tools/make_detection_golden.py). Everything is drawn from seeded ``numpy.random.RandomState``
streams, so either side rebuilds the same inputs; the fixtures store them as well.

Bounds. ``SUM_BOUND`` = 5e-5 of the largest reference magnitude is the project's bound for fixed-order
fp32 sums; it holds for the loss terms and the gradients of the fused loss wherever the reference's
own fp32-vs-fp64 error on the case (recorded as ``fp32_vs_fp64`` in ``detection_loss.npz``) uses at
most a quarter of it. Where it uses more -- the aspect-ratio term, a squared difference of two
arctangents that cancels -- the bound of that quantity is four times the recorded error (``bound`` in
the fixture, ``loss_bound`` below): never a figure taken from the code under test."""
import os

import numpy as np

from classification_cases import STEP_EPS, STEP_LR, fill, zero_dropout  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SUM_BOUND = 5e-5
MARGIN = 1e-4            # every comparison the code makes stays this far from equality
IOU_THRESHOLD = 0.5

GRIDS = {"unit": (1, 1, 1, 1, 1), "mid": (2, 3, 3, 5, 2), "wide": (1, 2, 9, 9, 5)}   # (B, A, H, W, D)
# name: (grid, positives as a count or a list of (b, h, w, d, a), seed)
LOSS_CASES = {
    "unit_one": ("unit", [(0, 0, 0, 0, 0)], 3),
    "mid_one": ("mid", [(1, 2, 3, 1, 1)], 4),
    # first and last cell of the table, and two anchors positive in one cell
    "mid_corners": ("mid", [(0, 0, 0, 0, 0), (1, 2, 4, 1, 2), (0, 1, 2, 0, 0), (0, 1, 2, 0, 2)], 5),
    "mid_none": ("mid", [], 6),
    "wide_one": ("wide", [(0, 4, 7, 2, 1)], 7),
    "wide_many": ("wide", 70, 8),
}


def loss_case(name):
    """Heads, anchor map, anchors and correction factor of one loss case (fp32 numpy): centre in
    (-1, 1) as behind a tanh (near the target's at the positives), objectness in (0.05, 0.95) as
    behind a sigmoid, the map's objectness in (0.6, 0.95) at the positives and 0 elsewhere."""
    grid, positives, seed = LOSS_CASES[name]
    B, A, H, W, D = GRIDS[grid]
    rs = np.random.RandomState(seed)
    centre = np.tanh(rs.randn(B, 3 * A, H, W, D)).astype(np.float32)
    size = (0.3 * rs.randn(B, 3 * A, H, W, D)).astype(np.float32)
    obj = rs.uniform(0.05, 0.95, (B, A, H, W, D)).astype(np.float32)
    target = np.zeros((B, 1 + 7 * A, H, W, D), np.float32)
    target[:, 0] = rs.randint(0, 3, (B, H, W, D))
    if isinstance(positives, int):
        flat = rs.choice(B * A * H * W * D, positives, replace=False)
        positives = [tuple(int(v) for v in np.unravel_index(f, (B, H, W, D, A))) for f in sorted(flat)]
    for b, h, w, d, a in positives:
        c = 1 + 7 * a
        target[b, c, h, w, d] = rs.uniform(0.6, 0.95)
        target[b, c + 1:c + 4, h, w, d] = rs.uniform(-0.9, 0.9, 3)
        target[b, c + 4:c + 7, h, w, d] = 0.3 * rs.randn(3)
        # the predicted box stays on its target: F.binary_cross_entropy refuses a target ("iou")
        # outside [0, 1], which boxes that miss each other produce (a negative intersection size)
        centre[b, 3 * a:3 * a + 3, h, w, d] = np.clip(
            target[b, c + 1:c + 4, h, w, d] + rs.uniform(-0.1, 0.1, 3), -0.99, 0.99)
    anchors = rs.uniform(4.0, 8.0, (A, 3)).astype(np.float32)
    corr = np.array([8.0, 8.0, 4.0], np.float32)
    return dict(centre=centre, size=size, obj=obj, target=target, anchors=anchors, corr=corr,
                positives=np.array(sorted(positives), np.int64).reshape(-1, 5))


def table_target(grid, kind, seed=0):
    """An anchor map [B, 1 + 7 A, H, W, D] whose objectness channels make ``kind`` cells positive:
    "none", "all" or a count."""
    B, A, H, W, D = GRIDS[grid]
    rs = np.random.RandomState(100 + seed)
    target = rs.uniform(-1, 1, (B, 1 + 7 * A, H, W, D)).astype(np.float32)
    cells = B * A * H * W * D
    n = {"none": 0, "all": cells}.get(kind, kind)
    flags = np.zeros(cells, bool)
    flags[rs.choice(cells, n, replace=False)] = True
    flags = flags.reshape(B, H, W, D, A)
    for a in range(A):
        target[:, 1 + 7 * a] = np.where(flags[..., a], rs.uniform(0.6, 0.9, (B, H, W, D)),
                                        rs.uniform(0.0, 0.4, (B, H, W, D)))
    return target


def box_pair_iou(a, b):
    """calculate_iou of utils.py in fp64 numpy, a [6] against b [n, 6]."""
    inter = np.prod(np.minimum(a[3:], b[:, 3:]) - np.maximum(a[:3], b[:, :3]) + 1, axis=1)
    union = np.prod(a[3:] - a[:3] + 1) + np.prod(b[:, 3:] - b[:, :3] + 1, axis=1) - inter
    return np.where(union > 0, inter / np.where(union > 0, union, 1.0), 0.0)


def nms_case(n, threshold=0.5, score_threshold=0.1):
    """(boxes [n, 6], scores [n]) fp32: clusters of near-duplicates around a few centres, distinct
    scores (a shuffled grid, some below ``score_threshold``). A seed with a pair whose IoU lies
    within ``MARGIN`` of the threshold is rejected."""
    for seed in range(50):
        rs = np.random.RandomState(1000 * n + seed)
        k = max(1, n // 6)
        # (many candidates: the clusters spread out, or some pair of the n^2 / 2 always lands on the margin)
        centres = rs.uniform(5, 60 if n <= 200 else 600, (k, 3))
        which = rs.randint(0, k, n)
        c = centres[which] + rs.uniform(-1.5, 1.5, (n, 3))
        half = rs.uniform(2.0, 4.0, (n, 3))
        boxes = np.concatenate([c - half, c + half], 1).astype(np.float32)
        scores = (0.05 + 0.9 * (rs.permutation(n) + 0.5) / n).astype(np.float32)
        b64 = boxes.astype(np.float64)
        ok = True
        for i in range(n):
            iou32 = box_pair_iou(b64[i], b64[i + 1:])
            if iou32.size and np.abs(iou32 - threshold).min() < MARGIN:
                ok = False
                break
        if ok:
            return boxes, scores
    raise AssertionError(f"nms_case({n}): no seed keeps every IoU away from the threshold")


NMS_SIZES = (1, 2, 64, 65, 130, 1000)
# beyond 4096 candidates the sweep keeps more than one removed-word per lane (64 words of 64 bits each)
NMS_LARGE = (4500, 16384)


def nms_case_large(n, torch, device, threshold=0.5):
    """(boxes, scores) fp32 for many candidates: groups of six on a line along x -- three near-duplicates
    and three more shifted by 3 along y, so two of every six survive -- far enough apart that boxes
    of different groups miss each other along x alone (a negative "IoU"). The margin of every one of
    the n^2 / 2 pairs is checked in fp64 on ``device`` (numpy would take seconds); a seed with a pair
    within ``MARGIN`` of the threshold is rejected."""
    for seed in range(20):
        rs = np.random.RandomState(7 * n + seed)
        group = np.arange(n) // 6
        c = np.stack([30.0 * group, np.full(n, 20.0) + 3.0 * ((np.arange(n) % 6) // 3), np.full(n, 20.0)], 1)
        c = c + rs.uniform(-0.2, 0.2, (n, 3))
        half = rs.uniform(2.9, 3.1, (n, 3))
        boxes = np.concatenate([c - half, c + half], 1).astype(np.float32)
        scores = (0.15 + 0.8 * (rs.permutation(n) + 0.5) / n).astype(np.float32)
        b = torch.from_numpy(boxes).to(device).double()
        vol = (b[:, 3:] - b[:, :3] + 1).prod(1)
        worst = float("inf")
        for lo in range(0, n, 2048):
            a = b[lo:lo + 2048, None]
            inter = (torch.minimum(a[..., 3:], b[None, :, 3:]) - torch.maximum(a[..., :3], b[None, :, :3]) + 1).prod(-1)
            union = vol[lo:lo + 2048, None] + vol[None] - inter
            iou = torch.where(union > 0, inter / union, torch.zeros_like(union))
            worst = min(worst, float((iou - threshold).abs().min()))
        if worst >= MARGIN:
            return boxes, scores
    raise AssertionError(f"nms_case_large({n}): no seed keeps every IoU away from the threshold")


def match_case(seed=0):
    """Per-image predictions and targets for the mAP matching: image 0 ordinary, image 1 with no
    overlap at all, image 2 with no prediction above the score threshold, image 3 with many
    predictions. Scores are shuffled grids (distinct, off the score threshold); the golden tool asserts
    MARGIN for the score order, the threshold and the gap between the two best IoUs of every target.
    Returns (preds, targets): lists of dicts of fp32 / int64 numpy arrays."""
    rs = np.random.RandomState(77 + seed)

    def boxes_around(c, n, jitter, lo=2.0, hi=4.0):
        cc = c + rs.uniform(-jitter, jitter, (n, 3))
        half = rs.uniform(lo, hi, (n, 3))
        return np.concatenate([cc - half, cc + half], 1).astype(np.float32)

    preds, targets = [], []
    t0 = np.concatenate([boxes_around(np.array([10., 10., 10.]), 1, 0), boxes_around(np.array([30., 30., 20.]), 1, 0)])
    p0 = np.concatenate([boxes_around(np.array([10., 10., 10.]), 5, 1.0), boxes_around(np.array([30., 30., 20.]), 4, 1.0)])
    preds.append(dict(boxes=p0, scores=(0.55 + 0.44 * (rs.permutation(9) + 0.5) / 9).astype(np.float32)))
    targets.append(dict(boxes=t0, labels=np.array([1, 0])))
    # no overlap: predictions beyond every target corner (check_overlap needs one axis each way)
    t1 = boxes_around(np.array([50., 50., 50.]), 2, 2.0)
    p1 = boxes_around(np.array([50., 50., 50.]), 3, 1.0)
    p1[:, :3] += 100
    p1[:, 3:] += 100
    preds.append(dict(boxes=p1, scores=(0.55 + 0.44 * (rs.permutation(3) + 0.5) / 3).astype(np.float32)))
    targets.append(dict(boxes=t1, labels=np.array([1, 1])))
    t2 = boxes_around(np.array([20., 20., 20.]), 1, 0)
    p2 = boxes_around(np.array([20., 20., 20.]), 3, 1.0)
    preds.append(dict(boxes=p2, scores=(0.1 + 0.3 * (rs.permutation(3) + 0.5) / 3).astype(np.float32)))
    targets.append(dict(boxes=t2, labels=np.array([1])))
    t3 = boxes_around(np.array([40., 12., 25.]), 3, 6.0)
    p3 = boxes_around(np.array([40., 12., 25.]), 150, 7.0)
    preds.append(dict(boxes=p3, scores=(0.3 + 0.7 * (rs.permutation(150) + 0.5) / 150).astype(np.float32)))
    targets.append(dict(boxes=t3, labels=np.array([1, 0, 1])))
    for p in preds:
        p["labels"] = p["scores"].copy()          # n_classes == 2: the "classes" are the objectness
    return preds, targets


# anchor-map cases: name -> (anchor sizes, input_sh, output_sh, iou_thresh, boxes, classes, shape).
# Box corners are off the anchors' edges and the centre adjustments off 1 (the golden tool asserts a
# margin of MARGIN for every comparison the transform makes)
_ANCH = [[8.0, 8.0, 4.0], [12.0, 10.0, 6.0]]
ANCHOR_CASES = {
    "none": (_ANCH, (16, 16, 8), (2, 2, 2), 0.3, np.zeros((0, 6)), np.zeros((0,)), None),
    "one": (_ANCH, (16, 16, 8), (2, 2, 2), 0.3, np.array([[1.37, 2.21, 0.43, 8.63, 9.12, 3.61]]),
            np.array([1.0]), None),
    # two boxes competing for cell (0, 0, 0)
    "two": (_ANCH, (16, 16, 8), (2, 2, 2), 0.3,
            np.array([[1.37, 2.21, 0.43, 8.63, 9.12, 3.61], [0.58, 1.13, 0.27, 9.41, 8.07, 4.19]]),
            np.array([1.0, 2.0]), None),
    "shape": (_ANCH, (16, 16, 8), (2, 2, 2), 0.3, np.array([[3.13, 4.27, 1.09, 17.21, 18.33, 7.17]]),
              np.array([2.0]), np.array([32, 32, 16])),
    # input_sh / output_sh not an integer
    "ratio": (_ANCH, (16, 16, 8), (3, 3, 3), 0.2,
              np.array([[1.07, 1.52, 0.23, 7.11, 8.03, 2.77], [9.06, 9.53, 4.04, 15.47, 15.02, 7.46]]),
              np.array([1.0, 2.0]), None),
}

# ---- the two fixture networks ----------------------------------------------------------------------
NETS = ("yolo_bin", "yolo_tri")
SHAPE = (2, 1, 16, 16, 8)
OUT_SH = (2, 2, 2)
_STRUCT = dict(backbone_str="resnet", in_channels=1, resnet_structure=[(8, 16, 3, 1), (16, 32, 3, 1)],
               maxpool_structure=[(2, 2, 2), (2, 2, 1)], pyramid_layers=[1, 2, [3, 3, 1]])
NET_CONFIGS = {
    "yolo_bin": dict(_STRUCT, n_classes=2, anchor_sizes=[[14.0, 14.0, 7.0], [16.0, 12.0, 8.0]]),
    "yolo_tri": dict(_STRUCT, n_classes=3, anchor_sizes=[[14.0, 14.0, 7.0]]),
}
STEP_WD = 0.005
# boxes (input voxels, corner format) and classes per item of the batch
# (large boxes and anchors on the 2 x 2 x 2 grid: whatever centre the untrained heads predict, the
# predicted box still meets its target, so the "iou" handed to F.binary_cross_entropy as a target stays
# in [0, 1] -- the reference raises otherwise)
NET_BOXES = [np.array([[1.03, 1.52, 0.47, 14.06, 14.51, 7.02]]),
             np.array([[2.04, 1.07, 0.27, 15.02, 13.05, 7.46], [0.53, 2.52, 1.04, 12.51, 15.47, 7.73]])]
NET_CLASSES = [np.array([1.0]), np.array([2.0, 1.0])]


def net_input():
    g = np.meshgrid(*[np.arange(float(s)) for s in SHAPE[2:]], indexing="ij")
    rs = np.random.RandomState(11)
    x = np.stack([np.stack([np.sin((b + 1) * 0.37 * g[0] + c) * np.cos((b + 2) * 0.23 * g[1])
                            * np.cos(0.45 * g[2] + b) for c in range(SHAPE[1])])
                  for b in range(SHAPE[0])])
    return (x + 0.2 * rs.rand(*SHAPE)).astype(np.float32)


def net_label(name, transform_cls):
    """The anchor maps [B, 1 + 7 A, 2, 2, 2] (fp64) of the batch from ``transform_cls``
    (a ``BBToAdjustedAnchors``)."""
    t = transform_cls(NET_CONFIGS[name]["anchor_sizes"], SHAPE[2:], OUT_SH, 0.3)
    classes = NET_CLASSES if NET_CONFIGS[name]["n_classes"] > 2 else [np.minimum(c, 1.0) for c in NET_CLASSES]
    return np.stack([t(b, c) for b, c in zip(NET_BOXES, classes)])


def net_batch(name, label, torch, device="cpu", dtype=None):
    classes = NET_CLASSES if NET_CONFIGS[name]["n_classes"] > 2 else [np.minimum(c, 1.0) for c in NET_CLASSES]
    dtype = dtype or torch.float32
    return {"image": torch.from_numpy(net_input()).to(device=device, dtype=dtype),
            "label": torch.from_numpy(label).to(device),
            "boxes": [torch.from_numpy(b).to(dtype) for b in NET_BOXES],
            "labels": [torch.from_numpy(c).long() for c in classes]}


def build_net(name, cls, get_adn_fn, dev="cpu", **extra):
    kw = dict(NET_CONFIGS[name])
    net = cls(dev=dev, adn_fn=get_adn_fn(3, "batch", "swish", 0.0), **kw, **extra)
    zero_dropout(net)
    return net


def loss_bound(gold, name, quantity):
    """The recorded bound of ``quantity`` in loss case ``name`` (SUM_BOUND for one the fixture does
    not list: a quantity that is exactly zero in the reference)."""
    names = [str(k) for k in gold[f"{name}:fp32_vs_fp64_names"]]
    if quantity not in names:
        return SUM_BOUND
    return float(gold[f"{name}:bound"][names.index(quantity)])


def fill_net(net, gain):
    """Name-keyed weights for every entry of the state_dict but ``anchor_tensor`` (a frozen Parameter
    that holds the anchor sizes, not a weight)."""
    sd = net.state_dict()
    filled = fill(sd, gain)
    filled["anchor_tensor"] = sd["anchor_tensor"].clone()
    net.load_state_dict(filled)
    return net


class Gold:
    """The records of one fixture file (``files`` and items: what cases.grad_rel_err reads)."""

    def __init__(self, name):
        self._g = np.load(os.path.join(GOLD, f"detection_{name}.npz"), allow_pickle=False)
        self.files = list(self._g.files)

    def __getitem__(self, k):
        return self._g[k]

    def __contains__(self, k):
        return k in self.files
