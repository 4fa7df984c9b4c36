"""numpy restatement of the reference's PI-CAI route for the tests: scipy.ndimage.label with the full
3x3x3 structure (vectorised union-find: hook every root onto its smallest neighbouring root, then
pointer-jump, until no edge joins two sets; components numbered in the raster order of their first
voxel), and picai_eval's evaluate_case (eval.py:51-251) with full-volume masks and a dense IoU
matrix. The assignment and the AP / AUROC curves are the package's host functions, checked against
the fixture and against scipy / scikit-learn on their own."""
import numpy as np

from adell_mri_amd.modules.segmentation.picai_eval import linear_sum_assignment_max

_OFFSETS = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dz, dy, dx) < (0, 0, 0)]


def label(mask):
    """(labels int32, count) of a 3-D boolean mask, as ndimage.label(mask, np.ones((3, 3, 3)))."""
    mask = np.asarray(mask, dtype=bool)
    assert mask.ndim == 3
    D, H, W = mask.shape
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    A, B = [], []
    for dz, dy, dx in _OFFSETS:
        # v in v_reg, its backward neighbour n = v + offset (a smaller index) in n_reg
        v_reg = tuple(slice(max(0, -d), s - max(0, d)) for d, s in zip((dz, dy, dx), (D, H, W)))
        n_reg = tuple(slice(max(0, -d) + d, s - max(0, d) + d) for d, s in zip((dz, dy, dx), (D, H, W)))
        both = mask[v_reg] & mask[n_reg]
        A.append(idx[v_reg][both])
        B.append(idx[n_reg][both])
    A = np.concatenate(A) if A else np.zeros(0, np.int64)
    B = np.concatenate(B) if B else np.zeros(0, np.int64)
    parent = idx.ravel().copy()
    while True:
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
        ra, rb = parent[A], parent[B]
        diff = ra != rb
        if not diff.any():
            break
        hi = np.maximum(ra, rb)[diff]
        lo = np.minimum(ra, rb)[diff]
        np.minimum.at(parent, hi, lo)
    flat = mask.ravel()
    roots = flat & (parent == idx.ravel())
    number = np.cumsum(roots).astype(np.int32)
    out = np.where(flat, number[parent], 0).astype(np.int32).reshape(mask.shape)
    return out, int(roots.sum())


def evaluate_case(y_det, y_true, min_overlap=0.1, threshold=0.1):
    """(y_list, case confidence, case target) of one case: the reference's evaluate_case with
    get_lesions (y_det > threshold) as the detection-map post-processing."""
    y_true = np.asarray(y_true).astype(np.int32)
    det = np.asarray(y_det, dtype=np.float32) > np.float32(threshold)
    lab_p, n_p = label(det)
    conf = [1.0] * n_p
    y_list = []
    if not y_true.any():
        y_list = [(0, c, 0.0) for c in conf]
    else:
        lab_t, n_t = label(y_true != 0)
        ov = np.zeros((n_t, n_p))
        for g in range(n_t):
            gm = lab_t == g + 1
            for c in range(n_p):
                pm = lab_p == c + 1
                inter = float(np.sum(pm[gm]))
                den = float(np.sum(pm)) + float(np.sum(gm)) - inter
                ov[g, c] = (inter + 1e-8) / (den + 1e-8)
        ov[ov < min_overlap] = 0
        ov[ov > 0] += 1
        rows, cols = linear_sum_assignment_max(ov)
        keep = ov[rows, cols] > 0
        rows, cols = rows[keep], cols[keep]
        for r, c in zip(rows, cols):
            y_list.append((1, conf[c], ov[r, c] - 1))
        y_list += [(1, 0.0, 0.0)] * (n_t - len(rows))
        suff = (ov > 0).any(axis=0)
        y_list += [(0, conf[c], 0.0) for c in range(n_p) if not suff[c]]
    case_conf = float(det.max()) if det.size else 0.0
    return y_list, case_conf, max((r[0] for r in y_list), default=0)


def evaluate(y_det, y_true, min_overlap=0.1, threshold=0.1):
    """Metrics of the package (AP / AUROC / score over the restated y_lists)."""
    from adell_mri_amd.modules.segmentation.picai_eval import Metrics

    lr, ct, cp = {}, {}, {}
    for i, (p, t) in enumerate(zip(y_det, y_true)):
        lr[i], cp[i], ct[i] = evaluate_case(p, t, min_overlap, threshold)
    return Metrics(lr, ct, cp)


def sorted_y_list(y_list):
    return sorted((int(a), float(b), float(c)) for a, b, c in y_list)
