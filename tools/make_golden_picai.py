"""Generate tests/golden/picai_eval.npz from the REAL reference's picai_eval (build host only; the
reference tree does not travel to the GPU machine).

Import recipe of oracle/make_golden.py: empty package stubs with the right __path__, then the leaf
modules. Three more pieces are needed:
  * an empty ``SimpleITK`` module (the reference imports it for file reading only);
  * ``precision_recall_curve(probas_pred=...)``: scikit-learn 1.7 dropped that keyword (the
    reference pins >= 1.5.0, where it was deprecated), so the name the reference imported is
    rebound to an adapter that passes it on as ``y_score``;
  * the default branch of ``get_lesions`` (modules/segmentation/pl.py:75-97, ``x > threshold``),
    restated in one line because pl.py imports Lightning.

Probabilities are stored as uint8 levels k: the map is k / 255 in float32 on both sides, so the 0.1
threshold is exact (no level lies on it) and the file stays small.

    python tools/make_golden_picai.py
"""
import os
import sys
import types

import numpy as np

REF = os.environ.get("ADELL_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "picai_eval.npz")
SHAPE = (20, 24, 28)      # not a multiple of the labelling kernel's 8 x 16 x 32 tiles

sys.dont_write_bytecode = True
for name, path in [("adell_mri", "adell_mri"), ("adell_mri.modules", "adell_mri/modules"),
                   ("adell_mri.modules.segmentation", "adell_mri/modules/segmentation"),
                   ("adell_mri.modules.segmentation.picai_eval",
                    "adell_mri/modules/segmentation/picai_eval")]:
    m = types.ModuleType(name)
    m.__path__ = [os.path.join(REF, path)]
    sys.modules[name] = m
sys.modules["SimpleITK"] = types.ModuleType("SimpleITK")

from scipy import ndimage  # noqa: E402
from sklearn import metrics as skm  # noqa: E402

import adell_mri.modules.segmentation.picai_eval.metrics as ref_metrics  # noqa: E402
from adell_mri.modules.segmentation.picai_eval.eval import evaluate  # noqa: E402


def _prc(y_true, probas_pred=None, *, sample_weight=None, **kw):
    return skm.precision_recall_curve(y_true, probas_pred, sample_weight=sample_weight, **kw)


ref_metrics.precision_recall_curve = _prc


def get_lesions(x, threshold=0.1):
    return x > threshold     # pl.py:75-97 with extract_lesions=False


def box(a, z, y, x, value):
    a[z[0]:z[1], y[0]:y[1], x[0]:x[1]] = value


def cases():
    """(name, pred uint8 levels, target float32) per case."""
    rng = np.random.default_rng(20261016)
    out = []

    def new():
        return np.zeros(SHAPE, np.uint8), np.zeros(SHAPE, np.float32)

    # benign: false-positive blobs, one touching the border
    p, t = new()
    box(p, (2, 5), (3, 6), (4, 8), 200)
    box(p, (10, 12), (0, 2), (25, 28), 60)       # border, level 60 > 25.5
    box(p, (14, 16), (14, 16), (14, 16), 20)     # below the threshold: no candidate
    out.append(("benign_fp", p, t))
    # benign, nothing detected
    p, t = new()
    box(p, (5, 8), (5, 8), (5, 8), 25)           # 25/255 < 0.1
    out.append(("benign_empty", p, t))
    # one GT lesion split across two candidates (both IoU >= 0.1) plus a distant FP
    p, t = new()
    box(t, (4, 10), (4, 10), (4, 12), 1.0)
    box(p, (4, 10), (4, 10), (4, 7), 180)
    box(p, (4, 10), (4, 10), (9, 12), 140)
    box(p, (15, 18), (18, 21), (20, 24), 90)
    out.append(("split_lesion", p, t))
    # a lesion missed entirely, another found
    p, t = new()
    box(t, (2, 6), (2, 6), (2, 6), 1.0)
    box(t, (12, 16), (14, 18), (18, 22), 1.0)
    box(p, (12, 16), (14, 18), (18, 22), 255)
    out.append(("missed_lesion", p, t))
    # components joined only through an edge or a corner (6-connectivity would split them)
    p, t = new()
    for k in range(6):
        p[3 + k, 3 + k, 3 + k] = 230             # corner chain
        t[3 + k, 3 + k, 3 + k] = 1.0
    for k in range(5):
        p[12, 4 + k, 10 + k] = 120               # edge chain in one plane
    t[12, 4, 10] = 1.0
    t[13, 5, 10] = 1.0                           # edge-joined GT pair
    out.append(("diagonal_joins", p, t))
    # lesions touching the volume border on every side
    p, t = new()
    box(t, (0, 3), (0, 4), (0, 5), 1.0)
    box(p, (0, 3), (0, 4), (0, 5), 255)
    box(t, (17, 20), (20, 24), (24, 28), 1.0)
    box(p, (18, 20), (21, 24), (23, 28), 77)
    out.append(("border", p, t))
    # fractional and negative target values: astype(int32) truncates toward zero
    p, t = new()
    box(t, (2, 6), (2, 6), (2, 6), 0.7)          # -> 0
    box(t, (8, 11), (2, 6), (2, 6), -0.9)        # -> 0
    box(t, (2, 6), (10, 14), (10, 14), 1.9)      # -> 1
    box(t, (12, 15), (12, 15), (20, 24), -1.2)   # -> -1, a lesion
    box(t, (14, 18), (2, 5), (20, 24), 2.5)      # -> 2, a lesion
    box(p, (2, 6), (10, 14), (10, 14), 100)
    box(p, (12, 15), (12, 15), (20, 24), 100)
    box(p, (2, 6), (2, 6), (2, 6), 100)          # on the truncated-away region: FP
    out.append(("truncation", p, t))
    # IoU exactly at 0.1 (kept) and just below it (dropped)
    p, t = new()
    box(t, (2, 7), (2, 7), (2, 6), 1.0)          # 100 voxels
    box(p, (2, 7), (2, 4), (2, 3), 150)          # 10 voxels inside: IoU = 10 / 100
    box(t, (10, 15), (10, 15), (10, 14), 1.0)    # 100 voxels
    box(p, (10, 15), (10, 12), (10, 11), 150)    # 10 inside
    p[9, 9, 9] = 150                             # + 1 outside, corner-joined: IoU = 10 / 101
    out.append(("iou_threshold", p, t))
    # random blobs: several lesions and many candidates
    for r in range(3):
        g = rng.random(SHAPE)
        t = np.zeros(SHAPE, np.float32)
        centres = rng.integers(2, np.array(SHAPE) - 2, size=(4, 3))
        zz, yy, xx = np.meshgrid(*[np.arange(s) for s in SHAPE], indexing="ij")
        for c in centres:
            rad = rng.uniform(1.5, 3.5)
            t[(zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= rad * rad] = 1.0
        prob = np.clip(0.6 * t + 0.45 * g ** 3 - 0.05, 0, 1)
        p = np.round(prob * 255).astype(np.uint8)
        out.append((f"random_{r}", p, t))
    return out


def to_prob(levels):
    return levels.astype(np.float32) / np.float32(255)


def run(preds, trues):
    m = evaluate(y_det=list(preds), y_true=list(trues), y_det_postprocess_func=get_lesions,
                 num_parallel_calls=1, verbose=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        vals = np.array([m.AP, m.score, m.auroc], np.float64)
    return m, vals


def main():
    import warnings

    warnings.simplefilter("ignore")
    cs = cases()
    names = [c[0] for c in cs]
    pred = np.stack([c[1] for c in cs])
    target = np.stack([c[2] for c in cs])
    probs = [to_prob(p) for p in pred]
    st = np.ones((3, 3, 3))
    lab_pred, lab_true, n_pred, n_true = [], [], [], []
    for p, t in zip(probs, target):
        lp, npd = ndimage.label(get_lesions(p), structure=st)
        lt, nt = ndimage.label(t.astype(np.int32), structure=st)
        lab_pred.append(lp.astype(np.int32))
        lab_true.append(lt.astype(np.int32))
        n_pred.append(npd)
        n_true.append(nt)
    m, full = run(probs, target)
    # y_lists, flattened: rows (case, is_lesion, confidence, overlap)
    rows = []
    for i in range(len(cs)):
        for is_lesion, conf, ov in m.lesion_results[i]:
            rows.append((i, float(is_lesion), float(conf), float(ov)))
    y_list = np.array(rows, np.float64).reshape(-1, 4)
    case_target = np.array([m.case_target[i] for i in range(len(cs))], np.float64)
    case_pred = np.array([float(m.case_pred[i]) for i in range(len(cs))], np.float64)
    benign = [i for i in range(len(cs)) if case_target[i] == 0]
    malignant = [i for i in range(len(cs)) if case_target[i] == 1]
    _, benign_vals = run([probs[i] for i in benign], [target[i] for i in benign])
    _, malignant_vals = run([probs[i] for i in malignant], [target[i] for i in malignant])
    # the test-step quirk (pl.py:503-509): a batch of four, micro-batches of two, every micro-batch's
    # predictions zipped with the WHOLE batch's targets -> targets 0, 1, 0, 1
    qi = [2, 3, 8, 9]
    quirk_pairs = [0, 1, 0, 1]
    _, quirk_vals = run([probs[i] for i in qi], [target[qi[k]] for k in quirk_pairs])
    np.savez_compressed(
        OUT, names=np.array(names), pred_levels=pred, target=target,
        labels_pred=np.stack(lab_pred), labels_true=np.stack(lab_true),
        n_pred=np.array(n_pred, np.int32), n_true=np.array(n_true, np.int32), y_list=y_list,
        case_target=case_target, case_pred=case_pred, values_full=full,
        benign_idx=np.array(benign, np.int32), values_benign=benign_vals,
        malignant_idx=np.array(malignant, np.int32), values_malignant=malignant_vals,
        quirk_idx=np.array(qi, np.int32), quirk_pairs=np.array(quirk_pairs, np.int32),
        values_quirk=quirk_vals)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(cs)} cases, AP/score/AUROC {full}, "
          f"benign {benign_vals}, malignant {malignant_vals}, quirk {quirk_vals}")


if __name__ == "__main__":
    main()
