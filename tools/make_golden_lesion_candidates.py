"""Generate tests/golden/lesion_candidates.npz from the REAL reference's
adell_mri/modules/extract_lesion_candidates.py (build host only; the reference tree does not travel
to the GPU machine). The module is loaded by file path (it needs numpy and scipy only); for the
end-to-end cases the vendored picai_eval.evaluate is loaded by the stub recipe of
tools/make_golden_picai.py.

Generated with numpy 2.2.6 and scipy 1.15.3 (the versions are stored in the file too).

Probabilities are stored as uint8 levels k: the map is k / 255 in float32. Outputs are stored as the
index map in the smallest integer type plus the confidence list; the hard map is
``float32(confidence)`` on every voxel of its index (the generator checks that this reproduces the
reference's map, and stores the map itself for the one case where it does not: the whole-volume
candidate stored on top of earlier ones).

Every case asserts on the reference's own output what it is there for, so that a later edit cannot
quietly lose its point.

    python tools/make_golden_lesion_candidates.py
"""
import importlib.util
import json
import os
import sys
import types
import warnings

import numpy as np
import scipy

REF = os.environ.get("ADELL_REFERENCE", "/root/reference")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "lesion_candidates.npz")
S = (20, 24, 28)          # not a multiple of the labelling kernel's 8 x 16 x 32 tiles
L = (40, 48, 72)

sys.dont_write_bytecode = True
warnings.simplefilter("ignore")
_spec = importlib.util.spec_from_file_location(
    "ref_extract_lesion_candidates",
    os.path.join(REF, "adell_mri", "modules", "extract_lesion_candidates.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def load_evaluate():
    for name, path in [("adell_mri", "adell_mri"), ("adell_mri.modules", "adell_mri/modules"),
                       ("adell_mri.modules.segmentation", "adell_mri/modules/segmentation"),
                       ("adell_mri.modules.segmentation.picai_eval",
                        "adell_mri/modules/segmentation/picai_eval")]:
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, path)]
        sys.modules[name] = m
    sys.modules["SimpleITK"] = types.ModuleType("SimpleITK")
    from sklearn import metrics as skm

    import adell_mri.modules.segmentation.picai_eval.metrics as ref_metrics
    from adell_mri.modules.segmentation.picai_eval.eval import evaluate

    def _prc(y_true, probas_pred=None, *, sample_weight=None, **kw):
        return skm.precision_recall_curve(y_true, probas_pred, sample_weight=sample_weight, **kw)

    ref_metrics.precision_recall_curve = _prc
    return evaluate


def to_prob(levels):
    return levels.astype(np.float32) / np.float32(255)


def box(a, z, y, x, value):
    a[z[0]:z[1], y[0]:y[1], x[0]:x[1]] = value


def bump(a, centre, sigma, peak):
    """A smooth blob: level peak * exp(-d^2 / (2 sigma^2)), kept where larger than what is there."""
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in a.shape], indexing="ij")
    d2 = (zz - centre[0]) ** 2 + (yy - centre[1]) ** 2 + (xx - centre[2]) ** 2
    v = np.round(peak * np.exp(-d2 / (2.0 * sigma * sigma))).astype(np.uint8)
    np.maximum(a, v, out=a)


# ---- inputs -------------------------------------------------------------------------------
def inputs():
    rng = np.random.default_rng(20261017)
    out = {}
    a = np.zeros(S, np.uint8)
    bump(a, (5, 6, 7), 2.0, 240)
    bump(a, (14, 17, 20), 1.8, 180)
    bump(a, (5, 18, 8), 1.6, 120)
    bump(a, (15, 5, 21), 1.5, 60)
    out["blobs"] = a
    a = np.zeros(L, np.uint8)
    bump(a, (9, 10, 12), 3.0, 250)
    bump(a, (30, 38, 60), 2.5, 170)
    bump(a, (8, 40, 33), 2.2, 110)
    bump(a, (31, 9, 50), 2.0, 70)
    out["blobs_large"] = a
    # dynamic-fast: thr = (250 / 255) / 2.5, which level 100 equals and level 99 does not reach
    a = np.zeros(S, np.uint8)
    box(a, (3, 7), (3, 8), (3, 9), 100)
    a[5, 5, 5] = 250
    box(a, (12, 16), (12, 17), (14, 20), 99)
    out["thr_equality"] = a
    # 10 voxels (removed), 11 voxels (kept; the 11th joined through a corner), both at level 200
    a = np.zeros(S, np.uint8)
    box(a, (2, 3), (2, 4), (2, 7), 200)
    box(a, (10, 11), (10, 12), (10, 15), 200)
    a[9, 9, 9] = 200
    out["size_10_11"] = a
    # two blobs with the same peak: the earlier one in raster order is taken first
    a = np.zeros(S, np.uint8)
    box(a, (12, 15), (4, 7), (4, 8), 200)
    box(a, (3, 6), (15, 18), (18, 22), 200)
    out["equal_peaks"] = a
    # a core inside a weaker shell, and a distant weaker blob: the shell is the second choice, touches
    # the stored core and is rejected (but removed); the distant blob comes third
    a = np.zeros(S, np.uint8)
    box(a, (3, 9), (3, 9), (3, 9), 90)
    box(a, (4, 8), (4, 8), (4, 8), 250)
    box(a, (14, 17), (16, 19), (20, 23), 80)
    out["adjacent"] = a
    # eight blobs of distinct peaks
    a = np.zeros(L, np.uint8)
    k = 0
    for z in (8, 30):
        for y in (8, 24, 40):
            for x in (12, 36, 60):
                if k < 8:
                    bump(a, (z, y, x), 1.7, 250 - 25 * k)
                k += 1
    out["many_blobs"] = a
    a = np.zeros(S, np.uint8)
    a[10, 11, 12] = 255
    out["hot_voxel"] = a
    a = np.zeros(S, np.uint8)
    box(a, (3, 6), (3, 7), (3, 8), 200)
    a[15, 18, 22] = 100
    out["hot_after_stored"] = a
    out["all_zero"] = np.zeros(S, np.uint8)
    out["below_001"] = rng.integers(0, 3, size=S).astype(np.uint8)       # levels 0..2: < 0.01
    # noisy background around blobs: many small components, most of them too small
    a = (rng.random(S) ** 6 * 120).astype(np.uint8)
    bump(a, (6, 7, 8), 2.0, 230)
    bump(a, (13, 16, 19), 1.8, 160)
    out["noisy"] = a
    return out


DEFAULTS = dict(threshold="dynamic-fast", min_voxels_detection=10, num_lesions_to_extract=5,
                dynamic_threshold_factor=2.5, max_prob_round_decimals=None,
                remove_adjacent_lesion_candidates=True)


def case_list():
    """(case name, input name, keyword overrides)."""
    out = []
    for inp in ("blobs", "blobs_large", "noisy"):
        for tag, thr in (("s01", 0.1), ("s05", 0.5), ("fast", "dynamic-fast"), ("dyn", "dynamic")):
            out.append((f"{inp}_{tag}", inp, dict(threshold=thr)))
        for d in (4, 2):
            for tag, thr in (("s01", 0.1), ("fast", "dynamic-fast"), ("dyn", "dynamic")):
                out.append((f"{inp}_{tag}_r{d}", inp, dict(threshold=thr, max_prob_round_decimals=d)))
    out.append(("thr_equality_fast", "thr_equality", dict(threshold="dynamic-fast")))
    out.append(("thr_equality_dyn", "thr_equality", dict(threshold="dynamic")))
    out.append(("size_10_11_s01", "size_10_11", dict(threshold=0.1)))
    out.append(("size_10_11_dyn", "size_10_11", dict(threshold="dynamic")))
    out.append(("size_10_11_min9", "size_10_11", dict(threshold=0.1, min_voxels_detection=9)))
    out.append(("equal_peaks_dyn", "equal_peaks", dict(threshold="dynamic")))
    out.append(("equal_peaks_fast", "equal_peaks", dict(threshold="dynamic-fast")))
    out.append(("adjacent_dyn", "adjacent", dict(threshold="dynamic")))
    out.append(("adjacent_dyn_keep", "adjacent", dict(threshold="dynamic",
                                                      remove_adjacent_lesion_candidates=False)))
    for n in (2, 5, 8):
        out.append((f"many_blobs_dyn_n{n}", "many_blobs", dict(threshold="dynamic",
                                                               num_lesions_to_extract=n)))
    out.append(("many_blobs_fast", "many_blobs", dict(threshold="dynamic-fast")))
    out.append(("hot_voxel_dyn", "hot_voxel", dict(threshold="dynamic")))
    out.append(("hot_voxel_fast", "hot_voxel", dict(threshold="dynamic-fast")))
    out.append(("hot_after_stored_dyn", "hot_after_stored", dict(threshold="dynamic")))
    out.append(("hot_after_stored_dyn_keep", "hot_after_stored",
                dict(threshold="dynamic", remove_adjacent_lesion_candidates=False)))
    for inp in ("all_zero", "below_001"):
        for tag, thr in (("s01", 0.1), ("fast", "dynamic-fast"), ("dyn", "dynamic")):
            out.append((f"{inp}_{tag}", inp, dict(threshold=thr)))
    out.append(("blobs_dyn_factor4", "blobs", dict(threshold="dynamic", dynamic_threshold_factor=4.0)))
    return out


BATCH4 = ["blobs_dyn", "adjacent_dyn", "hot_voxel_dyn", "all_zero_dyn"]


def reconstruct(indexed, conf):
    hard = np.zeros(indexed.shape, np.float32)
    for i, c in conf:
        hard[indexed == i] = np.float32(c)
    return hard


def self_check(name, levels, kw, hard, conf, indexed):
    """What the case is there for, asserted on the reference's output."""
    def need(ok, what):
        assert ok, f"case {name}: {what}"

    ids = [i for i, _ in conf]
    if name.startswith(("blobs_", "blobs_large_")) and "_r" not in name and "factor" not in name:
        need(len(conf) >= 2, "several candidates")
    if name == "thr_equality_fast":
        need(indexed[3, 3, 3] > 0 and indexed[5, 5, 5] == indexed[3, 3, 3], "the level-100 plateau "
             "is kept at thr = (250/255)/2.5")
        need(not indexed[12:16, 12:17, 14:20].any(), "the level-99 block is dropped")
    if name == "size_10_11_s01":
        need(len(conf) == 1 and indexed[2, 2, 2] == 0 and indexed[10, 10, 10] > 0,
             "10 voxels removed, 11 kept")
        need(int((indexed > 0).sum()) == 11, "the kept component has 11 voxels")
    if name == "size_10_11_min9":
        need(len(conf) == 2, "both kept at min_voxels_detection=9")
    if name == "equal_peaks_dyn":
        need(ids == [1, 2] and conf[0][1] == conf[1][1], "two equal confidences")
        need(indexed[3, 15, 18] == 1 and indexed[12, 4, 4] == 2, "raster order decides")
    if name == "adjacent_dyn":
        need(ids == [1, 2], "core and distant blob stored")
        need(indexed[3, 3, 3] == 0 and indexed[5, 5, 5] == 1 and indexed[15, 17, 21] == 2,
             "the shell is rejected and not counted")
    if name == "adjacent_dyn_keep":
        need(ids == [1, 2, 3] and indexed[3, 3, 3] == 2 and indexed[15, 17, 21] == 3,
             "the shell is stored without the adjacency test")
    if name.startswith("many_blobs_dyn_n"):
        n = int(name.rsplit("n", 1)[1])
        need(len(conf) == n, f"{n} candidates extracted")
    if name == "hot_voxel_dyn":
        need(conf == [(1, 0.0)] and (indexed == 1).all() and not hard.any(),
             "index 1 everywhere with confidence 0")
    if name == "hot_after_stored_dyn":
        need(len(conf) == 1 and set(np.unique(indexed)) == {0, 1}, "ends after one lesion of five")
    if name == "hot_after_stored_dyn_keep":
        need([i for i, _ in conf] == [1, 2] and conf[1][1] == 0.0
             and set(np.unique(indexed)) == {2, 3}, "the whole volume is stored on top")
    if name.startswith(("all_zero_", "below_001_dyn")):
        need(conf == [] and not indexed.any() and not hard.any(), "nothing extracted")
    if name.endswith(("_r4", "_r2")) and "dyn" not in name:
        d = kw["max_prob_round_decimals"]
        need(all(c == np.round(c, d) for _, c in conf), "rounded confidences")
        raw = [float(to_prob(levels)[indexed == i].max()) for i, _ in conf]
        need(any(c != r for (_, c), r in zip(conf, raw)), "rounding changes a value")


def run_reference(levels, kw):
    hard, conf, indexed = ref.extract_lesion_candidates(to_prob(levels), **kw)
    assert hard.dtype == np.float32
    return hard, [(int(i), float(c)) for i, c in conf], indexed


def smallest(indexed):
    m = int(indexed.max()) if indexed.size else 0
    assert indexed.min() >= 0
    return indexed.astype(np.uint8 if m < 256 else np.uint16 if m < 65536 else np.int32)


# ---- end to end ---------------------------------------------------------------------------
def e2e_cases():
    rng = np.random.default_rng(20261018)
    preds, targets = [], []
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in S], indexing="ij")
    for k in range(10):
        p = (rng.random(S) ** 8 * 60).astype(np.uint8)
        t = np.zeros(S, np.uint8)
        n_les = [0, 1, 2, 0, 1, 3, 0, 2, 1, 0][k]
        centres = rng.integers(4, np.array(S) - 4, size=(n_les, 3))
        for j, c in enumerate(centres):
            rad = rng.uniform(2.0, 3.2)
            t[(zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= rad * rad] = 1
            if (k + j) % 3 != 2:                       # every third lesion is missed
                bump(p, tuple(c + rng.integers(-1, 2, size=3)), rad / 1.5,
                     int(rng.integers(170, 256)))
        for _ in range(int(rng.integers(0, 3))):       # false positives
            c = rng.integers(3, np.array(S) - 3, size=3)
            bump(p, tuple(c), 1.8, int(rng.integers(60, 256)))
        preds.append(p)
        targets.append(t)
    return np.stack(preds), np.stack(targets)


def main():
    ins = inputs()
    data = {"numpy_version": np.array(np.__version__), "scipy_version": np.array(scipy.__version__)}
    for k, v in ins.items():
        data[f"in_{k}"] = v
    meta = []
    explicit_hard = []
    for name, inp, over in case_list():
        kw = dict(DEFAULTS, **over)
        hard, conf, indexed = run_reference(ins[inp], kw)
        self_check(name, ins[inp], kw, hard, conf, indexed)
        data[f"{name}_indexed"] = smallest(indexed)
        data[f"{name}_ids"] = np.array([i for i, _ in conf], np.int32)
        data[f"{name}_conf"] = np.array([c for _, c in conf], np.float64)
        if not np.array_equal(reconstruct(indexed, conf).view(np.uint32), hard.view(np.uint32)):
            data[f"{name}_hard"] = hard
            explicit_hard.append(name)
        meta.append({"name": name, "input": inp, "kwargs": kw,
                     "indexed_dtype": str(indexed.dtype)})
    assert explicit_hard == ["hot_after_stored_dyn_keep"], explicit_hard
    names = [m["name"] for m in meta]
    assert all(b in names for b in BATCH4)
    assert len({ins[m["input"]].shape for m in meta if m["name"] in BATCH4}) == 1
    data["cases"] = np.array(json.dumps(meta))
    data["batch4"] = np.array(BATCH4)

    evaluate = load_evaluate()
    preds, targets = e2e_cases()
    data["e2e_levels"] = preds
    data["e2e_target"] = targets
    assert (targets.reshape(len(targets), -1).max(1) == 0).sum() >= 3
    for tag, kw in (("dyn", dict(threshold="dynamic")), ("s05", dict(threshold=0.5))):
        dets = [ref.extract_lesion_candidates(to_prob(p), **kw)[0] for p in preds]
        m = evaluate(y_det=dets, y_true=[t.astype(np.float32) for t in targets],
                     y_det_postprocess_func=None, num_parallel_calls=1, verbose=0)
        rows = []
        for i in range(len(preds)):
            for is_lesion, c, ov in m.lesion_results[i]:
                rows.append((i, float(is_lesion), float(c), float(ov)))
        vals = np.array([m.AP, m.score, m.auroc], np.float64)
        assert np.isfinite(vals).all(), f"e2e {tag}: {vals}"
        y_list = np.array(rows, np.float64).reshape(-1, 4)
        confs = y_list[:, 2]
        assert len(np.unique(confs[confs > 0])) >= 4, f"e2e {tag}: real confidences expected"
        data[f"e2e_{tag}_values"] = vals
        data[f"e2e_{tag}_y_list"] = y_list
        data[f"e2e_{tag}_case_pred"] = np.array([float(m.case_pred[i]) for i in range(len(preds))])
        data[f"e2e_{tag}_case_target"] = np.array([float(m.case_target[i])
                                                   for i in range(len(preds))])
        print(f"e2e {tag}: AP/score/AUROC {vals}, {len(rows)} list entries")
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes): {len(meta)} cases")


if __name__ == "__main__":
    main()
