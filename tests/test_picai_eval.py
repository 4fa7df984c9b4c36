"""CPU checks of the PI-CAI evaluation: the numpy restatement (tests/picai_ref.py) reproduces the
reference's fixture (tools/make_golden_picai.py), and the package's host functions (assignment,
AP, AUROC) reproduce its values and, where they can be imported, scipy's and scikit-learn's."""
import os

import numpy as np
import pytest

import picai_ref
from adell_mri_amd.modules.segmentation import picai_eval as pe

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "picai_eval.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def _probs(fx, i):
    return fx["pred_levels"][i].astype(np.float32) / np.float32(255)


def _close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    m = ~np.isnan(a)
    np.testing.assert_allclose(a[m], b[m], rtol=0, atol=1e-12)


def test_fixture_is_complete(fx):
    assert len(fx["names"]) >= 10
    assert fx["values_full"].shape == (3,)
    assert 0 < len(fx["benign_idx"]) < len(fx["names"])


def test_restated_labels_match_scipy_labels(fx):
    for i in range(len(fx["names"])):
        lp, n_p = picai_ref.label(_probs(fx, i) > np.float32(0.1))
        lt, n_t = picai_ref.label(fx["target"][i].astype(np.int32) != 0)
        assert n_p == fx["n_pred"][i] and np.array_equal(lp, fx["labels_pred"][i]), fx["names"][i]
        assert n_t == fx["n_true"][i] and np.array_equal(lt, fx["labels_true"][i]), fx["names"][i]


def test_restated_cases_match_reference(fx):
    y = fx["y_list"]
    for i in range(len(fx["names"])):
        y_list, conf, target = picai_ref.evaluate_case(_probs(fx, i), fx["target"][i])
        ref = [(int(a), float(b), float(c)) for _, a, b, c in y[y[:, 0] == i]]
        assert picai_ref.sorted_y_list(y_list) == sorted(ref), fx["names"][i]
        assert conf == fx["case_pred"][i] and target == fx["case_target"][i], fx["names"][i]


def _values(m):
    with np.errstate(invalid="ignore", divide="ignore"):
        return [m.AP, m.score, m.auroc]


def test_host_metrics_reproduce_reference_values(fx):
    n = len(fx["names"])
    probs = [_probs(fx, i) for i in range(n)]
    _close(_values(picai_ref.evaluate(probs, fx["target"])), fx["values_full"])
    for key in ("benign", "malignant"):
        idx = fx[f"{key}_idx"]
        m = picai_ref.evaluate([probs[i] for i in idx], [fx["target"][i] for i in idx])
        _close(_values(m), fx[f"values_{key}"])
    qi, qp = fx["quirk_idx"], fx["quirk_pairs"]
    m = picai_ref.evaluate([probs[i] for i in qi], [fx["target"][qi[k]] for k in qp])
    _close(_values(m), fx["values_quirk"])


def test_metrics_from_fixture_lists(fx):
    """AP / AUROC / score from the reference's own y_lists and case values."""
    y = fx["y_list"]
    n = len(fx["names"])
    lr = {i: [tuple(r[1:]) for r in y[y[:, 0] == i]] for i in range(n)}
    m = pe.Metrics(lr, dict(enumerate(fx["case_target"])), dict(enumerate(fx["case_pred"])))
    _close(_values(m), fx["values_full"])


def test_case_from_record_handles_every_rule():
    # 2 GT lesions (100 and 50 voxels), 4 candidates: c1 matches g1; c2 lies inside g1 with IoU
    # exactly 0.1 (unmatched, but not an FP); c3 overlaps g2 below 0.1 (FP); c4 nowhere (FP); g2 missed
    gcnt, ccnt = [100, 50], [40, 10, 20, 5]
    conf = np.array([1.0, 1.0, 1.0, 1.0], np.float32).view(np.int32)
    pairs = [(1, 1, 40), (1, 2, 10), (2, 3, 6)]    # IoU 0.4, 0.1, 6 / 64
    rec = [4, 2, 3] + gcnt + ccnt + conf.tolist() + [v for p in pairs for v in p]
    y_list, case_conf, target = pe.case_from_record(np.array(rec, np.int32), n_voxels=1000)
    assert sorted(r[:2] for r in y_list) == [(0, 1.0), (0, 1.0), (1, 0.0), (1, 1.0)]
    assert y_list[0][2] == ((40 + 1e-8) / (100 + 1e-8) + 1) - 1
    assert case_conf == 1.0 and target == 1
    # benign: every candidate an FP; nothing detected: case confidence 0
    y_list, case_conf, target = pe.case_from_record(np.array([0, 0, 0], np.int32), n_voxels=8)
    assert y_list == [] and case_conf == 0.0 and target == 0


def test_assignment_small_cases():
    r, c = pe.linear_sum_assignment_max(np.array([[1.5, 1.2], [1.4, 0.0]]))
    assert r.tolist() == [0, 1] and c.tolist() == [1, 0]
    r, c = pe.linear_sum_assignment_max(np.array([[1.5], [1.9], [0.0]]))
    assert r.tolist() == [1] and c.tolist() == [0]
    r, c = pe.linear_sum_assignment_max(np.zeros((0, 3)))
    assert len(r) == 0


def test_assignment_matches_scipy_on_random_inputs():
    opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(1)
    for _ in range(200):
        n, m = rng.integers(1, 9, size=2)
        a = rng.random((n, m))
        a[a < 0.5] = 0
        a[a > 0] += 1
        r, c = pe.linear_sum_assignment_max(a)
        rs, cs = opt.linear_sum_assignment(a, maximize=True)
        assert abs(a[r, c].sum() - a[rs, cs].sum()) < 1e-12
        assert len(set(r.tolist())) == len(r) and len(set(c.tolist())) == len(c)


def test_curves_match_sklearn_on_random_inputs():
    skm = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(2)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        y = rng.integers(0, 2, n)
        s = np.round(rng.random(n), int(rng.integers(0, 3)))
        p, r, t = pe.precision_recall_curve(y, s)
        ps, rs, ts = skm.precision_recall_curve(y, s)
        np.testing.assert_array_equal(p, ps)
        np.testing.assert_array_equal(r, rs)
        np.testing.assert_array_equal(t, ts)
        with np.errstate(invalid="ignore", divide="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                f, tp, _ = pe.roc_curve(y, s)
                fs, tps, _ = skm.roc_curve(y, s)
                _close(f, fs)
                _close(tp, tps)
                _close([pe.auc(f, tp)], [skm.auc(fs, tps)])


def test_package_does_not_import_scipy_or_sklearn():
    import subprocess
    import sys

    code = ("import sys; import adell_mri_amd.modules.segmentation.picai_eval; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('scipy', 'sklearn')]; "
            "assert not bad, bad")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root)


def test_min_overlap_below_the_device_bound_is_refused():
    with pytest.raises(ValueError, match="min_overlap"):
        pe.PicaiEval(min_overlap=0.05)
    with pytest.raises(ValueError, match="min_overlap"):
        pe.evaluate([], [], min_overlap=0.01)
    assert pe.PicaiEval(min_overlap=0.3).min_overlap == 0.3


def test_compute_without_cases_raises_clearly():
    with pytest.raises(ValueError, match="no case"):
        pe.PicaiEval().compute()
