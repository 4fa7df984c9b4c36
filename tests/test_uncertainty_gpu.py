"""GPU tests of the bootstrap AUC kernel, ``bootstrap_metric``'s fast path, the adaptive-prediction-set
kernel and the wrappers' calibration. Every kernel result is computed twice and compared bit for bit;
the pair counts are integers and are compared exactly."""
import numpy as np
import pytest
import torch

import uncertainty_cases as C
import uncertainty_ref as R

pytestmark = pytest.mark.gpu


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def counts(s, y, rows, cuda):
    """int64 [R, 4] of ``ops.boot_auroc_pairs``, launched twice."""
    from adell_mri_amd import ops

    tables = ops.boot_auroc_tables(dev(s, cuda), dev(y, cuda))
    idx = dev(rows.astype(np.int32), cuda)
    a = ops.boot_auroc_pairs(idx, *tables)
    b = ops.boot_auroc_pairs(idx, *ops.boot_auroc_tables(dev(s, cuda), dev(y, cuda)))
    assert a.dtype == torch.int64 and a.shape == (rows.shape[0], 4) and torch.equal(a, b)
    return a.cpu().numpy()


def binary_metric(s, y, cuda, parts=1):
    from adell_mri_amd import classification_metrics as CM

    metric = CM.BinaryAUROC() if s.ndim == 1 else CM.MulticlassAUROC(s.shape[1])
    for ps, py in zip(np.array_split(s, parts), np.array_split(y, parts)):
        metric.update(dev(ps, cuda), dev(py, cuda))
    return metric


# ---- the pair counts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 31, 32, 33, 64, 65, 300, 2049])
def test_counts_equal_pair_counting(cuda, n):
    """Scores with one decimal: at most eleven tie groups, which cross the 32-bit words of the masks."""
    s, y = C.pair_case(n, "ties")
    for R_ in (1, 3, 100):
        for m in (max(n // 2, 1), n):
            rows = C.resample_rows(n, R_, m)
            got = counts(s, y, rows, cuda)
            want = [R.pair_counts(s[r], y[r]) + (0,) for r in rows.astype(np.int64)]
            assert got.tolist() == [list(w) for w in want], (n, R_, m)


def test_nan_scores_count_as_in_pair_counting(cuda):
    """Every comparison with a NaN is false: a NaN positive counts 0 against every negative, a NaN
    negative 0 against every positive -- what ``cls_auroc_pairs`` counts."""
    from adell_mri_amd import ops

    n = 65
    s, y = C.pair_case(n, "ties")
    s[[0, 7, 31, 32, 64]] = np.nan
    y[[0, 7]], y[[31, 32]] = 1, 0
    rows = np.concatenate([C.resample_rows(n, 3, n // 2), C.resample_rows(n, 3, n // 2, seed=1)])
    rows = np.concatenate([rows, np.arange(n, dtype=np.int32)[None, :n // 2]])
    got = counts(s, y, rows, cuda)
    want = [R.pair_counts(s[r], y[r]) + (0,) for r in rows.astype(np.int64)]
    assert got.tolist() == [list(w) for w in want]
    whole = ops.cls_auroc_pairs(dev(s, cuda), dev(y, cuda)).tolist()
    assert whole == list(R.pair_counts(s, y))


@pytest.mark.parametrize("n", [33, 300])
def test_equal_scores_give_one_half(cuda, n):
    from adell_mri_amd.utils.bootstrap_metrics import bootstrap_auroc_values

    s, y = C.pair_case(n, "equal")
    rows = C.resample_rows(n, 3, n // 2)
    got = counts(s, y, rows, cuda)
    assert got[:, 0].tolist() == (got[:, 1] * got[:, 2]).tolist()
    values = bootstrap_auroc_values(binary_metric(s, y, cuda), dev(rows, cuda))
    assert values.dtype == torch.float64 and values.tolist() == [0.5] * 3


def test_a_resample_without_a_positive_is_nan(cuda):
    from adell_mri_amd.utils.bootstrap_metrics import bootstrap_auroc_values, bootstrap_metric

    n = 65
    s, y = C.pair_case(n, "ties")
    rows = C.resample_rows(n, 3, n // 2)
    y[rows[1]] = 0                                      # row 1 selects negatives only
    got = counts(s, y, rows, cuda)
    assert got[1].tolist() == [0, 0, n // 2, 0]
    metric = binary_metric(s, y, cuda)
    values = bootstrap_auroc_values(metric, dev(rows, cuda)).cpu().numpy()
    want = [R.auc(s[r], y[r]) for r in rows.astype(np.int64)]
    assert np.isnan(values[1]) and values[0] == want[0] and values[2] == want[2]
    # ... and reaches the mean and the quantiles, as in the reference's loop
    mean, qs = bootstrap_metric(metric, sample_idxs=torch.from_numpy(rows))
    assert torch.isnan(mean).all() and torch.isnan(qs).all()
    # no positive at all: every resample
    s, y = C.pair_case(n, "nopos")
    assert np.isnan(bootstrap_auroc_values(binary_metric(s, y, cuda), dev(rows, cuda)).cpu().numpy()).all()


def test_multiclass_macro_with_an_out_of_range_label(cuda):
    from adell_mri_amd.utils.bootstrap_metrics import bootstrap_auroc_values

    n, K = 97, 3
    s, y = C.pair_case(n, "ties", classes=K)
    y[11] = 7
    rows = C.resample_rows(n, 5, n // 2)
    rows[0, 0] = 11 if 11 not in rows[0] else rows[0, 0]          # a row that holds the skipped sample
    assert 11 in rows[0]
    y[rows[2]] = np.where(y[rows[2]] == 2, 0, y[rows[2]])         # class 2 has no positive in row 2
    metric = binary_metric(s, y, cuda, parts=2)
    a = bootstrap_auroc_values(metric, dev(rows, cuda))
    b = bootstrap_auroc_values(metric, dev(rows, cuda))
    assert torch.equal(a, b)
    want = np.array([R.macro_auc(s[r], y[r], K) for r in rows.astype(np.int64)])
    # the same fp64 operations in the same order per class; the macro sums three terms
    np.testing.assert_allclose(a.cpu().numpy(), want, rtol=4e-16, atol=0)
    for c in range(K):
        one = R.one_vs_rest(y, c, K)
        got = counts(s[:, c].copy(), one, rows, cuda)
        assert got[:, :3].tolist() == [list(R.pair_counts(s[r, c], one[r])) for r in rows.astype(np.int64)]


def test_duplicate_and_out_of_range_indices_raise(cuda):
    from adell_mri_amd import ops
    from adell_mri_amd.utils.bootstrap_metrics import bootstrap_metric

    n = 64
    s, y = C.pair_case(n, "ties")
    tables = ops.boot_auroc_tables(dev(s, cuda), dev(y, cuda))
    rows = C.resample_rows(n, 4, n // 2)
    rows[2, 5] = rows[2, 9]
    with pytest.raises(ValueError, match=r"twice or one outside \[0, 64\): rows \[2\]"):
        ops.boot_auroc_pairs(dev(rows, cuda), *tables)
    with pytest.raises(ValueError, match="twice"):
        bootstrap_metric(binary_metric(s, y, cuda), sample_idxs=torch.from_numpy(rows))
    for bad in (-1, n, 2 ** 31 - 1):
        rows = C.resample_rows(n, 4, n // 2)
        rows[3, 0] = bad
        with pytest.raises(ValueError, match=r"rows \[3\]"):
            ops.boot_auroc_pairs(dev(rows, cuda), *tables)
    with pytest.raises(ValueError, match="int32"):
        ops.boot_auroc_pairs(dev(rows.astype(np.int64), cuda), *tables)


def test_the_cap_and_the_loop_route_beyond_it(cuda):
    """n = BOOT_MAX_N is the largest bitmask launch (72 KiB of LDS per block); one sample more takes a
    ``cls_auroc_pairs`` per resample and agrees with the same restatement."""
    from adell_mri_amd import ops
    from adell_mri_amd.utils import bootstrap_metrics as B

    for n, route in ((ops.BOOT_MAX_N, "bitmask"), (ops.BOOT_MAX_N + 1, "loop")):
        assert ops.boot_auroc_route(n) == route
        rng = np.random.RandomState(n % 1000)
        s = np.round(rng.rand(n), 3).astype(np.float32)
        y = rng.randint(0, 2, n).astype(np.int64)
        rows = np.stack([rng.permutation(n)[:n // 2] for _ in range(2)]).astype(np.int32)
        want = [list(R.pair_counts_sorted(s[r], y[r])) for r in rows.astype(np.int64)]
        if route == "bitmask":
            assert counts(s, y, rows, cuda)[:, :3].tolist() == want
        else:
            tables = ops.boot_auroc_tables(dev(s, cuda), dev(y, cuda))
            with pytest.raises(ValueError, match="outside"):
                ops.boot_auroc_pairs(dev(rows, cuda), *tables)
            got = B._auroc_counts(dev(s, cuda), dev(y, cuda), dev(rows, cuda), route)
            assert got.cpu().numpy().tolist() == want
        values = B.bootstrap_auroc_values(binary_metric(s, y, cuda), dev(rows, cuda)).cpu().numpy()
        assert values.tolist() == [w[0] / (2.0 * w[1] * w[2]) for w in want]


# ---- bootstrap_metric, end to end -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.BOOT_CASES))
def test_bootstrap_metric_equals_the_reference(cuda, name):
    from adell_mri_amd.utils.bootstrap_metrics import bootstrap_auroc_values, bootstrap_metric

    g, key = C.golden(), "boot_" + name
    n, K, samples, size, seed = C.BOOT_CASES[name]
    s, y = g[key + "_scores"], g[key + "_labels"]
    metric = binary_metric(s, y, cuda, parts=3)
    stored = [t.clone() for t in metric.scores + metric.labels]
    before = metric.compute()
    mean, qs = bootstrap_metric(metric, samples=samples, sample_size=size, seed=seed)
    mean2, qs2 = bootstrap_metric(metric, samples=samples, sample_size=size, seed=seed)
    assert torch.equal(mean, mean2) and torch.equal(qs, qs2)
    assert mean.shape == (1,) and qs.shape == (2, 1) and mean.dtype == qs.dtype == torch.float32
    assert mean.is_cuda and qs.is_cuda
    # an fp64 value rounded to fp32: within one ulp of fp32 of the reference's fp64 result
    for got, want in ((mean.cpu().numpy(), g[key + "_mean"]), (qs.cpu().numpy(), g[key + "_quantiles"])):
        assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    # the stored state is as it was (the reference leaves the last resample there)
    assert len(metric.scores) == 3 and all(torch.equal(a, b) for a, b in
                                           zip(stored, metric.scores + metric.labels))
    assert torch.equal(before, metric.compute())
    # every resample, on the recorded rows
    values = bootstrap_auroc_values(metric, dev(g[key + "_idx"], cuda)).cpu().numpy()
    assert np.abs(values - g[key + "_values"]).max() < 1e-14
    mean3, qs3 = bootstrap_metric(metric, sample_idxs=torch.from_numpy(g[key + "_idx"]))
    assert torch.equal(mean3, mean) and torch.equal(qs3, qs)


# ---- adaptive prediction sets -----------------------------------------------------------------------------------------
def aps_twice(p, y, cuda):
    from adell_mri_amd import functional as HF

    a = HF.aps_cumulative(dev(p, cuda), None if y is None else dev(y, cuda))
    b = HF.aps_cumulative(dev(p, cuda), None if y is None else dev(y, cuda))
    bits = torch.int32                                  # bit for bit: a NaN score equals itself
    assert torch.equal(a[0].view(bits), b[0].view(bits))
    assert y is None or torch.equal(a[1].view(bits), b[1].view(bits))
    return a[0].cpu().numpy(), None if y is None else a[1].cpu().numpy()


@pytest.mark.parametrize("n,K", C.APS_CASES)
def test_aps_kernel_equals_the_reference(cuda, n, K):
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.conformal_prediction import AdaptivePredictionSets

    g, key = C.golden(), C.aps_key(n, K)
    p, y = g[key + "_p"], g[key + "_y"]
    assert HF.aps_route(dev(p, cuda)) == "kernel"
    cum, scores = aps_twice(p, y, cuda)
    assert np.array_equal(cum, g[key + "_cum"]) and np.array_equal(scores, g[key + "_scores"])
    assert np.array_equal(aps_twice(p, None, cuda)[0], cum)
    aps = AdaptivePredictionSets(C.ALPHA)
    aps.update(dev(y[:n // 2], cuda), dev(p[:n // 2], cuda))
    aps.update(dev(y[n // 2:], cuda), dev(p[n // 2:], cuda))
    aps.calculate()
    assert aps.qhat.is_cuda and aps.qhat.item() == g[key + "_qhat"]
    out = aps(dev(p, cuda))
    assert torch.equal(out, aps(dev(p, cuda)))
    assert np.array_equal(out.cpu().numpy(), g[key + "_out"])
    # a calibration row whose score IS qhat holds its own label when predicted again
    at = np.flatnonzero(scores == g[key + "_qhat"])
    assert at.size >= 1 and (out.cpu().numpy()[at, y[at]] == 1).all()


def test_aps_kernel_with_ties_and_bad_labels(cuda):
    from adell_mri_amd import functional as HF

    for n, K in ((41, 7), (9, 64), (6, 1)):
        p, y = C.aps_tied_inputs(n, K)
        y[1], y[4] = -1, K
        cum, scores = aps_twice(p, y, cuda)
        want = R.aps_cumulative(p)
        assert np.array_equal(cum, want)
        ok = (y >= 0) & (y < K)
        assert np.array_equal(scores[ok], want[np.arange(n)[ok], y[ok]]) and np.isnan(scores[~ok]).all()
        for qhat in (0.0, 0.5, 1.0):
            sets = HF.aps_sets(dev(p, cuda), qhat)
            assert sets.dtype == torch.bool and np.array_equal(sets.cpu().numpy(), R.aps_sets(p, qhat))


def test_wide_rows_take_the_composite(cuda):
    from adell_mri_amd import functional as HF
    from adell_mri_amd import ops

    p, y = C.aps_tied_inputs(19, 65)           # multiples of 1 / 16: every order of summation is exact
    assert HF.aps_route(dev(p, cuda)) == "composite"
    with pytest.raises(ValueError, match="65 classes"):
        ops.aps_cumulative(dev(p, cuda))
    cum, scores = aps_twice(p, y, cuda)
    assert np.array_equal(cum, R.aps_cumulative(p)) and np.array_equal(scores, R.aps_scores(p, y))
    assert np.array_equal(HF.aps_sets(dev(p, cuda), 0.75).cpu().numpy(), R.aps_sets(p, 0.75))


# ---- wrappers ---------------------------------------------------------------------------------------------------------
def wrapper_case(name, cuda):
    """(wrapper in eval() mode on the device, n_classes, three batches of four items)."""
    if name == "avg3":
        import ensemble_cases as EC
        from test_ensemble import build_pl

        shape, n_classes = EC.input_shape(name), EC.CONFIGS[name][1]
    else:
        import classification_cases as CC
        from test_classification import build_pl

        shape, n_classes = CC.CONFIGS[name][2], CC.CONFIGS[name][1]["n_classes"]
    torch.manual_seed(5)
    net = build_pl(name)[0].to(cuda).eval()
    g = torch.Generator().manual_seed(3)
    batches = [{"image": torch.randn((4,) + tuple(shape[1:]), generator=g).to(cuda),
                "label": torch.randint(0, n_classes, (4, 1), generator=g)} for _ in range(3)]
    return net, n_classes, batches


@pytest.mark.parametrize("name", ["cat2", "cat3", "vit_cls", "avg3"])
def test_wrapper_calibration(cuda, name):
    from adell_mri_amd.modules.conformal_prediction import AdaptivePredictionSets

    net, K, batches = wrapper_case(name, cuda)
    with pytest.raises(RuntimeError, match="Model needs to be calibrated before calibrated prediction"):
        net.predict_calibrated_step(batches[0], 0)
    net.calibrate(batches)
    assert net.calibrated is True and net.calibration.qhat.is_cuda
    assert not net.calibration.qhat.requires_grad
    out = net.predict_calibrated_step(batches[2], 2)
    assert out.shape == (4, 2 * K) and out.dtype == torch.float32
    assert torch.equal(out, net.predict_calibrated_step(batches[2], 2))
    with torch.no_grad():
        raw = [net.predict_step(b, 0)["prediction"] for b in batches]
    if K == 2:
        probs = [torch.cat([1 - torch.sigmoid(z).reshape(-1, 1), torch.sigmoid(z).reshape(-1, 1)], 1)
                 for z in raw]
    else:
        probs = [torch.softmax(z, -1) for z in raw]
    hand = AdaptivePredictionSets(0.2)
    for b, p in zip(batches, probs):
        hand.update(b["label"].reshape(-1).to(cuda), p)
    hand.calculate()
    assert torch.equal(hand.qhat, net.calibration.qhat)
    assert torch.equal(hand(probs[2]), out)
    sets, p = out.detach()[:, :K], out.detach()[:, K:]
    assert set(sets.unique().tolist()) <= {0.0, 1.0}
    assert bool(sets[torch.arange(4, device=cuda), p.argmax(1)].all())
    # the sets are those of the restatement on the same probabilities
    assert np.array_equal(sets.cpu().numpy() == 1,
                          R.aps_sets(p.cpu().numpy(), net.calibration.qhat.item()))


def test_ordinal_wrapper_refuses_calibration(cuda):
    net, _, batches = wrapper_case("ord4", cuda)
    with pytest.raises(NotImplementedError, match="ordinal"):
        net.calibrate(batches)
    with pytest.raises(RuntimeError, match="calibrated"):
        net.predict_calibrated_step(batches[0], 0)
