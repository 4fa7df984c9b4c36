"""Lesion-candidate extraction without a GPU: the numpy restatement (tests/lesion_candidates_ref.py)
against the fixture generated from the real reference (tools/make_golden_lesion_candidates.py) and,
where scipy imports, against scipy; the API surface; the fixture's completeness."""
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lesion_candidates_ref as lcr  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "lesion_candidates.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def cases(fx):
    return json.loads(str(fx["cases"]))


def probs(levels):
    return levels.astype(np.float32) / np.float32(255)


def expected(fx, case):
    """(hard float32, [(index, confidence)], indexed int64) of a fixture case."""
    name = case["name"]
    indexed = fx[f"{name}_indexed"].astype(np.int64)
    conf = [(int(i), float(c)) for i, c in zip(fx[f"{name}_ids"], fx[f"{name}_conf"])]
    if f"{name}_hard" in fx:
        hard = fx[f"{name}_hard"]
    else:
        hard = np.zeros(indexed.shape, np.float32)
        for i, c in conf:
            hard[indexed == i] = np.float32(c)
    return hard, conf, indexed


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_restatement_reproduces_every_fixture_case(fx):
    for case in cases(fx):
        hard, conf, indexed = lcr.extract(probs(fx["in_" + case["input"]]), **case["kwargs"])
        want_hard, want_conf, want_indexed = expected(fx, case)
        assert np.array_equal(indexed, want_indexed), case["name"]
        assert conf == want_conf, (case["name"], conf, want_conf)
        assert same_bits(hard, want_hard), case["name"]


def _smooth(rng, shape):
    coarse = rng.random(tuple(s // 4 + 2 for s in shape))
    x = coarse
    for ax, s in enumerate(shape):
        pos = np.linspace(0, x.shape[ax] - 1, s)
        lo = np.floor(pos).astype(int)
        hi = np.minimum(lo + 1, x.shape[ax] - 1)
        w = (pos - lo).reshape([-1 if a == ax else 1 for a in range(3)])
        x = np.take(x, lo, axis=ax) * (1 - w) + np.take(x, hi, axis=ax) * w
    return (x ** 4).astype(np.float32)


def test_restatement_equals_scipy_on_random_maps():
    pytest.importorskip("scipy")
    from scipy import ndimage

    rng = np.random.default_rng(5)
    st = np.ones((3, 3, 3))
    for shape in ((12, 14, 18), (20, 24, 28)):
        x = _smooth(rng, shape)
        for thr in (0.05, 0.2):
            for d in (None, 3):
                hard, conf, indexed = lcr.static(x, thr, 10, d)
                clipped = x.copy()
                clipped[x < thr] = 0
                lab, n = ndimage.label(clipped, structure=st)
                want_conf = []
                want_idx = lab.copy()
                want_hard = np.zeros_like(x)
                for i in range(1, n + 1):
                    m = lab == i
                    if m.sum() <= 10:
                        want_idx[m] = 0
                        continue
                    p = np.max(m.astype(np.int32) * clipped)
                    p = np.round(p, d) if d is not None else p
                    want_hard[m] = p
                    want_conf.append((i, float(p)))
                assert np.array_equal(indexed, want_idx) and conf == want_conf
                assert same_bits(hard, want_hard)
        # the dynamic mode's adjacency test: binary dilation with the full structure
        mask = rng.random(shape) > 0.97
        assert np.array_equal(lcr._dilate(mask), ndimage.binary_dilation(mask, structure=st))


def test_api_surface_matches_the_reference():
    from adell_mri_amd import ops
    from adell_mri_amd.modules import extract_lesion_candidates as elc
    from adell_mri_amd.modules.segmentation import pl

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items()}

    assert defaults(elc.extract_lesion_candidates_static) == {
        "softmax": inspect.Parameter.empty, "threshold": 0.10, "min_voxels_detection": 10,
        "max_prob_round_decimals": 4}
    assert defaults(elc.extract_lesion_candidates_dynamic) == {
        "softmax": inspect.Parameter.empty, "min_voxels_detection": 10, "num_lesions_to_extract": 5,
        "dynamic_threshold_factor": 2.5, "max_prob_round_decimals": None,
        "remove_adjacent_lesion_candidates": True, "max_prob_failsafe_stopping_threshold": 0.01}
    common = {"threshold": "dynamic-fast", "min_voxels_detection": 10, "num_lesions_to_extract": 5,
              "dynamic_threshold_factor": 2.5, "max_prob_round_decimals": None,
              "remove_adjacent_lesion_candidates": True}
    assert defaults(elc.extract_lesion_candidates) == {"softmax": inspect.Parameter.empty, **common}
    assert defaults(ops.lesion_candidates) == {"x": inspect.Parameter.empty, **common}
    assert defaults(pl.get_lesions) == {"x": inspect.Parameter.empty, "threshold": 0.1,
                                        "extract_lesions": False}


def test_error_types_without_a_gpu():
    import torch

    from adell_mri_amd import ops
    from adell_mri_amd.modules import extract_lesion_candidates as elc

    for bad in (np.zeros((4, 4, 4), np.float64), np.zeros((4, 4, 4), np.int32),
                np.zeros((4, 4, 4), np.complex64)):
        with pytest.raises(TypeError):
            elc.extract_lesion_candidates(bad)
    for dt in (torch.float64, torch.int32, torch.complex64):
        with pytest.raises(TypeError):
            ops.lesion_candidates(torch.zeros((4, 4, 4), dtype=dt))
    with pytest.raises(ValueError):
        ops.lesion_candidates(torch.zeros((4, 4, 4)), threshold="fast")
    with pytest.raises(ValueError):
        elc.extract_lesion_candidates(torch.zeros((4, 4)))
    with pytest.raises(NotImplementedError):
        elc.extract_lesion_candidates_dynamic(torch.zeros((4, 4, 4)),
                                              max_prob_failsafe_stopping_threshold=0.02)
    # no CPU fallback: a host tensor is refused
    from adell_mri_amd._lib import AdellHipError

    with pytest.raises(AdellHipError):
        ops.lesion_candidates(torch.zeros((4, 4, 4)))
    with pytest.raises(AdellHipError):
        ops.lesion_candidates(torch.zeros((4, 4)))


def test_package_imports_neither_scipy_nor_sklearn():
    code = ("import sys; import adell_mri_amd; "
            "import adell_mri_amd.modules.extract_lesion_candidates; "
            "import adell_mri_amd.modules.segmentation.pl; "
            "bad = [m for m in sys.modules if m.split('.')[0] in ('scipy', 'sklearn')]; "
            "assert not bad, bad")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=ROOT)


def test_accumulator_defaults_are_unchanged():
    from adell_mri_amd.modules.segmentation import picai_eval as pe
    from adell_mri_amd.modules.segmentation.pl import UNetBasePL

    acc = pe.PicaiEval()
    assert acc.threshold == 0.1 and acc.extract_lesions is False and acc.min_overlap == 0.1
    assert UNetBasePL.picai_threshold == 0.1 and UNetBasePL.picai_extract_lesions is False
    sig = inspect.signature(pe.evaluate).parameters
    assert sig["threshold"].default == 0.1 and sig["extract_lesions"].default is False
    with pytest.raises(ValueError):
        pe.PicaiEval(threshold="dynamic")        # needs extract_lesions=True
    assert pe.PicaiEval(threshold="dynamic", extract_lesions=True).extract_kwargs == dict(
        min_voxels_detection=10, num_lesions_to_extract=5, dynamic_threshold_factor=2.5,
        max_prob_round_decimals=None, remove_adjacent_lesion_candidates=True)


def test_binding_declares_the_new_entry_points():
    from adell_mri_amd import _lib

    for name in ("adell_lesion_candidates", "adell_lesion_candidates_workspace",
                 "adell_lesion_candidates_capacity"):
        assert name in _lib.SIGNATURES
    h = _lib.lib()
    assert h.adell_lesion_candidates_capacity(20, 24, 28, 2, 10, 5) == 5
    # static: a kept component has at least 11 voxels
    assert h.adell_lesion_candidates_capacity(20, 24, 28, 0, 10, 5) == 20 * 24 * 28 // 11
    assert h.adell_lesion_candidates_capacity(20, 24, 28, 3, 10, 5) == 0
    assert h.adell_lesion_candidates_workspace(4, 20, 24, 28, 2) > h.adell_lesion_candidates_workspace(
        4, 20, 24, 28, 0) > 0


def test_fixture_is_complete(fx):
    cs = cases(fx)
    names = [c["name"] for c in cs]
    assert len(names) == len(set(names)) >= 40
    assert str(fx["numpy_version"]) and str(fx["scipy_version"])
    modes = {}
    for c in cs:
        kw = c["kwargs"]
        thr = kw["threshold"]
        modes.setdefault(thr if isinstance(thr, str) else "static", []).append(c)
        for key in ("indexed", "ids", "conf"):
            assert f"{c['name']}_{key}" in fx, c["name"]
        assert f"in_{c['input']}" in fx and fx["in_" + c["input"]].dtype == np.uint8
    assert all(len(modes[m]) >= 8 for m in ("static", "dynamic", "dynamic-fast"))
    shapes = {fx["in_" + c["input"]].shape for c in cs}
    assert shapes == {(20, 24, 28), (40, 48, 72)}
    assert {c["kwargs"]["max_prob_round_decimals"] for c in cs} == {None, 2, 4}
    assert {c["kwargs"]["num_lesions_to_extract"] for c in cs} >= {2, 5, 8}
    assert any(not c["kwargs"]["remove_adjacent_lesion_candidates"] for c in cs)
    for needed in ("thr_equality_fast", "size_10_11_s01", "equal_peaks_dyn", "adjacent_dyn",
                   "adjacent_dyn_keep", "hot_voxel_dyn", "hot_after_stored_dyn", "all_zero_dyn",
                   "below_001_dyn"):
        assert needed in names
    # the points of the special cases, on the stored results
    assert fx["hot_voxel_dyn_conf"].tolist() == [0.0] and (fx["hot_voxel_dyn_indexed"] == 1).all()
    assert len(fx["adjacent_dyn_ids"]) == 2 and len(fx["adjacent_dyn_keep_ids"]) == 3
    assert len(fx["hot_after_stored_dyn_ids"]) == 1
    batch = [str(n) for n in fx["batch4"]]
    assert len(batch) == 4 and all(b in names for b in batch)
    assert fx["e2e_levels"].shape[0] >= 8 and fx["e2e_levels"].shape == fx["e2e_target"].shape
    empty = (fx["e2e_target"].reshape(len(fx["e2e_target"]), -1).max(1) == 0).sum()
    assert 0 < empty < len(fx["e2e_target"])
    for tag in ("dyn", "s05"):
        assert fx[f"e2e_{tag}_values"].shape == (3,) and np.isfinite(fx[f"e2e_{tag}_values"]).all()
        assert fx[f"e2e_{tag}_y_list"].shape[1] == 4
    assert os.path.getsize(GOLDEN) < 1 << 20
