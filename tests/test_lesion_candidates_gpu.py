"""Lesion-candidate extraction on the device (ops.lesion_candidates, csrc/components.hip, and the
mirror module modules/extract_lesion_candidates.py) against the fixture generated from the real
reference and against the numpy restatement: index maps equal, hard maps equal as bit patterns,
lists equal."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from adell_mri_amd import ops
from adell_mri_amd._lib import AdellHipError
from adell_mri_amd.modules import extract_lesion_candidates as elc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lesion_candidates_ref as lcr  # noqa: E402
from test_lesion_candidates import GOLDEN, expected, probs, same_bits  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def cases(fx):
    return json.loads(str(fx["cases"]))


def table(n, ids, conf, vol=None):
    """[(index, float32 confidence as float)] of one volume from the device table."""
    if vol is not None:
        n, ids, conf = n[vol], ids[vol], conf[vol]
    k = int(n)
    assert not ids[k:].any() and not conf[k:].any()          # the rest of the table is zero
    return [(int(i), float(c)) for i, c in zip(ids[:k].cpu().numpy(), conf[:k].cpu().numpy())]


def painted(conf):
    """The device table holds the value the map is painted with: float32 of the list's float64."""
    return [(i, float(np.float32(c))) for i, c in conf]


def test_ops_reproduces_every_fixture_case(cuda, fx):
    for case in cases(fx):
        x = torch.from_numpy(probs(fx["in_" + case["input"]])).to(cuda)
        want_hard, want_conf, want_indexed = expected(fx, case)
        for _ in range(2):                                   # every call twice: the same bits
            hard, indexed, n, ids, conf = ops.lesion_candidates(x, **case["kwargs"])
            assert hard.dtype == torch.float32 and indexed.dtype == torch.int32
            assert hard.shape == x.shape and indexed.shape == x.shape and n.dim() == 0
            assert np.array_equal(indexed.cpu().numpy(), want_indexed), case["name"]
            assert same_bits(hard.cpu().numpy(), want_hard), case["name"]
            assert table(n, ids, conf) == painted(want_conf), case["name"]


def test_mirror_module_reproduces_every_fixture_case(cuda, fx):
    for case in cases(fx):
        p = probs(fx["in_" + case["input"]])
        want_hard, want_conf, want_indexed = expected(fx, case)
        # a tensor in: tensors out
        hard, conf, indexed = elc.extract_lesion_candidates(torch.from_numpy(p).to(cuda),
                                                            **case["kwargs"])
        assert hard.is_cuda and indexed.is_cuda and indexed.dtype == torch.int32
        assert conf == want_conf, (case["name"], conf, want_conf)
        assert all(type(i) is int and type(c) is float for i, c in conf)
        assert np.array_equal(indexed.cpu().numpy(), want_indexed), case["name"]
        assert same_bits(hard.cpu().numpy(), want_hard), case["name"]
        # numpy in: numpy out, of the reference's dtypes
        hard, conf, indexed = elc.extract_lesion_candidates(p, **case["kwargs"])
        assert isinstance(hard, np.ndarray) and isinstance(indexed, np.ndarray)
        assert str(indexed.dtype) == case["indexed_dtype"], case["name"]
        assert conf == want_conf and np.array_equal(indexed, want_indexed), case["name"]
        assert same_bits(hard, want_hard), case["name"]


def test_static_and_dynamic_functions_by_name(cuda, fx):
    x = torch.from_numpy(probs(fx["in_blobs"])).to(cuda)
    for name, got in (
            ("blobs_s01_r4", elc.extract_lesion_candidates_static(x)),        # defaults: 0.1, 4
            ("blobs_dyn", elc.extract_lesion_candidates_dynamic(x)),
            ("blobs_dyn_r2", elc.extract_lesion_candidates_dynamic(x, max_prob_round_decimals=2))):
        case = [c for c in cases(fx) if c["name"] == name][0]
        want_hard, want_conf, want_indexed = expected(fx, case)
        assert got[1] == want_conf, name
        assert np.array_equal(got[2].cpu().numpy(), want_indexed)
        assert same_bits(got[0].cpu().numpy(), want_hard)
    from adell_mri_amd.modules.segmentation.pl import get_lesions

    case = [c for c in cases(fx) if c["name"] == "blobs_dyn"][0]
    assert same_bits(get_lesions(x, "dynamic", True).cpu().numpy(), expected(fx, case)[0])
    assert torch.equal(get_lesions(x), x > 0.1)


def test_batch_of_four_equals_the_single_runs(cuda, fx):
    by_name = {c["name"]: c for c in cases(fx)}
    batch = [by_name[str(n)] for n in fx["batch4"]]
    kw = batch[0]["kwargs"]
    assert all(c["kwargs"] == kw for c in batch)
    x = torch.from_numpy(np.stack([probs(fx["in_" + c["input"]]) for c in batch])).to(cuda)
    for shape in ((4,), (2, 2)):
        xb = x.view(shape + x.shape[1:])
        hard, indexed, n, ids, conf = ops.lesion_candidates(xb, **kw)
        assert n.shape == shape and ids.shape[:-1] == shape and hard.shape == xb.shape
        hard, indexed = hard.view(x.shape), indexed.view(x.shape)
        n, ids, conf = n.view(4), ids.view(4, -1), conf.view(4, -1)
        for k, c in enumerate(batch):
            want_hard, want_conf, want_indexed = expected(fx, c)
            assert np.array_equal(indexed[k].cpu().numpy(), want_indexed), c["name"]
            assert same_bits(hard[k].cpu().numpy(), want_hard), c["name"]
            assert table(n, ids, conf, k) == painted(want_conf), c["name"]


def _smooth_fields(seed, n, size, cuda):
    """Smooth random probability maps with a few peaks each: coarse noise, trilinear upsampling."""
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((n, 1, size // 8, size // 8, size // 8), generator=g)
    x = torch.nn.functional.interpolate(coarse, size=(size, size, size), mode="trilinear",
                                        align_corners=True)[:, 0]
    x = (x - x.amin()) / (x.amax() - x.amin())
    x = x ** 6 * torch.linspace(1.0, 0.4, n).view(n, 1, 1, 1)
    x[n - 1] *= 0.005                                   # one volume below the stopping threshold
    return x.contiguous().to(cuda)


@pytest.mark.parametrize("size", [64, 128])
def test_random_smooth_fields_against_the_restatement(cuda, size):
    x = _smooth_fields(size, 4, size, cuda)
    xn = x.cpu().numpy()
    runs = [dict(threshold=0.1, max_prob_round_decimals=4), dict(threshold="dynamic-fast"),
            dict(threshold="dynamic"), dict(threshold="dynamic", max_prob_round_decimals=2,
                                            num_lesions_to_extract=12),
            dict(threshold="dynamic", remove_adjacent_lesion_candidates=False,
                 num_lesions_to_extract=3, min_voxels_detection=200)]
    for kw in runs:
        out1 = ops._lesion_candidates(x, **dict(lcr_defaults(), **kw))
        out2 = ops._lesion_candidates(x, **dict(lcr_defaults(), **kw))
        for a, b in zip(out1[:6], out2[:6]):
            assert torch.equal(a, b), kw
        hard, indexed, n, ids, conf, peak, rounds = out1
        most = 0
        for k in range(4):
            want_hard, want_conf, want_indexed = lcr.extract(xn[k], **kw)
            if kw["threshold"] == "dynamic":
                most = max(most, lcr.dynamic.rounds)
            assert np.array_equal(indexed[k].cpu().numpy(), want_indexed), (kw, k)
            assert same_bits(hard[k].cpu().numpy(), want_hard), (kw, k)
            assert table(n, ids, conf, k) == painted(want_conf), (kw, k)
        # the rounds of a batch are those of its slowest volume; none for the static modes
        assert rounds == (most if kw["threshold"] == "dynamic" else None), kw


def lcr_defaults():
    return dict(threshold="dynamic-fast", min_voxels_detection=10, num_lesions_to_extract=5,
                dynamic_threshold_factor=2.5, max_prob_round_decimals=None,
                remove_adjacent_lesion_candidates=True)


def test_half_precision_inputs_are_converted(cuda, fx):
    p = torch.from_numpy(probs(fx["in_blobs"])).to(cuda)
    for dt in (torch.float16, torch.bfloat16):
        x = p.to(dt)
        for thr in ("dynamic", "dynamic-fast", 0.1):
            got = ops.lesion_candidates(x, threshold=thr)
            want = ops.lesion_candidates(x.to(torch.float32), threshold=thr)
            assert got[0].dtype == torch.float32
            assert all(torch.equal(a, b) for a, b in zip(got, want))
    h, conf, idx = elc.extract_lesion_candidates(probs(fx["in_blobs"]).astype(np.float16))
    assert h.dtype == np.float32 and len(conf) >= 1


def test_unsupported_inputs_raise(cuda):
    for dt in (torch.float64, torch.complex64, torch.int64):
        with pytest.raises(TypeError):
            ops.lesion_candidates(torch.zeros((8, 8, 8), dtype=dt, device=cuda))
        with pytest.raises(TypeError):
            elc.extract_lesion_candidates(torch.zeros((8, 8, 8), dtype=dt, device=cuda))
    with pytest.raises(AdellHipError):
        ops.lesion_candidates(torch.zeros((8, 8), device=cuda))
    with pytest.raises(ValueError):
        elc.extract_lesion_candidates(torch.zeros((8, 8), device=cuda))
    with pytest.raises(ValueError):
        ops.lesion_candidates(torch.zeros((8, 8, 8), device=cuda), threshold="static")


def test_labelling_and_tables_are_unchanged(cuda):
    """The labelling sequence gained a predicate and a per-volume switch; the entry points that were
    there keep their results on the PI-CAI fixture."""
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "picai_eval.npz")))
    p = torch.from_numpy(fx["pred_levels"].astype(np.float32) / np.float32(255)).to(cuda)
    t = torch.from_numpy(fx["target"]).to(cuda)
    lab, cnt = ops.label_components(p, threshold=0.1)
    assert np.array_equal(lab.cpu().numpy(), fx["labels_pred"])
    assert cnt.cpu().tolist() == fx["n_pred"].tolist()
    lab, cnt = ops.label_components(torch.trunc(t))
    assert np.array_equal(lab.cpu().numpy(), fx["labels_true"])
    assert cnt.cpu().tolist() == fx["n_true"].tolist()
    hdr, _ = ops.picai_tables(p, t)
    hdr = hdr.cpu().numpy()
    assert hdr[:, 0].tolist() == fx["n_pred"].tolist() and hdr[:, 1].tolist() == fx["n_true"].tolist()
    from adell_mri_amd.modules.segmentation import picai_eval as pe

    m = pe.evaluate(list(p), list(t))
    with np.errstate(invalid="ignore", divide="ignore"):
        got = [m.AP, m.score, m.auroc]
    assert all(abs(g - w) < 1e-12 for g, w in zip(got, fx["values_full"]))
