"""PI-CAI evaluation fed by the lesion-candidate extraction: the reference's test route
(extract_lesion_candidates on every prediction, then picai_eval.evaluate(y_det_postprocess_func=None))
against the end-to-end values of tests/golden/lesion_candidates.npz, through ``evaluate`` and through
a wrapper's validation / test loops."""
import math
import os

import numpy as np
import pytest
import torch

from adell_mri_amd.modules.segmentation import picai_eval as pe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lesion_candidates.npz")
MODES = [("dyn", "dynamic"), ("s05", 0.5)]


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def _inputs(fx, cuda):
    p = torch.from_numpy(fx["e2e_levels"].astype(np.float32) / np.float32(255)).to(cuda)
    t = torch.from_numpy(fx["e2e_target"].astype(np.float32)).to(cuda)
    return p, t


def _values(m):
    with np.errstate(invalid="ignore", divide="ignore"):
        return [m.AP, m.score, m.auroc]


def _same(got, want):
    for g, w in zip(got, want):
        assert not math.isnan(w) and abs(g - w) < 1e-12, (got, list(want))


def _sorted(rows):
    return sorted((int(a), float(b), float(c)) for a, b, c in rows)


@pytest.mark.parametrize("tag,threshold", MODES)
def test_evaluate_with_extraction_reproduces_the_fixture(cuda, fx, tag, threshold):
    p, t = _inputs(fx, cuda)
    y = fx[f"e2e_{tag}_y_list"]
    for dets, trues in ((list(p), list(t)), (p, t)):          # a list of cases, and one batch
        m = pe.evaluate(dets, trues, threshold=threshold, extract_lesions=True)
        print(tag, _values(m), fx[f"e2e_{tag}_values"].tolist())
        for i in range(p.shape[0]):
            want = _sorted(r[1:] for r in y[y[:, 0] == i])
            assert _sorted(m.lesion_results[i]) == want, (tag, i)
            assert m.case_pred[i] == fx[f"e2e_{tag}_case_pred"][i]
            assert m.case_target[i] == fx[f"e2e_{tag}_case_target"][i]
        _same(_values(m), fx[f"e2e_{tag}_values"])


def test_extraction_changes_the_operating_points(cuda, fx):
    """The default route gives every candidate confidence 1; the extraction gives real ones."""
    p, t = _inputs(fx, cuda)
    plain = pe.evaluate(p, t)
    assert {r[1] for r in plain.lesion_results_flat} <= {0.0, 1.0}
    real = pe.evaluate(p, t, threshold="dynamic", extract_lesions=True)
    assert len({r[1] for r in real.lesion_results_flat}) > 5


def _net(cuda, stub=True, **kw):
    from adell_mri_amd.modules.segmentation.pl import UNetPL

    torch.manual_seed(3)
    net = UNetPL(image_key="image", label_key="mask", spatial_dimensions=3, conv_type="regular",
                 link_type="residual", upscale_type="transpose", norm_type="instance", padding=1,
                 dropout_param=0.0, depth=[4, 8], kernel_sizes=[3, 3], strides=[2, 2],
                 in_channels=1, n_classes=2, batch_size=2, **kw).to(cuda)
    if not stub:
        return net

    # the network replaced by the identity on the image: the loops see the fixture's maps
    def step(x, y, y_class, x_cond, x_fc):
        return x, None, torch.zeros(1, device=x.device), None
    net.step = step
    return net


def _batches(fx, cuda):
    p, t = _inputs(fx, cuda)
    return [{"image": p[k:k + 2].unsqueeze(1), "mask": t[k:k + 2].unsqueeze(1)}
            for k in range(0, p.shape[0], 2)]


@pytest.mark.parametrize("tag,threshold", MODES)
def test_wrapper_returns_the_fixture_values(cuda, fx, tag, threshold):
    from adell_mri_amd import trainer

    net = _net(cuda, picai_eval=True)
    for k in ("val_metrics", "test_metrics"):
        setattr(net, k, torch.nn.ModuleDict())
    net.picai_extract_lesions = True
    net.picai_threshold = threshold
    # micro-batches of two: validation pairs each with its own targets, and so does the test step
    # here (its whole-batch pairing takes the first two targets of a batch of two)
    batches = _batches(fx, cuda)
    out = trainer.validate_steps(net, batches)
    assert set(out) == {"val_loss", "V_AP", "V_R", "V_AUC"}
    _same([out["V_AP"], out["V_R"], out["V_AUC"]], fx[f"e2e_{tag}_values"])
    out = trainer.test_steps(net, batches)
    assert set(out) == {"test_loss", "V_AP", "V_R", "V_AUC"}
    _same([out["V_AP"], out["V_R"], out["V_AUC"]], fx[f"e2e_{tag}_values"])
    acc = net.picai_accumulator()
    assert acc.extract_lesions is True and acc.threshold == threshold


def test_attribute_off_returns_todays_keys_and_values(cuda, fx):
    from adell_mri_amd import trainer

    p, t = _inputs(fx, cuda)
    want = _values(pe.evaluate(p, t))            # the default route: pred > 0.1, confidence 1
    net = _net(cuda, picai_eval=True)
    for k in ("val_metrics", "test_metrics"):
        setattr(net, k, torch.nn.ModuleDict())
    assert net.picai_extract_lesions is False and net.picai_threshold == 0.1
    out = trainer.validate_steps(net, _batches(fx, cuda))
    assert set(out) == {"val_loss", "V_AP", "V_R", "V_AUC"}
    _same([out["V_AP"], out["V_R"], out["V_AUC"]], want)
    acc = net.picai_accumulator()
    assert acc.extract_lesions is False and acc.threshold == 0.1
    plain = _net(cuda, stub=False)               # picai_eval off: the real network, no PI-CAI keys
    g = torch.Generator().manual_seed(11)
    small = [{"image": torch.rand((2, 1, 16, 16, 16), generator=g).to(cuda),
              "mask": t[k:k + 2, 2:18, 4:20, 6:22].contiguous().unsqueeze(1)} for k in (0, 2)]
    assert set(trainer.validate_steps(plain, small)) == {"val_loss", "V_IoU", "V_Dice"}
    assert set(trainer.test_steps(plain, small)) == {"test_loss", "T_IoU", "T_Pr", "T_F1", "T_Dice"}
    assert plain.picai_accumulator() is None
