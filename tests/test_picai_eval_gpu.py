"""PI-CAI evaluation on the device (ops.picai_tables, modules/segmentation/picai_eval.py) against the
reference's fixture (tools/make_golden_picai.py) and the numpy restatement (tests/picai_ref.py), and
through the wrappers' validation / test loops."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from adell_mri_amd.modules.segmentation import picai_eval as pe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import picai_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "picai_eval.npz")


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(GOLDEN))


def _probs(fx):
    return fx["pred_levels"].astype(np.float32) / np.float32(255)


def _same(got, want):
    for g, w in zip(got, want):
        assert (math.isnan(g) and math.isnan(w)) or abs(g - w) < 1e-12, (got, want)


def _values(m):
    with np.errstate(invalid="ignore", divide="ignore"):
        return [m.AP, m.score, m.auroc]


def test_evaluate_reproduces_the_fixture(cuda, fx):
    p = torch.from_numpy(_probs(fx)).to(cuda)
    t = torch.from_numpy(fx["target"]).to(cuda)
    m = pe.evaluate(list(p), list(t))
    y = fx["y_list"]
    for i in range(len(fx["names"])):
        ref = sorted((int(a), float(b), float(c)) for _, a, b, c in y[y[:, 0] == i])
        assert picai_ref.sorted_y_list(m.lesion_results[i]) == ref, fx["names"][i]
        assert m.case_target[i] == fx["case_target"][i] and m.case_pred[i] == fx["case_pred"][i]
    _same(_values(m), fx["values_full"])
    for key in ("benign", "malignant"):
        idx = torch.from_numpy(fx[f"{key}_idx"].astype(np.int64)).to(cuda)
        _same(_values(pe.evaluate(p[idx], t[idx])), fx[f"values_{key}"])


def test_accumulator_over_updates_and_reset(cuda, fx):
    p = torch.from_numpy(_probs(fx)).to(cuda).unsqueeze(1)
    t = torch.from_numpy(fx["target"]).to(cuda).unsqueeze(1)
    acc = pe.PicaiEval()
    for k in range(0, p.shape[0], 3):
        acc.update(p[k:k + 3], t[k:k + 3])
    assert len(acc) == p.shape[0]
    vals = acc.compute()
    _same([vals["AP"], vals["R"], vals["AUC"]], fx["values_full"])
    acc.reset()
    assert len(acc) == 0


def test_tables_are_deterministic_and_match_counts(cuda, fx):
    from adell_mri_amd import ops

    p = torch.from_numpy(_probs(fx)).to(cuda)
    t = torch.from_numpy(fx["target"]).to(cuda)
    h1, o1 = ops.picai_tables(p, t)
    h2, o2 = ops.picai_tables(p, t)
    h1 = h1.cpu().numpy()
    assert np.array_equal(h1, h2.cpu().numpy())
    assert h1[:, 0].tolist() == fx["n_pred"].tolist() and h1[:, 1].tolist() == fx["n_true"].tolist()
    off = 0
    o1, o2 = o1.cpu().numpy(), o2.cpu().numpy()
    for i, (nc, ng, npairs) in enumerate(h1):
        size = 3 + ng + 2 * nc + 3 * npairs
        a, b = o1[off:off + size], o2[off:off + size]
        # counts equal; the pair triples in any order
        assert np.array_equal(a[:3 + ng + 2 * nc], b[:3 + ng + 2 * nc])
        pa = sorted(map(tuple, a[3 + ng + 2 * nc:].reshape(-1, 3)))
        assert pa == sorted(map(tuple, b[3 + ng + 2 * nc:].reshape(-1, 3)))
        gc = np.bincount(fx["labels_true"][i].ravel(), minlength=ng + 1)[1:]
        cc = np.bincount(fx["labels_pred"][i].ravel(), minlength=nc + 1)[1:]
        assert a[3:3 + ng].tolist() == gc.tolist() and a[3 + ng:3 + ng + nc].tolist() == cc.tolist()
        off += size


def test_non_binary_detection_map_confidence(cuda):
    d = torch.zeros((1, 10, 12, 14), device=cuda)
    d[0, 1:3, 1:3, 1:3] = 0.25
    d[0, 1, 1, 1] = 0.75
    d[0, 6:8, 6:8, 6:8] = 0.5
    t = torch.zeros_like(d)
    t[0, 6:8, 6:8, 6:8] = 1
    m = pe.evaluate(d, t, threshold=None)
    assert sorted(m.lesion_results[0]) == [(0, 0.75, 0.0), (1, 0.5, 1.0)]
    assert m.case_pred[0] == 0.75


def _net(cuda, **kw):
    from adell_mri_amd.modules.segmentation.pl import UNetPL

    torch.manual_seed(3)
    return UNetPL(image_key="image", label_key="mask", spatial_dimensions=3, conv_type="regular",
                  link_type="residual", upscale_type="transpose", norm_type="instance", padding=1,
                  dropout_param=0.0, depth=[4, 8], kernel_sizes=[3, 3], strides=[2, 2],
                  in_channels=1, n_classes=2, batch_size=2, **kw).to(cuda)


def _batches(cuda, fx):
    g = torch.Generator().manual_seed(11)
    out = []
    for k in (0, 4, 8):
        x = torch.rand((2, 1, 16, 16, 16), generator=g)
        y = torch.from_numpy(fx["target"][k:k + 2, 2:18, 4:20, 6:22].copy()).unsqueeze(1)
        out.append({"image": x.to(cuda), "mask": y.to(cuda)})
    return out


# fixture cases per batch: (benign_fp, split_lesion), (missed_lesion, truncation),
# (benign_empty, iou_threshold); the truncation case has targets 0.7 / 1.9 / -1.2 / 2.5
_PAIRS = [(0, 2), (3, 6), (1, 7)]


def _stub_step(net):
    """The network replaced by the identity on the image: the batch's image IS the prediction, so
    the loops see the fixture's probability maps (the loss is a constant)."""
    def step(x, y, y_class, x_cond, x_fc):
        return x, None, torch.zeros(1, device=x.device), None
    net.step = step
    for k in ("val_metrics", "test_metrics"):    # their targets must be 0 / 1; these are not
        setattr(net, k, torch.nn.ModuleDict())
    return net


def _fixture_batches(cuda, fx, image="image"):
    p = torch.from_numpy(_probs(fx)).unsqueeze(1)
    t = torch.from_numpy(fx["target"]).unsqueeze(1)
    return [{image: p[list(b)].to(cuda), "mask": t[list(b)].to(cuda)} for b in _PAIRS]


def _ref_values(fx, pairs, rounded=False):
    p, t = _probs(fx), fx["target"]
    return _values(picai_ref.evaluate([p[a] for a, _ in pairs],
                                      [np.round(t[b]) if rounded else t[b] for _, b in pairs]))


def _differ(a, b):
    return any(not (math.isnan(x) and math.isnan(y)) and abs(x - y) > 1e-9 for x, y in zip(a, b))


def test_validate_and_test_steps_pair_as_the_reference(cuda, fx):
    """validation: each micro-batch's raw prediction with its own raw target; test: with the WHOLE
    batch's targets (sic, pl.py:503-509), i.e. micro-batch m of one case pairs with case 0."""
    from adell_mri_amd import trainer

    net = _stub_step(_net(cuda, picai_eval=True))
    net.train_batch_size = 1
    batches = _fixture_batches(cuda, fx)
    own = [(i, i) for b in _PAIRS for i in b]
    whole = [(i, b[0]) for b in _PAIRS for i in b]
    want_val, want_test = _ref_values(fx, own), _ref_values(fx, whole)
    # the checks below can tell the pairings, and raw from rounded targets, apart
    assert _differ(want_val, want_test)
    assert _differ(want_val, _ref_values(fx, own, rounded=True))
    out = trainer.validate_steps(net, batches)
    assert set(out) == {"val_loss", "V_AP", "V_R", "V_AUC"}
    _same([out["V_AP"], out["V_R"], out["V_AUC"]], want_val)
    out = trainer.test_steps(net, batches)
    assert set(out) == {"test_loss", "V_AP", "V_R", "V_AUC"}
    _same([out["V_AP"], out["V_R"], out["V_AUC"]], want_test)
    assert len(net.picai_accumulator()) == 0


def test_semi_supervised_steps_pair_correctly(cuda, fx):
    from adell_mri_amd import trainer
    from adell_mri_amd.modules.semi_supervised_segmentation.pl import UNetContrastiveSemiSL

    net = UNetContrastiveSemiSL(image_key="image", label_key="mask", semi_sl_image_key_1=None,
                                semi_sl_image_key_2=None, spatial_dimensions=3,
                                conv_type="regular", link_type="residual", upscale_type="transpose",
                                norm_type="instance", padding=1, dropout_param=0.0, depth=[4, 8],
                                kernel_sizes=[3, 3], strides=[2, 2], in_channels=1, n_classes=2,
                                batch_size=1, picai_eval=True).to(cuda)
    _stub_step(net)
    batches = _fixture_batches(cuda, fx)
    want = _ref_values(fx, [(i, i) for b in _PAIRS for i in b])
    for run in (trainer.validate_steps, trainer.test_steps):
        out = run(net, batches)
        _same([out["V_AP"], out["V_R"], out["V_AUC"]], want)


def test_brunet_steps_collect_the_whole_batch(cuda, fx):
    from adell_mri_amd import trainer
    from adell_mri_amd.modules.segmentation.pl import BrUNetPL

    net = BrUNetPL(image_keys=["t2", "adc"], label_key="mask", spatial_dimensions=3,
                   conv_type="regular", link_type="residual", upscale_type="transpose",
                   norm_type="instance", padding=1, dropout_param=0.0, depth=[4, 8],
                   kernel_sizes=[3, 3], strides=[2, 2], in_channels=1, n_classes=2, batch_size=1,
                   picai_eval=True).to(cuda)

    def step(x, x_weights, y, y_class, x_cond, x_fc):
        return x[0], None, torch.zeros(1, device=y.device), None
    net.step = step
    for k in ("val_metrics", "test_metrics"):
        setattr(net, k, torch.nn.ModuleDict())
    batches = []
    for b in _fixture_batches(cuda, fx, "t2"):
        n = b["t2"].shape[0]
        batches.append(dict(b, adc=b["t2"], t2_weight=torch.ones(n, device=cuda),
                            adc_weight=torch.ones(n, device=cuda)))
    want = _ref_values(fx, [(i, i) for b in _PAIRS for i in b])
    for run in (trainer.validate_steps, trainer.test_steps):
        out = run(net, batches)
        _same([out["V_AP"], out["V_R"], out["V_AUC"]], want)


def test_real_network_leaves_module_state_alone(cuda, fx):
    from adell_mri_amd import trainer

    net = _net(cuda, picai_eval=True)
    batches = _batches(cuda, fx)
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    nbuf = len(list(net.buffers()))
    out = trainer.validate_steps(net, batches)
    assert {"val_loss", "V_IoU", "V_Dice", "V_AP", "V_R", "V_AUC"} == set(out)
    assert list(net.state_dict()) == list(sd) and len(list(net.buffers())) == nbuf
    assert all(torch.equal(v, net.state_dict()[k]) for k, v in sd.items())


def test_evaluate_takes_cases_of_different_shapes(cuda, fx):
    p, t = _probs(fx), fx["target"]
    dets = [torch.from_numpy(p[i]).to(cuda) for i in range(4)]
    trues = [torch.from_numpy(t[i]).to(cuda) for i in range(4)]
    dets[1], trues[1] = dets[1][:, 2:, 3:], trues[1][:, 2:, 3:]      # 20 x 22 x 25
    m = pe.evaluate(dets, trues)
    want = picai_ref.evaluate([d.cpu().numpy() for d in dets], [y.cpu().numpy() for y in trues])
    _same(_values(m), _values(want))
    for i in range(4):
        assert picai_ref.sorted_y_list(m.lesion_results[i]) == picai_ref.sorted_y_list(
            want.lesion_results[i])


def test_non_fp32_inputs_follow_their_own_dtype(cuda):
    from adell_mri_amd import ops

    t = torch.zeros((1, 6, 6, 6), dtype=torch.float64, device=cuda)
    t[0, 1:3, 1:3, 1:3] = 0.9999999999          # astype(int32) -> 0, fp32 would give 1
    t[0, 4:6, 4:6, 4:6] = 1.0
    d = torch.zeros((1, 6, 6, 6), device=cuda)
    d[0, 1:3, 1:3, 1:3] = 0.9
    m = pe.evaluate(d, t)
    assert sorted(m.lesion_results[0]) == [(0, 1.0, 0.0), (1, 0.0, 0.0)]
    x = torch.zeros((5, 5, 5), dtype=torch.float64, device=cuda)
    x[0, 0, 0] = 1e-60                          # 0 in fp32
    x[4, 4, 4] = 0.1 + 1e-12                    # > 0.1 in float64, not in fp32
    lab, n = ops.label_components(x)
    assert int(n) == 2 and int(lab[0, 0, 0]) == 1 and int(lab[4, 4, 4]) == 2
    lab, n = ops.label_components(x, threshold=0.1)
    assert int(n) == 1 and int(lab[4, 4, 4]) == 1


def test_picai_off_keeps_keys(cuda, fx):
    from adell_mri_amd import trainer

    net = _net(cuda)
    batches = _batches(cuda, fx)
    assert set(trainer.validate_steps(net, batches)) == {"val_loss", "V_IoU", "V_Dice"}
    assert set(trainer.test_steps(net, batches)) == {"test_loss", "T_IoU", "T_Pr", "T_F1", "T_Dice"}
    assert net.picai_accumulator() is None


def test_unsupported_wrappers_raise(cuda):
    from adell_mri_amd.modules.segmentation.pl import UNetPL

    net2d = UNetPL(spatial_dimensions=2, depth=[4, 8], kernel_sizes=[3, 3], strides=[2, 2],
                   n_classes=2, picai_eval=True)
    with pytest.raises(NotImplementedError, match="equal rank"):
        net2d.picai_accumulator()
    mc = UNetPL(spatial_dimensions=3, depth=[4, 8], kernel_sizes=[3, 3], strides=[2, 2],
                n_classes=3, picai_eval=True)
    with pytest.raises(NotImplementedError, match="equal rank"):
        mc.picai_accumulator()
