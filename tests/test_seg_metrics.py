"""CPU-side checks of the segmentation metrics (adell_mri_amd.metrics, ops.seg_confusion_update):
the metric dicts of the wrappers (reference pl.py:148-187, 655-671), that they add nothing to a
module's parameters / buffers / state_dict, argument errors raised before any launch, and the
fp64 restatement the GPU tests measure against."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from adell_mri_amd import _lib, ops
from adell_mri_amd import metrics as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seg_metrics_ref as ref  # noqa: E402


@pytest.mark.parametrize("bottleneck", [False, True])
def test_metric_dict_keys_binary(bottleneck):
    from adell_mri_amd.modules.segmentation.pl import get_metric_dict

    md = get_metric_dict(2, bottleneck)
    assert list(md) == ["IoU", "Pr", "F1", "Dice"]       # AUC_bn is never built
    assert [type(m) for m in md.values()] == [M.BinaryJaccardIndex, M.BinaryPrecision,
                                              M.BinaryFBetaScore, M.Dice]
    assert md["F1"].beta == 1.0 and all(m.num_classes == 1 for m in md.values())
    md = get_metric_dict(2, bottleneck, ["IoU", "Dice", "AUC_bn"], prefix="V_")
    assert list(md) == ["V_IoU", "V_Dice"]
    md = get_metric_dict(2, bottleneck, None, prefix="T_")
    assert list(md) == ["T_IoU", "T_Pr", "T_F1", "T_Dice"]


@pytest.mark.parametrize("bottleneck", [False, True])
def test_metric_dict_keys_multiclass(bottleneck):
    from adell_mri_amd.modules.segmentation.pl import get_metric_dict

    md = get_metric_dict(3, bottleneck, prefix="T_")
    assert list(md) == ["T_IoU", "T_Pr", "T_F1", "T_Dice"]
    assert [type(m) for m in md.values()] == [M.MulticlassJaccardIndex, M.MulticlassPrecision,
                                              M.MulticlassFBetaScore, M.MulticlassDice]
    assert all(m.num_classes == 3 and m.average == "macro" for m in md.values())
    assert list(get_metric_dict(3, bottleneck, ["IoU", "Dice", "AUC_bn"], "V_")) == ["V_IoU", "V_Dice"]
    assert isinstance(get_metric_dict(3, bottleneck, dev="cpu"), dict)


def _wrappers():
    from adell_mri_amd.modules.activations import activation_factory
    from adell_mri_amd.modules.segmentation.pl import (BrUNetPL, SWINUNetPL, UNetPL, UNETRPL,
                                                       UNetPlusPlusPL)
    from adell_mri_amd.modules.semi_supervised_segmentation.pl import UNetContrastiveSemiSL
    from cases import SWIN_CASES, UNET_CASES, UNETPP_CASES, UNETR_CASES

    def kw(d):
        d = copy.deepcopy(d)
        d["activation_fn"] = activation_factory[d["activation_fn"]]
        return d

    unet = kw(UNET_CASES["unet3d_cfg2_small"])
    return {
        "UNetPL": lambda: UNetPL(**unet),
        "UNetPL_bn": lambda: UNetPL(**dict(unet, bottleneck_classification=True)),
        "UNETRPL": lambda: UNETRPL(**kw(UNETR_CASES["unetr3d_small"])),
        "SWINUNetPL": lambda: SWINUNetPL(**kw(SWIN_CASES["swinunet3d_small"])),
        "UNetPlusPlusPL": lambda: UNetPlusPlusPL(**kw(UNETPP_CASES["unetpp3d_small"])),
        "BrUNetPL": lambda: BrUNetPL(image_keys=["t2", "adc"], **unet),
        "UNetContrastiveSemiSL": lambda: UNetContrastiveSemiSL(**unet),
        "UNetPL_3class": lambda: UNetPL(**dict(unet, n_classes=3)),
    }


@pytest.mark.parametrize("name", list(_wrappers()))
def test_every_wrapper_builds_its_three_dicts(name):
    net = _wrappers()[name]()
    nc = net.n_classes
    assert list(net.train_metrics) == ["IoU", "Dice"]
    assert list(net.val_metrics) == ["V_IoU", "V_Dice"]
    assert list(net.test_metrics) == ["T_IoU", "T_Pr", "T_F1", "T_Dice"]
    want_c = 1 if nc <= 2 else nc
    for d in (net.train_metrics, net.val_metrics, net.test_metrics):
        assert all(m.num_classes == want_c for m in d.values())
    assert net.compute_train_metrics is False


@pytest.mark.parametrize("name", ["UNetPL", "UNetPL_bn", "UNETRPL", "SWINUNetPL", "UNetPlusPlusPL",
                                  "BrUNetPL", "UNetContrastiveSemiSL"])
def test_metrics_add_no_parameter_buffer_or_state(name):
    net = _wrappers()[name]()
    keys = list(net.state_dict())
    params = [id(p) for p in net.parameters()]
    buffers = [id(b) for b in net.buffers()]
    for k in ("train_metrics", "val_metrics", "test_metrics"):
        delattr(net, k)
    assert keys == list(net.state_dict())
    assert params == [id(p) for p in net.parameters()]
    assert buffers == [id(b) for b in net.buffers()]


def test_state_is_a_plain_attribute_that_moves_and_keeps_its_dtype():
    m = M.MulticlassDice(4)
    assert m.state.dtype == torch.int64 and m.state.shape == (13,)
    assert list(m.buffers()) == [] and list(m.state_dict()) == [] and list(m.parameters()) == []
    m.state[0] = 7
    m.half()
    m.double()
    m.to(torch.float32)
    assert m.state.dtype == torch.int64 and int(m.state[0]) == 7
    m.reset()
    assert int(m.state.abs().sum()) == 0


def test_argument_errors():
    # C > 32: refused at construction and in the ops layer, before anything reaches a kernel
    with pytest.raises(ValueError):
        M.MulticlassJaccardIndex(33)
    with pytest.raises(_lib.AdellHipError, match="32"):
        ops.seg_confusion_update(torch.zeros(1, 33, 4), torch.zeros(1, 4),
                                 [torch.zeros(100, dtype=torch.int64)])
    with pytest.raises(ValueError):
        M.MulticlassPrecision(1)
    with pytest.raises(NotImplementedError, match="num_classes=1"):
        M.Dice(num_classes=3)
    with pytest.raises(NotImplementedError):
        M.Dice(num_classes=1, multiclass=True)
    with pytest.raises(NotImplementedError):
        M.Dice(num_classes=1, zero_division=1)
    with pytest.raises(NotImplementedError, match="macro"):
        M.MulticlassFBetaScore(3, average="micro")
    # mismatched shapes
    with pytest.raises(ValueError):
        M.BinaryJaccardIndex().update(torch.rand(2, 1, 4, 4), torch.zeros(2, 1, 4, 5))
    with pytest.raises(ValueError):
        M.MulticlassJaccardIndex(3).update(torch.rand(2, 4, 4, 4), torch.zeros(2, 4, 4))
    with pytest.raises(_lib.AdellHipError, match="does not match"):
        ops.seg_confusion_update(torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 5),
                                 [torch.zeros(10, dtype=torch.int64)])
    with pytest.raises(_lib.AdellHipError, match="int64"):
        ops.seg_confusion_update(torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4),
                                 [torch.zeros(9, dtype=torch.int64)])
    with pytest.raises(_lib.AdellHipError, match="states"):
        ops.seg_confusion_update(torch.zeros(2, 1, 4, 4), torch.zeros(2, 4, 4),
                                 [torch.zeros(4, dtype=torch.int64)] * 9)
    # no CPU fallback
    with pytest.raises(_lib.AdellHipError, match="CPU"):
        ops.seg_confusion_update(torch.zeros(2, 1, 4, 4), torch.zeros(2, 4, 4),
                                 [torch.zeros(4, dtype=torch.int64)])
    with pytest.raises(_lib.AdellHipError, match="unknown metric"):
        ops.seg_metric_compute(torch.zeros(4, dtype=torch.int64), "recall")


def test_library_refuses_bad_arguments_before_a_launch():
    import ctypes

    h = _lib.lib()
    assert h.adell_seg_confusion_workspace(0, 1) == 0
    assert h.adell_seg_confusion_workspace(1000, 33) == 0
    assert h.adell_seg_confusion_workspace(4 * 256 * 4 * 3, 1) == 3 * 8 * 4
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    states = (ctypes.c_void_p * 1)(p)
    assert h.adell_seg_confusion_update(p, p, 0, 1, 33, 4, 0, p, 1 << 20, states, 1, None) == _lib.E_BADARG
    assert h.adell_seg_confusion_update(p, p, 0, 1, 1, 4, 0, p, 1 << 20, states, 9, None) == _lib.E_BADARG
    assert h.adell_seg_confusion_update(p, p, 3, 1, 1, 4, 0, p, 1 << 20, states, 1, None) == _lib.E_BADARG
    assert h.adell_seg_confusion_update(p, p, 0, 1, 1, 1 << 20, 0, p, 4, states, 1, None) == _lib.E_BADARG
    assert b"workspace" in h.adell_last_error()
    assert h.adell_seg_metric_compute(p, 1, 4, 1.0, p, None) == _lib.E_BADARG
    assert h.adell_seg_metric_compute(p, 1, 2, 0.0, p, None) == _lib.E_BADARG


def test_restatement_on_a_hand_example():
    # binary: 6 voxels, probabilities; 0.5 exactly is negative
    p = np.array([0.9, 0.5, 0.2, 0.7, 0.0, 0.51], np.float32).reshape(1, 1, 6)
    t = np.array([1, 1, 0, 0, 0, 1], np.float32).reshape(1, 6)
    c, bad = ref.counts(p, t)
    assert c.tolist() == [[2, 1, 1]] and not bad           # tp: 0.9, 0.51; fp: 0.7; fn: 0.5
    assert ref.value(c, "iou") == 0.5
    assert ref.value(c, "precision") == 2 / 3
    assert ref.value(c, "dice") == 4 / 6
    assert ref.value(c, "fbeta", 2.0) == 5 * 2 / (5 * 2 + 4 * 1 + 1)
    # logits: 0 is out of range? no -- in [0, 1]; a 2.0 switches the update to the sigmoid mask
    c, _ = ref.counts(np.array([0.0, 2.0, -1.0], np.float32).reshape(1, 1, 3), np.array([[0, 1, 1]]))
    assert c.tolist() == [[1, 0, 1]]
    # nothing anywhere: 0, not 1
    assert ref.value(np.zeros((1, 3), np.int64), "dice") == 0.0
    # targets round half to even; 1.5 -> 2 is outside {0, 1}
    assert not ref.counts(p[..., :3], np.array([[0.5, -0.4, 1.4]], np.float32))[1]
    assert ref.counts(p[..., :3], np.array([[0.5, 1.5, 1.0]], np.float32))[1]
    # multi-class: ties -> first index, absent classes skipped in the macro mean
    p = np.array([[[1, 0, 0, 2], [1, 3, 0, 2], [0, 0, 0, 0]]], np.float32)   # [1, 3, 4]
    t = np.array([[0, 1, 2, 1]])
    c, _ = ref.counts(p, t)                                # argmax: 0, 1, 0, 0
    assert c.tolist() == [[1, 2, 0], [1, 0, 1], [0, 0, 1]]
    assert ref.value(c, "iou") == (1 / 3 + 1 / 2 + 0) / 3
