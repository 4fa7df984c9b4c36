"""Segmentation metrics on the device (csrc/seg_metrics.hip, adell_mri_amd.metrics, the wrappers'
metric dicts, trainer.validate_steps / test_steps) against the fp64 restatement of
tests/seg_metrics_ref.py on the same tensors: counts equal as integers, values within 1 ulp of
fp32."""
import os
import sys

import numpy as np
import pytest
import torch

from adell_mri_amd import metrics as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seg_metrics_ref as ref  # noqa: E402

BINARY = [("iou", M.BinaryJaccardIndex, {}), ("precision", M.BinaryPrecision, {}),
          ("fbeta", M.BinaryFBetaScore, {"beta": 2.0}), ("dice", M.Dice, {})]
MULTI = [("iou", M.MulticlassJaccardIndex), ("precision", M.MulticlassPrecision),
         ("fbeta", M.MulticlassFBetaScore), ("dice", M.MulticlassDice)]


def _binary_metrics(cuda):
    return [(k, cls(**kw).to(cuda), kw.get("beta", 1.0)) for k, cls, kw in BINARY]


def _multi_metrics(cuda, C):
    return [(k, cls(C).to(cuda), 1.0) for k, cls in MULTI]


def _check(ms, updates):
    """``ms``: [(kind, metric, beta)] all fed with ``updates`` [(pred, target)] through ONE fused
    update per step; compares state counts and values with the restatement."""
    want = None
    for pred, target in updates:
        M.update_many([m for _, m, _ in ms], pred, target)
        c, bad = ref.counts(pred.cpu().numpy(), target.cpu().numpy())
        assert not bad
        want = c if want is None else want + c
    for kind, m, beta in ms:
        st = m.state.cpu().numpy()
        assert st[:-1].reshape(-1, 3).tolist() == want.tolist(), kind
        assert st[-1] == 0
        got = float(m.compute())
        w = ref.value(want, kind, beta)
        assert ref.within_one_ulp(got, w), (kind, got, w)
    return want


def _probs(shape, seed, dev):
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(shape, generator=g)
    flat = p.view(-1)
    n = flat.numel()
    idx = torch.randperm(n, generator=g)
    k = max(1, n // 16)
    flat[idx[:k]] = 0.5                                          # exact halves: negative
    flat[idx[k:2 * k]] = float(np.nextafter(np.float32(0.5), np.float32(1)))
    flat[idx[2 * k:3 * k]] = float(np.nextafter(np.float32(0.5), np.float32(0)))
    flat[idx[3 * k:4 * k]] = 0.0
    flat[idx[4 * k:5 * k]] = 1.0
    return p.to(dev)


def _mask(shape, seed, dev, p=0.3):
    g = torch.Generator().manual_seed(seed + 1000)
    return (torch.rand(shape, generator=g) < p).float().to(dev)


@pytest.mark.parametrize("shape", [(1, 1, 8, 8, 8), (2, 1, 5, 7, 9), (3, 1, 33, 17), (1, 1, 3),
                                   (2, 1, 64, 64, 65), (3, 1, 1021)])
def test_binary_probabilities_with_exact_halves(cuda, shape):
    ms = _binary_metrics(cuda)
    _check(ms, [(_probs(shape, 1, cuda), _mask(shape, 1, cuda)),
                (_probs(shape, 2, cuda), _mask((shape[0],) + shape[2:], 2, cuda))])


def test_binary_full_size_update(cuda):
    shape = (2, 1, 128, 128, 128)
    _check(_binary_metrics(cuda), [(_probs(shape, 3, cuda), _mask(shape, 3, cuda, 0.05))])


def test_out_of_range_switches_to_sigmoid_for_that_update_only(cuda):
    shape = (2, 1, 16, 16, 12)
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(shape, generator=g) * 3
    small = logits.abs() < 1e-6
    logits[small] = 1e-3                      # CPU and GPU sigmoid may round apart below 1e-6
    logits.view(-1)[::7] = 0.0                # sigmoid(0) = 0.5: negative
    logits.view(-1)[3::11] = 0.25             # in range, but the update is out of range
    y = _mask(shape, 5, cuda, 0.5)
    ms = _binary_metrics(cuda)
    c = _check(ms, [(_probs(shape, 6, cuda), y), (logits.to(cuda), y), (_probs(shape, 7, cuda), y)])
    # the mask of the in-range updates is p > 0.5, the logits' one sigmoid(x) > 0.5 = x > 0
    p1, p3 = _probs(shape, 6, cuda), _probs(shape, 7, cuda)
    t = y.bool()
    tp = int(((p1 > 0.5) & t).sum() + ((logits.to(cuda) > 0) & t).sum() + ((p3 > 0.5) & t).sum())
    assert c[0, 0] == tp


def test_nan_and_inf_predictions(cuda):
    shape = (2, 1, 9, 9, 9)
    p = _probs(shape, 8, cuda).cpu()
    p.view(-1)[::13] = float("nan")
    p.view(-1)[1::17] = float("inf")
    p.view(-1)[2::19] = -float("inf")
    _check(_binary_metrics(cuda), [(p.to(cuda), _mask(shape, 8, cuda, 0.5))])
    # only NaN / inf and values inside [0, 1]: still the sigmoid mask (NaN counts as outside)
    q = _probs(shape, 9, cuda).cpu()
    q.view(-1)[::29] = float("nan")
    _check(_binary_metrics(cuda), [(q.to(cuda), _mask(shape, 9, cuda, 0.5))])


@pytest.mark.parametrize("dtype", ["f32_fractions", "uint8", "bool", "int64"])
@pytest.mark.parametrize("shape", [(2, 1, 12, 12, 12), (3, 1, 7, 11)])
def test_target_dtypes(cuda, dtype, shape):
    y = _mask(shape, 10, cuda).cpu()
    if dtype == "f32_fractions":
        y = y.clone()
        y.view(-1)[::5] = 0.5          # rounds to 0
        y.view(-1)[1::7] = -0.4        # rounds to -0 = 0
        y.view(-1)[2::9] = 1.4         # rounds to 1
    elif dtype == "uint8":
        y = y.to(torch.uint8)
    elif dtype == "bool":
        y = y.bool()
    else:
        y = y.long()
    _check(_binary_metrics(cuda), [(_probs(shape, 10, cuda), y.to(cuda))])


def test_unaligned_views_take_the_scalar_path(cuda):
    shape = (3, 1, 5, 6, 7)
    p = _probs(shape, 11, cuda).reshape(-1)
    y = _mask(shape, 11, cuda).reshape(-1)
    n = p.numel() - 1
    pv, yv = p[1:].view(1, 1, n), y[1:].view(1, n)      # 4-byte offsets
    _check(_binary_metrics(cuda), [(pv, yv)])
    yb = y.to(torch.uint8)
    _check(_binary_metrics(cuda), [(pv, yb[1:].view(1, n))])


def _mc_case(shape, C, seed, dev, layout="ncdhw"):
    g = torch.Generator().manual_seed(seed)
    B, sp = shape[0], shape[1:]
    logits = torch.randint(0, 4, (B, C) + sp, generator=g).float()    # many ties
    y = torch.randint(0, C - 1, (B,) + sp, generator=g)                 # class C-1 absent in y
    logits[:, 0] = torch.where(logits[:, 0] > 2, torch.full_like(logits[:, 0], float("nan")),
                               logits[:, 0]) if seed % 2 else logits[:, 0]
    pred = logits.to(dev)
    if layout == "cl":
        pred = pred.contiguous(memory_format=torch.channels_last_3d if len(sp) == 3
                               else torch.channels_last)
    return pred, y.to(dev)


@pytest.mark.parametrize("C", [3, 5])
@pytest.mark.parametrize("shape,layout", [((2, 8, 8, 8), "ncdhw"), ((1, 5, 7, 9), "ncdhw"),
                                          ((3, 12, 13), "ncdhw"), ((2, 8, 8, 8), "cl"),
                                          ((2, 9, 10), "cl")])
def test_multiclass(cuda, C, shape, layout):
    ms = _multi_metrics(cuda, C)
    p1, y1 = _mc_case(shape, C, 1, cuda, layout)
    p2, y2 = _mc_case(shape, C, 2, cuda, layout)
    y2 = y2.float().unsqueeze(1)                       # [B, 1, ...] fp32 targets
    c = _check(ms, [(p1, y1), (p2, y2)])
    assert c[C - 1, 2] == 0                            # absent from the targets: no fn


def test_multiclass_fp32_targets_round(cuda):
    C = 3
    p, y = _mc_case((2, 6, 6, 6), C, 3, cuda)
    yf = y.float().cpu()
    yf.view(-1)[::5] = 0.5
    yf.view(-1)[1::7] = 1.5
    yf.view(-1)[2::9] = -0.4
    _check(_multi_metrics(cuda, C), [(p, yf.to(cuda))])


def test_several_updates_equal_one_on_the_concatenation(cuda):
    shapes = [(1, 1, 10, 12, 14), (2, 1, 10, 12, 14), (1, 1, 10, 12, 14)]
    ps = [_probs(s, 20 + i, cuda) for i, s in enumerate(shapes)]
    ys = [_mask(s, 20 + i, cuda) for i, s in enumerate(shapes)]
    a, b = M.BinaryJaccardIndex().to(cuda), M.BinaryJaccardIndex().to(cuda)
    for p, y in zip(ps, ys):
        a.update(p, y)
    b.update(torch.cat(ps), torch.cat(ys))
    assert torch.equal(a.state, b.state)
    assert float(a.compute()) == float(b.compute())
    C = 4
    pm = [_mc_case((1, 6, 7, 8), C, 30 + i, cuda)[0] for i in range(3)]
    ym = [_mc_case((1, 6, 7, 8), C, 30 + i, cuda)[1] for i in range(3)]
    a, b = M.MulticlassDice(C).to(cuda), M.MulticlassDice(C).to(cuda)
    for p, y in zip(pm, ym):
        a.update(p, y)
    b.update(torch.cat(pm), torch.cat(ym))
    assert torch.equal(a.state, b.state)


def test_reset(cuda):
    m = M.BinaryPrecision().to(cuda)
    m.update(_probs((1, 1, 8, 8), 40, cuda), _mask((1, 1, 8, 8), 40, cuda))
    assert int(m.state[:3].sum()) > 0
    m.reset()
    assert int(m.state.abs().sum()) == 0
    assert float(m.compute()) == 0.0                  # nothing seen: 0
    _check([("precision", m, 1.0)], [(_probs((1, 1, 8, 8), 41, cuda), _mask((1, 1, 8, 8), 41, cuda))])


def test_bad_target_raises_at_compute(cuda):
    m = M.BinaryJaccardIndex().to(cuda)
    y = _mask((1, 1, 8, 8), 50, cuda)
    y[0, 0, 3, 3] = 1.5                                # rounds to 2
    m.update(_probs((1, 1, 8, 8), 50, cuda), y)        # no error here: update does not synchronise
    with pytest.raises(RuntimeError, match="outside"):
        m.compute()
    m.reset()
    m.update(_probs((1, 1, 8, 8), 50, cuda), _mask((1, 1, 8, 8), 50, cuda))
    m.compute()
    mc = M.MulticlassJaccardIndex(3).to(cuda)
    p, y = _mc_case((1, 4, 4, 4), 3, 4, cuda)
    y[0, 1, 1, 1] = 3
    mc.update(p, y)
    with pytest.raises(RuntimeError, match=r"\[0, 3\)"):
        mc.compute()


def _device_kernels(prof):
    """Device kernel names (a template kernel's demangled name starts with its return type)."""
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA
             and not e.name.lower().startswith(("memcpy", "memset"))]
    return [n[5:] if n.startswith("void ") else n for n in names]


def test_update_metrics_is_one_fused_update(cuda):
    from torch.profiler import ProfilerActivity, profile

    from adell_mri_amd.modules.segmentation.pl import get_metric_dict, update_metrics

    md = get_metric_dict(2, False, None, "T_", dev=cuda)
    assert len(md) == 4
    p, y = _probs((2, 1, 16, 16, 16), 60, cuda), _mask((2, 1, 16, 16, 16), 60, cuda)
    update_metrics(None, md, p, y, None, None)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        update_metrics(None, md, p, y, None, None)
        torch.cuda.synchronize()
    names = _device_kernels(prof)
    assert len(names) == 2 and all(n.startswith("adell_") for n in names), names
    assert "seg_confusion_partials" in names[0] and "seg_confusion_finalize" in names[1]
    c, _ = ref.counts(p.cpu().numpy(), y.cpu().numpy())
    for m in md.values():
        assert (m.state[:3].cpu().numpy() == 2 * c[0]).all()


def test_update_metrics_does_not_synchronise(cuda):
    from adell_mri_amd.modules.segmentation.pl import get_metric_dict, update_metrics

    md = get_metric_dict(3, False, None, "V_", dev=cuda)
    p, y = _mc_case((2, 8, 8, 8), 3, 61, cuda)
    mb = get_metric_dict(2, False, None, "V_", dev=cuda)
    pb, yb = _probs((2, 1, 8, 8, 8), 61, cuda), _mask((2, 1, 8, 8, 8), 61, cuda)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        update_metrics(None, md, p, y.unsqueeze(1).float(), None, None)
        update_metrics(None, mb, pb, yb, None, None)
        for m in list(md.values()) + list(mb.values()):
            m.compute_async()
    finally:
        torch.cuda.set_sync_debug_mode(0)
    torch.cuda.synchronize()


# ---- wrappers and loops -------------------------------------------------------------------------
def _net(cuda):
    import ddp_worker

    return ddp_worker.build(cuda)


def _val_batches(cuda):
    g = np.load(os.path.join(ROOT, "tests", "golden", "unet3d_cfg2_small.npz"))
    x, y = torch.from_numpy(g["x"]).to(cuda), torch.from_numpy(g["y"]).to(cuda)
    return [{"image": x[i:i + 1], "mask": y[i:i + 1]} for i in range(x.shape[0])]


def test_validate_and_test_steps_on_unet(cuda):
    from adell_mri_amd import trainer

    net = _net(cuda)
    batches = _val_batches(cuda)
    net.eval()
    with torch.no_grad():
        today = [float(net._evaluation_loss(b)) for b in batches]   # the loss without metrics
        preds = [net.predict_step(b)[0].cpu().numpy() for b in batches]
    net.train()
    out = trainer.validate_steps(net, batches)
    assert net.training
    assert set(out) == {"val_loss", "V_IoU", "V_Dice"}
    assert out["val_loss"] == pytest.approx(float(np.mean(today)), rel=1e-12, abs=0)
    c = sum(ref.counts(p, b["mask"].cpu().numpy())[0] for p, b in zip(preds, batches))
    assert ref.within_one_ulp(out["V_IoU"], ref.value(c, "iou"))
    assert ref.within_one_ulp(out["V_Dice"], ref.value(c, "dice"))
    assert all(int(m.state.abs().sum()) == 0 for m in net.val_metrics.values())   # reset
    out = trainer.test_steps(net, batches)
    assert set(out) == {"test_loss", "T_IoU", "T_Pr", "T_F1", "T_Dice"}
    assert out["test_loss"] == pytest.approx(float(np.mean(today)), rel=1e-12, abs=0)
    for k, kind in (("T_IoU", "iou"), ("T_Pr", "precision"), ("T_F1", "fbeta"), ("T_Dice", "dice")):
        assert ref.within_one_ulp(out[k], ref.value(c, kind)), k
    # validation_step's loss is bit-for-bit what it was without the metric update
    net.eval()
    with torch.no_grad():
        for b, t in zip(batches, today):
            assert float(net.validation_step(b, 0)) == t
    net.train()


def test_default_training_step_launches_what_it_did(cuda):
    from torch.profiler import ProfilerActivity, profile

    net = _net(cuda)
    batch = _val_batches(cuda)[0]

    def kernels(module):
        module.training_step(batch, 0)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            module.training_step(batch, 0)
            torch.cuda.synchronize()
        # without the bulk zero fill of the amax arena (functional._amax_pair): it runs once per
        # 256 conv calls, so where it falls depends on how many steps ran before
        return [n for n in _device_kernels(prof) if "FillFunctor<int>" not in n]

    with_dicts = kernels(net)
    stripped = _net(cuda)
    for k in ("train_metrics", "val_metrics", "test_metrics"):
        delattr(stripped, k)
    assert with_dicts == kernels(stripped)
    assert not any("seg_confusion" in n for n in with_dicts)
    assert all(int(m.state.abs().sum()) == 0 for m in net.train_metrics.values())

    net.compute_train_metrics = True
    on = kernels(net)
    extra = [n for n in on if "seg_confusion" in n]
    assert len(extra) == 2, extra
    import difflib
    rest = [n for n in on if "seg_confusion" not in n]
    assert rest == with_dicts, "\n".join(difflib.unified_diff(with_dicts, rest, lineterm=""))
    st = net.train_metrics["IoU"].state.cpu()
    assert int(st[:3].sum()) > 0 and int(st[3]) == 0
    assert torch.equal(st, net.train_metrics["Dice"].state.cpu())
    v = float(net.train_metrics["Dice"].compute())
    assert 0.0 <= v <= 1.0


def test_enable_graph_refuses_train_metrics(cuda):
    from adell_mri_amd.trainer import StepRunner

    net = _net(cuda)
    net.compute_train_metrics = True
    runner = StepRunner(net)
    with pytest.raises(RuntimeError, match="compute_train_metrics"):
        runner.enable_graph(_val_batches(cuda)[0])
