"""3-D object detection on the GPU: the kernels of csrc/detect.hip against the fp64 restatements
(tests/detection_ref.py, pinned to the reference by tests/test_detection.py), every kernel result computed
twice and compared bit for bit; two training steps and a validation step of the two fixture networks
against the real reference (tests/golden/detection_step_*.npz).

Bounds. Table and decode order: ``torch.equal`` to ``torch.where``. Loss terms and gradients:
``SUM_BOUND`` = 5e-5 of the largest reference magnitude, the project's bound for fixed-order sums. The
golden tool records the reference's OWN fp32-vs-fp64 error on every case; it uses at most a quarter of
that bound everywhere but for the aspect-ratio term of case ``mid_one`` (``ar``, ``m_ar``: 3.9e-5, a
squared difference of two arctangents that cancels), whose bound is therefore four times the recorded
error, 1.55e-4 (``bound`` in detection_loss.npz, ``detection_cases.loss_bound``) -- not a figure taken
from the code under test. Decoded boxes 1e-5 relative, matching IoU 1e-6, anchor map 1e-12 relative (the
device's fp64 ``log``), AMSGrad the tolerances of ``test_fused_adamw_matches_torch``. Steps: loss 1e-4,
gradients 5e-3 by ``cases.grad_rel_err``, parameters (2e-4, 2e-6); the reference's fp32 run uses at most
0.5 % of the parameter tolerance and 4.1e-5 relative on a gradient; the per-positive iou / cpd / ar of
the training steps are held to the gradients' 5e-3 of the largest reference magnitude (``fp32_vs_fp64`` in the step files)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import detection_cases as C
import detection_ref as R
from cases import grad_rel_err

pytestmark = pytest.mark.gpu


def rel(a, r):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).double()
    r = r.detach().double().cpu() if isinstance(r, torch.Tensor) else torch.as_tensor(np.asarray(r)).double()
    assert a.shape == r.shape, (a.shape, r.shape)
    if r.numel() == 0:
        return 0.0
    return float((a - r).abs().max() / (r.abs().max() + 1e-300))


def twice(fn):
    """fn() run two times: the first result, after asserting that the second is bit-identical."""
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert (u is None) == (v is None)
        if u is not None:
            same_nan = u.is_floating_point() and torch.equal(torch.isnan(u), torch.isnan(v))
            assert torch.equal(u, v) or (same_nan and torch.equal(torch.nan_to_num(u), torch.nan_to_num(v))), \
                "two runs differ"
    return a


@pytest.fixture(scope="module")
def loss_gold():
    return C.Gold("loss")


def channels_last(t):
    """The layout the conv kernels produce: [B, C, H, W, D] logical, channels last in memory."""
    return t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


# ---- positive-cell table ----------------------------------------------------------------------------------
TABLE_CASES = [("unit", "none"), ("unit", "all"), ("mid", "none"), ("mid", "all"), ("mid", 64), ("mid", 65),
               ("wide", 64), ("wide", 65), ("wide", 300), ("wide", "all")]


@pytest.mark.parametrize("grid,kind", TABLE_CASES)
@pytest.mark.parametrize("layout", ["dense", "channels_last"])
def test_positive_table_is_torch_where(cuda, grid, kind, layout):
    from adell_mri_amd import ops

    B, A, H, W, D = C.GRIDS[grid]
    target = torch.from_numpy(C.table_target(grid, kind)).to(cuda)
    if layout == "channels_last":
        target = channels_last(target)

    def run():      # rows beyond the count are not written: only the filled part is compared
        table, count = ops.det_positive_table(target, A, C.IOU_THRESHOLD)
        return table[:int(count)], count

    table, count = twice(run)
    stacked = torch.stack(torch.split(target[:, 1:], 7, 1), -1)
    want = torch.stack(torch.where(stacked[:, 0] > C.IOU_THRESHOLD), 1)
    n = int(count)
    assert n == want.shape[0] == ({"none": 0, "all": B * A * H * W * D}.get(kind, kind))
    assert table.dtype == torch.int32 and torch.equal(table[:n].long(), want)


def test_table_over_the_objectness_head_is_torch_where(cuda):
    from adell_mri_amd import ops

    g = torch.Generator().manual_seed(5)
    obj = torch.rand((2, 3, 3, 5, 2), generator=g).to(cuda)
    table, count = ops.det_positive_table(obj, 3, 0.5, 0, 1)
    want = torch.stack(torch.where(torch.stack(torch.split(obj, 1, 1), -1)[:, 0] > 0.5), 1)
    assert torch.equal(table[:int(count)].long(), want)


# ---- fused loss ---------------------------------------------------------------------------------------------
def _fused(case, dev, layout="dense"):
    from adell_mri_amd import functional as HF

    t = {k: torch.from_numpy(case[k]).to(dev) for k in ("centre", "size", "obj", "target", "anchors")}
    if layout == "channels_last":
        for k in ("centre", "size", "obj", "target"):
            t[k] = channels_last(t[k])

    def run():
        heads = [t[k].clone().requires_grad_(True) for k in ("centre", "size", "obj")]   # layout kept
        loss, parts, rows, table, count = HF.detection_loss(*heads, t["target"], t["anchors"], case["corr"],
                                                            C.IOU_THRESHOLD, return_parts=True)
        loss.backward()
        return (loss.detach(), parts, table[:int(count)], rows[:, :int(count)].clone(),
                heads[0].grad, heads[1].grad, heads[2].grad)

    return twice(run)


@pytest.mark.parametrize("layout", ["dense", "channels_last"])
@pytest.mark.parametrize("name", list(C.LOSS_CASES))
def test_fused_loss_forward_and_backward(cuda, loss_gold, name, layout):
    """Against the fp64 restatement; bounds in the module text (``loss_bound``)."""
    case = C.loss_case(name)
    want = R.step_loss(case["centre"], case["size"], case["obj"], case["target"], case["anchors"], case["corr"])
    loss, parts, table, rows, dc, ds, do = _fused(case, cuda, layout)
    n = len(case["positives"])
    assert np.array_equal(table.cpu().numpy(), case["positives"])
    figures = {}
    if n == 0:
        assert torch.isnan(loss) and torch.isnan(parts[0]) and torch.isnan(parts[2:]).all()
        figures["bce"] = rel(parts[1], want["bce"])
    else:
        for i, k in enumerate(("loss", "bce", "m_iou", "m_cpd", "m_ar")):
            figures[k] = rel(parts[i], want[k])
        assert float(loss) == float(parts[0])
        for i, k in enumerate(("iou", "cpd", "ar")):
            figures[k] = rel(rows[i], want[k])
    for k, g in (("dcentre", dc), ("dsize", ds), ("dobj", do)):
        assert g.shape == case[k[1:]].shape
        if np.abs(want[k]).max() == 0:
            assert float(g.abs().max()) == 0.0, k          # no positive: the composite's zeros
        else:
            figures[k] = rel(g, want[k])
    print(name, layout, {k: f"{v:.2e}" for k, v in figures.items()})
    for k, v in figures.items():
        assert v <= C.loss_bound(loss_gold, name, k), (k, v, C.loss_bound(loss_gold, name, k))


def test_fused_loss_equals_the_composite_on_the_device(cuda, loss_gold):
    """The in-repository oracle: YOLONet3dPL's composite path in torch ops on the same device."""
    from adell_mri_amd.modules.object_detection import complete_iou_loss
    from test_detection import _composite

    case = C.loss_case("wide_many")
    loss, _, _, _, dc, ds, do = _fused(case, cuda)
    ref_loss, ref_grads = _composite(case, complete_iou_loss, torch.float32, device=cuda)
    assert rel(loss, ref_loss) <= 1e-5
    for g, r in zip((dc, ds, do), ref_grads):
        assert rel(g, r) <= C.SUM_BOUND


def test_target_gradient_reaches_the_size_head(cuda, loss_gold):
    """The cross-entropy's gradient through its un-detached IoU target: the fused size and centre
    gradients equal the restatement WITH that path and differ from the restatement with the target's
    gradient cut."""
    case = C.loss_case("mid_corners")
    args = (case["centre"], case["size"], case["obj"], case["target"], case["anchors"], case["corr"])
    full = _fused(case, cuda)
    want_full, want_cut = R.step_loss(*args), R.step_loss(*args, cut_target=True)
    assert rel(full[5], want_full["dsize"]) <= C.SUM_BOUND and rel(full[4], want_full["dcentre"]) <= C.SUM_BOUND
    # ... and is nowhere near the restatement without it (the two restatements differ by a third)
    assert rel(want_cut["dsize"], want_full["dsize"]) > 1e-3 and rel(full[5], want_cut["dsize"]) > 1e-3


def test_fused_loss_reads_nothing_on_the_host(cuda):
    """Table, forward and backward under torch's synchronisation check: the positive count stays on the
    device (what lets the two-class training step run without a host read)."""
    from adell_mri_amd import functional as HF

    case = C.loss_case("wide_many")
    t = {k: torch.from_numpy(case[k]).to(cuda) for k in ("centre", "size", "obj", "target", "anchors")}
    corr = [float(v) for v in case["corr"]]

    def run():
        heads = [t[k].clone().requires_grad_(True) for k in ("centre", "size", "obj")]
        loss = HF.detection_loss(*heads, t["target"], t["anchors"], corr, C.IOU_THRESHOLD)
        loss.backward()
        return loss.detach(), heads[0].grad

    first = run()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


def test_loss_refuses_cpu_and_non_dense_inputs(cuda):
    from adell_mri_amd import _lib
    from adell_mri_amd import functional as HF

    case = C.loss_case("mid_one")
    t = {k: torch.from_numpy(case[k]) for k in ("centre", "size", "obj", "target", "anchors")}
    with pytest.raises(_lib.AdellHipError, match="CPU"):
        HF.detection_loss(t["centre"], t["size"], t["obj"], t["target"], t["anchors"], case["corr"])
    d = {k: v.to(cuda) for k, v in t.items()}
    wide = torch.zeros((2, 9, 3, 5, 4), device=cuda)
    with pytest.raises(_lib.AdellHipError, match="non-dense"):
        HF.detection_loss(wide[..., ::2], d["size"], d["obj"], d["target"], d["anchors"], case["corr"])
    with pytest.raises(_lib.AdellHipError, match="non-dense"):
        HF.detection_loss(d["centre"], d["size"], d["obj"], d["target"][:, :, :, :, ::1].transpose(2, 3)
                          .contiguous().transpose(2, 3), d["anchors"], case["corr"])
    with pytest.raises(ValueError, match="expected"):
        HF.detection_loss(d["centre"][:, :6].contiguous(), d["size"], d["obj"], d["target"], d["anchors"],
                          case["corr"])


# ---- decode ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["unit", "mid", "wide"])
@pytest.mark.parametrize("with_classes", [False, True])
def test_decode_equals_the_restatement(cuda, grid, with_classes):
    from adell_mri_amd import functional as HF

    B, A, H, W, D = C.GRIDS[grid]
    rs = np.random.RandomState(B * 7 + H)
    centre = np.tanh(rs.randn(B, 3 * A, H, W, D)).astype(np.float32)
    size = (0.3 * rs.randn(B, 3 * A, H, W, D)).astype(np.float32)
    obj = rs.uniform(0.05, 0.95, (B, A, H, W, D)).astype(np.float32)
    obj = np.where(np.abs(obj - 0.5) < 1e-3, 0.6, obj).astype(np.float32)
    cls = rs.rand(B, 3, H, W, D).astype(np.float32) if with_classes else None
    anchors = rs.uniform(2, 6, (A, 3)).astype(np.float32)
    corr = [8.0, 8.0, 4.0]
    dev = lambda a: None if a is None else channels_last(torch.from_numpy(a).to(cuda))   # noqa: E731

    def run():
        out = HF.detection_decode(dev(centre), dev(size), dev(obj), dev(cls), torch.from_numpy(anchors).to(cuda), corr)
        return [t for item in out for t in item]

    got = twice(run)
    want = R.decode(centre, size, obj, cls, anchors, corr)
    where = torch.where(torch.stack(torch.split(torch.from_numpy(obj), 1, 1), -1)[:, 0] > 0.5)
    assert sum(len(w[1]) for w in want) == len(where[0])
    for b in range(B):
        boxes, scores, classes = got[3 * b:3 * b + 3]
        wb, ws, wc = want[b]
        assert boxes.shape[0] == len(ws)
        if len(ws) == 0:
            continue
        assert np.array_equal(scores.cpu().numpy(), ws.astype(np.float32))       # the order of torch.where
        assert rel(boxes, wb) <= 1e-5
        assert rel(classes, wc) <= 1e-6


# ---- NMS ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.NMS_SIZES)
def test_nms_keeps_what_the_restatement_keeps(cuda, n):
    from adell_mri_amd.modules.object_detection import nms_nd

    boxes, scores = C.nms_case(n)
    tb, ts = torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda)
    kept = twice(lambda: (nms_nd(tb, ts, 0.1, 0.5, suppress=True),))[0]
    want = R.nms(boxes, scores, 0.1, 0.5, suppress=True)
    assert np.array_equal(kept.cpu().numpy(), want)
    as_written = nms_nd(tb, ts, 0.1, 0.5)
    assert np.array_equal(as_written.cpu().numpy(), R.nms(boxes, scores, 0.1, 0.5))
    if n >= 64:
        assert len(want) < len(as_written)


@pytest.mark.parametrize("n", C.NMS_LARGE)
def test_nms_beyond_one_word_per_lane(cuda, n):
    """More than 4096 candidates, and the limit itself: every removed-word slot of the sweep's lanes."""
    from adell_mri_amd import ops
    from adell_mri_amd.modules.object_detection import nms_nd

    assert n <= ops.det_nms_max()
    boxes, scores = C.nms_case_large(n, torch, cuda)
    tb, ts = torch.from_numpy(boxes).to(cuda), torch.from_numpy(scores).to(cuda)
    kept = twice(lambda: (nms_nd(tb, ts, 0.1, 0.5, suppress=True),))[0]
    want = R.nms(boxes, scores, 0.1, 0.5, suppress=True)
    assert len(want) == 2 * (n // 6) + min(n % 6, 1) + (1 if n % 6 > 3 else 0)
    assert np.array_equal(kept.cpu().numpy(), want)


def test_nms_refuses_more_than_its_limit(cuda):
    from adell_mri_amd import functional as HF
    from adell_mri_amd import ops

    n = ops.det_nms_max() + 1
    assert ops.det_nms_max() >= 8192
    boxes = torch.zeros((n, 6), device=cuda)
    with pytest.raises(ValueError, match="at most"):
        HF.detection_nms(boxes, torch.ones(n, device=cuda), 0.5)


# ---- matching ---------------------------------------------------------------------------------------------------
def test_matching_equals_the_restatement(cuda):
    from adell_mri_amd.modules.object_detection import mAP

    preds, targets = C.match_case()
    metric = mAP(iou_threshold=0.5, n_classes=2)
    to = lambda ds: [{k: torch.from_numpy(v).to(cuda) for k, v in d.items()} for d in ds]   # noqa: E731
    metric.update(to(preds), to(targets))
    # the kernel's tables
    from adell_mri_amd import ops
    sorted_preds = [metric._sorted(p) for p in metric.pred_list]
    starts = np.cumsum([0] + [s[0].shape[0] for s in sorted_preds]).astype(np.int32)
    tcount = [t["boxes"].shape[0] for t in targets]
    image = torch.from_numpy(np.repeat(np.arange(len(tcount)), tcount).astype(np.int32)).to(cuda)
    pb = torch.cat([s[0] for s in sorted_preds]).float().contiguous()
    tb = torch.cat([torch.from_numpy(t["boxes"]) for t in targets]).to(cuda).contiguous()
    best, iou = twice(lambda: ops.det_match(tb, image, pb, torch.from_numpy(starts).to(cuda)))
    at = 0
    for p, t in zip(preds, targets):
        wb, wi, any_hit, _ = R.match(p["boxes"], p["scores"], t["boxes"])
        k = len(t["boxes"])
        assert np.array_equal(best[at:at + k].cpu().numpy(), wb)
        np.testing.assert_allclose(iou[at:at + k].cpu().numpy(), wi, rtol=1e-6, atol=1e-7)
        at += k
    value = float(metric.compute())
    cpu_metric = mAP(iou_threshold=0.5, n_classes=2)
    cpu = lambda ds: [{k: torch.from_numpy(v) for k, v in d.items()} for d in ds]   # noqa: E731
    cpu_metric.update(cpu(preds), cpu(targets))
    assert value == pytest.approx(float(cpu_metric.compute()), rel=1e-6) and metric.hits == cpu_metric.hits == 2


# ---- anchor map ---------------------------------------------------------------------------------------------------
def test_anchor_maps_equal_the_fixture(cuda):
    from adell_mri_amd.utils.bounding_boxes import BBToAdjustedAnchors

    gold = C.Gold("anchors")
    for group in (("none", "one", "two"), ("shape",), ("ratio",)):
        anch, ish, osh, thr, _, _, shape = C.ANCHOR_CASES[group[0]]
        N = max(1, max(len(C.ANCHOR_CASES[g][4]) for g in group))
        boxes = np.zeros((len(group), N, 6))
        classes = np.zeros((len(group), N))
        counts = np.zeros(len(group), np.int32)
        for i, g in enumerate(group):
            b, c = C.ANCHOR_CASES[g][4], C.ANCHOR_CASES[g][5]
            boxes[i, :len(b)], classes[i, :len(b)], counts[i] = b, c, len(b)
        t = BBToAdjustedAnchors(anch, ish, osh, thr)
        got = twice(lambda: (t.batch(torch.from_numpy(boxes).to(cuda), torch.from_numpy(classes).to(cuda),
                                     torch.from_numpy(counts).to(cuda), shape=shape),))[0].cpu().numpy()
        assert got.dtype == np.float64
        for i, g in enumerate(group):
            want = gold[f"{g}:map"]
            assert np.array_equal(got[i] != 0, want != 0), g              # the set cells
            assert np.array_equal(got[i, 0], want[0]), g                   # the class plane
            np.testing.assert_allclose(got[i], want, rtol=1e-12, atol=0, err_msg=g)


# ---- AMSGrad ---------------------------------------------------------------------------------------------------
def test_fused_adamw_amsgrad_matches_torch(cuda):
    from adell_mri_amd.optim import FusedAdamW

    rng = np.random.default_rng(4)
    w0 = rng.standard_normal((33, 17)).astype(np.float32)
    a = torch.nn.Parameter(torch.from_numpy(w0.copy()).to(cuda))
    b = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    oa = FusedAdamW([a], lr=5e-3, weight_decay=1e-3, amsgrad=True)
    ob = torch.optim.AdamW([b], lr=5e-3, weight_decay=1e-3, amsgrad=True)
    for step in range(2):
        # a smaller second gradient: the running maximum, not the second moment, sets the step
        g = (rng.standard_normal(w0.shape) * (1.0 if step == 0 else 0.1)).astype(np.float32)
        oa.zero_grad()
        a.grad = torch.from_numpy(g).to(cuda)
        b.grad = torch.from_numpy(g.copy())
        oa.step()
        ob.step()
    np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=2e-5, atol=1e-6)
    sa, sb = oa.state_dict()["state"][0], ob.state_dict()["state"][0]
    np.testing.assert_allclose(sa["max_exp_avg_sq"].cpu().numpy(), sb["max_exp_avg_sq"].numpy(), rtol=2e-5,
                               atol=1e-9)
    assert float((sa["max_exp_avg_sq"] - sa["exp_avg_sq"]).max()) > 0


# ---- the fixture networks ---------------------------------------------------------------------------------------
def _build(name, dev):
    from adell_mri_amd.modules.layers.adn_fn import get_adn_fn
    from adell_mri_amd.modules.object_detection import YOLONet3dPL, complete_iou_loss

    n_classes = C.NET_CONFIGS[name]["n_classes"]
    net = C.build_net(name, YOLONet3dPL, get_adn_fn, dev="cpu", reg_loss_fn=complete_iou_loss,
                      classification_loss_fn=F.binary_cross_entropy if n_classes == 2 else F.cross_entropy,
                      iou_threshold=C.IOU_THRESHOLD, learning_rate=C.STEP_LR, weight_decay=C.STEP_WD,
                      optimizer_eps=C.STEP_EPS)
    return net


@pytest.mark.parametrize("name", C.NETS)
def test_steps_equal_the_reference(cuda, name):
    from adell_mri_amd.trainer import StepRunner, validate_steps

    gold = C.Gold(f"step_{name}")
    net = _build(name, cuda)
    C.fill_net(net, float(gold["gain"]))
    net = net.to(cuda).train()
    assert [tuple(v.shape) for v in net.state_dict().values()] == [
        tuple(int(d) for d in s.split(",")) if s else () for s in gold["state_shapes"]]
    batch = C.net_batch(name, gold["label"], torch, device=cuda)
    assert net.fused_loss(batch["image"])
    runner = StepRunner(net)
    for s in (1, 2):
        loss = runner.train_step(batch)
        torch.cuda.synchronize()
        terms, count = net.last_box_terms
        for i, k in enumerate(("iou", "cpd", "ar")):      # per positive, against the reference's step
            assert rel(terms[i, :int(count)], gold[f"{k}{s}"]) <= 5e-3, (s, k)
        want = float(gold[f"loss{s}"])
        loss = float(loss.detach())
        assert abs(loss - want) <= 1e-4 * abs(want), (s, loss, want)
        if s == 1:
            worst = 0.0
            for k, p in net.named_parameters():
                if "grad:" + k in gold.files:
                    worst = max(worst, grad_rel_err(gold, k, p.grad.detach().cpu().numpy()))
                    assert worst <= 5e-3, (k, worst)
        params = C.Gold(f"step_{name}_params{s}")
        for k, v in net.state_dict().items():
            if v.is_floating_point():
                np.testing.assert_allclose(v.detach().cpu().numpy(), params[f"step{s}:{k}"], rtol=2e-4, atol=2e-6,
                                           err_msg=f"step {s} {k}")
    net.eval()
    with torch.no_grad():
        vloss = net.validation_step(batch, 0)
    want = float(gold["val_loss"])
    assert abs(float(vloss) - want) <= 1e-4 * abs(want)
    for m in net.val_metrics.values():
        m.reset()
    out = validate_steps(net, [batch])
    assert abs(out["val_loss"] - want) <= 1e-4 * abs(want)
    assert set(out) >= {"val_loss", "v:cMSE_center", "v:sMSE_size", "v:objF1_obj", "v:mAP_mAP"}
    assert np.isfinite(out["v:cMSE_center"]) and np.isfinite(out["v:sMSE_size"])
    # the validation heads decoded on the device equal the restatement on the recorded heads
    boxes = net.recover_boxes_batch(*net(batch["image"]), to_dict=True)
    want_boxes = R.decode(gold["val:centre"], gold["val:size"], gold["val:obj"], None,
                          np.asarray(C.NET_CONFIGS[name]["anchor_sizes"]))
    for got, w in zip(boxes, want_boxes):
        margin = np.abs(gold["val:obj"] - 0.5).min()
        if margin > 1e-3:
            assert got["boxes"].shape[0] == len(w[1])


def test_two_class_fused_step_reads_nothing_on_the_host(cuda):
    """``_step_fused`` of the two-class wrapper -- loss, its backward and the training metrics -- from
    heads already computed, under torch's synchronisation check (the network body in front of it is
    the existing kernels' business)."""
    name = "yolo_bin"
    gold = C.Gold(f"step_{name}")
    net = C.fill_net(_build(name, cuda), float(gold["gain"])).to(cuda).train()
    batch = C.net_batch(name, gold["label"], torch, device=cuda)
    x, y = batch["image"], batch["label"].float()
    with torch.no_grad():
        heads = [h.detach() for h in net(x)]

    def run():
        leaves = [h.clone().requires_grad_(True) for h in heads[:3]] + [heads[3]]
        loss = net._step_fused(batch, x, y, leaves, net.train_metrics)
        loss.backward()
        return loss.detach(), leaves[1].grad

    first = run()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    values = {k: float(m.compute()) for k, m in net.train_metrics.items()}
    assert all(np.isfinite(v) for v in values.values()), values


def test_fit_steps_stays_finite(cuda):
    from adell_mri_amd.trainer import fit_steps

    name = "yolo_bin"
    gold = C.Gold(f"step_{name}")
    net = C.fill_net(_build(name, cuda), float(gold["gain"])).to(cuda)
    batch = C.net_batch(name, gold["label"], torch, device=cuda)
    losses = fit_steps(net, [batch] * 3)
    assert len(losses) == 3 and all(np.isfinite(float(v)) for v in losses)
