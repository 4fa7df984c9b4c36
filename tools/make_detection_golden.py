#!/usr/bin/env python3
"""Fixtures of the detection path from the REAL reference (needs a checkout of the reference,
ADELL_REFERENCE; no test reads it, the tests read the fixtures):

    python tools/make_detection_golden.py    -> tests/golden/detection_*.npz, detection_meta.json

The reference is imported through the stub recipe of tools/make_mil_golden.py (empty package stubs with
the right __path__, then the leaf modules). ``object_detection/pl.py`` needs ``lightning`` and
``torchmetrics`` and ``bounding_boxes.py`` needs ``monai.transforms`` and ``skimage.measure``: all four are
stubbed (``LightningModule`` = ``torch.nn.Module``, metric classes that accept anything and do nothing,
empty transform base classes), as is ``classification/pl.py`` for its ``meta_tensors_to_tensors``. What
runs is the reference's own ``YOLONet3dPL.step`` / ``calculate_loss`` (with an empty metric dict),
``complete_iou_loss``, ``nms_nd``, ``calculate_iou``, ``check_overlap``, ``mAP.compute_image`` (its average
precision replaced by a recorder) and ``BBToAdjustedAnchors``.

Recorded:
  detection_loss.npz     head-level loss cases (tests/detection_cases.py LOSS_CASES): inputs, fp64 loss
                         and terms, iou / cpd / ar per positive, gradients of the three heads, and the
                         reference's own fp32-vs-fp64 error per quantity (``fp32_vs_fp64``) with the
                         bound that follows from it (``bound``): SUM_BOUND where the error uses at most
                         a quarter of it, four times the error where it does not (printed).
  detection_boxes.npz    nms_nd as written and with the one-token correction (``is False`` -> ``not``)
                         applied to a copy of the function's text (not committed); calculate_iou and
                         check_overlap on pairs; what mAP.compute_image feeds its average precision.
  detection_anchors.npz  BBToAdjustedAnchors maps of ANCHOR_CASES.
  detection_step_<net>.npz  two training steps and a validation step of the two networks, in fp64
                         (fp32 copies of the tensors) with the fp32-vs-fp64 ratios of the reference;
                         the parameters after step s in detection_step_<net>_params<s>.npz.
  detection_meta.json    inspect.signature and state_dict keys / shapes of the two classes.

Asserted on the inputs: every comparison the code makes (map objectness against the threshold, corner
maxima / minima, IoU against the NMS threshold, score order, IoU argmax, the anchor map's tests) has a
margin of 1e-4, and no positive has iou = 1 with v = 0."""
import inspect
import json
import os
import sys
import types

import numpy as np

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("ADELL_REFERENCE") or os.path.join(os.path.dirname(ROOT), "reference")
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def _stub(name, **attrs):
    m = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


for name, path in [
    ("adell_mri", "adell_mri"), ("adell_mri.modules", "adell_mri/modules"),
    ("adell_mri.modules.layers", "adell_mri/modules/layers"), ("adell_mri.utils", "adell_mri/utils"),
    ("adell_mri.utils.monai_transforms", "adell_mri/utils/monai_transforms"),
    ("adell_mri.modules.object_detection", "adell_mri/modules/object_detection"),
    ("adell_mri.modules.classification", "adell_mri/modules/classification"),
]:
    _stub(name).__path__ = [os.path.join(REF, path)]


class _Nothing(torch.nn.Module):
    def __init__(self, *a, **k):
        super().__init__()

    def forward(self, *a, **k):
        return None


class _Recorder(_Nothing):
    fed = []

    def update(self, proba, classes):
        _Recorder.fed.append((proba.detach().clone(), classes.detach().clone()))

    def reset(self):
        pass


_pl = _stub("lightning.pytorch", LightningModule=torch.nn.Module)
_stub("lightning", pytorch=_pl)
_metric = _stub("torchmetrics.metric", Metric=torch.nn.Module)
_stub("torchmetrics", metric=_metric, MeanSquaredError=_Nothing, FBetaScore=_Nothing, Recall=_Nothing,
      Precision=_Nothing, AveragePrecision=_Recorder)
_tr = _stub("monai.transforms", Transform=object, MapTransform=object, RandomizableTransform=object)
_stub("monai", transforms=_tr)
_sk = _stub("skimage.measure")
_stub("skimage", measure=_sk)
_stub("adell_mri.modules.classification.pl", meta_tensors_to_tensors=lambda b: b)
import einops.layers.torch  # noqa: E402,F401

from adell_mri.modules.layers.adn_fn import get_adn_fn  # noqa: E402
from adell_mri.modules.object_detection import losses as RL  # noqa: E402
from adell_mri.modules.object_detection import map as RMAP  # noqa: E402
from adell_mri.modules.object_detection import pl as RPL  # noqa: E402
from adell_mri.modules.object_detection import utils as RU  # noqa: E402
from adell_mri.utils.monai_transforms.bounding_boxes import BBToAdjustedAnchors  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import detection_cases as C  # noqa: E402
from cases import grad_rel_err  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F = torch.nn.functional
TOL = dict(loss=1e-4, grad=5e-3, param=(2e-4, 2e-6))


def _ciou_fp64():
    """complete_iou_loss ends in ``iou.float()``, which the step's ``y_object[...] = iou`` refuses for an
    fp64 network (index_put of mixed dtypes). The fp64 runs use a copy of the function's text without
    that one cast (made here, not committed), so the fp64 records carry no fp32 rounding."""
    src = inspect.getsource(RL.complete_iou_loss)
    assert src.count("return iou.float(), cpd_component, ar_component") == 1
    ns = dict(vars(RL))
    exec(src.replace("return iou.float(), cpd_component, ar_component",
                     "return iou, cpd_component, ar_component"), ns)
    return ns["complete_iou_loss"]


_CIOU64 = _ciou_fp64()


def ciou_in_dtype(*args):
    """The reference's complete_iou_loss; for fp64 arguments its copy without the closing cast."""
    return (_CIOU64 if args[0].dtype == torch.float64 else RL.complete_iou_loss)(*args)


def anchor_margin(anch, ish, osh, thr, boxes, shape=None):
    """The smallest distance from equality over every comparison BBToAdjustedAnchors makes for these
    boxes: the anchor-against-box intersect tests and |centre adjustment| against 1 in every cell and
    axis, iou against the threshold, and iou against the value already stored in a cell it may take."""
    osh = np.asarray(osh)
    rel_a = np.asarray(ish) / osh
    rel = rel_a if shape is None else np.asarray(shape) / osh
    cells = np.array(list(np.ndindex(*osh)), np.float64)
    stored = np.zeros((len(anch), len(cells)))
    worst = np.inf
    for bx in np.asarray(boxes, np.float64).reshape(-1, 6):
        lo, hi = bx[:3] / rel, bx[3:] / rel
        sz, ctr = hi - lo, (lo + hi) / 2
        for ai, a in enumerate(anch):
            hf = np.asarray(a) / rel_a / 2
            adim = 2 * hf
            inter = np.prod(np.minimum(sz, adim) + 1 / rel)
            iou = inter / (np.prod(adim) + np.prod(sz + 1 / rel) - inter)
            adj = ctr - (cells + 0.5)
            worst = min(worst, abs(iou - thr), np.abs(cells + hf + 0.5 - lo).min(),
                        np.abs(cells - hf + 0.5 - hi).min(), np.abs(np.abs(adj) - 1).min())
            ok = (np.all(cells + hf + 0.5 > lo, 1) & np.all(cells - hf + 0.5 < hi, 1)
                  & np.all(np.abs(adj) < 1, 1) & (iou > thr))
            if ok.any():
                worst = min(worst, np.abs(iou - stored[ai][ok]).min())
                stored[ai][ok & (iou > stored[ai])] = iou
    return worst


def match_margin(pred, target, score_threshold=0.5, iou_threshold=0.5):
    """The smallest distance from equality over the comparisons of mAP.compute_image for one image:
    score against the threshold, the order of the kept scores, the gap between the best and the
    second-best IoU of a target box, and the best IoU against the hit threshold."""
    sc = pred["scores"].astype(np.float64)
    worst = np.abs(sc - score_threshold).min()
    keep = np.sort(sc[sc > score_threshold])
    if keep.size > 1:
        worst = min(worst, np.diff(keep).min())
    pb = pred["boxes"].astype(np.float64)[sc > score_threshold]
    for t in target["boxes"].astype(np.float64):
        if len(pb) == 0:
            continue
        ov = RU.check_overlap(torch.from_numpy(t[None]), torch.from_numpy(pb)).numpy()
        v = np.zeros(len(pb))
        if ov.any():
            v[ov] = RU.calculate_iou(torch.from_numpy(t[None]), torch.from_numpy(pb[ov])).numpy()
        top = np.sort(v)[::-1]
        if top[0] > 0:
            worst = min(worst, abs(top[0] - iou_threshold))
            if len(top) > 1:
                worst = min(worst, top[0] - top[1])
    return worst


# ---- head-level loss cases --------------------------------------------------------------------------
def reference_loss(case, dt):
    """YOLONet3dPL.step's arithmetic from the heads on (pl.py:255-264) and calculate_loss itself."""
    A = case["obj"].shape[1]
    heads = [torch.tensor(case[k], dtype=dt, requires_grad=True) for k in ("centre", "size", "obj")]
    y = torch.tensor(case["target"], dtype=dt)
    self = types.SimpleNamespace(
        anchor_tensor=torch.tensor(case["anchors"], dtype=dt).reshape(3 * A, 1, 1, 1),
        center_idxs=np.array([1, 2, 3]), size_idxs=np.array([4, 5, 6]), n_classes=2,
        reg_loss_fn=RL.complete_iou_loss, object_loss_fn=F.binary_cross_entropy, object_loss_params={})
    split = lambda x, n, dim: torch.split(x, int(x.shape[dim] // n), dim)   # noqa: E731
    y_class, y = y[:, 0], y[:, 1:]
    y = torch.stack(split(y, A, 1), -1)
    b, h, w, d, a = torch.where(y[:, 0] > C.IOU_THRESHOLD)
    prediction = [torch.stack(split(x, A, 1), -1) for x in heads] + [None]
    seen = {}

    def reg(*args):
        seen["iou"], seen["cpd"], seen["ar"] = out = ciou_in_dtype(*args)
        seen["corners"] = (args[0].detach(), args[1].detach())
        return out

    self.reg_loss_fn = reg
    corr = torch.tensor(case["corr"], dtype=dt)
    loss = RPL.YOLONet3dPL.calculate_loss(self, prediction, y, y_class, b, h, w, d, a, corr)
    grads = torch.autograd.grad(loss, heads, allow_unused=True)
    out = {"loss": loss.detach(), "rows": torch.stack([b, h, w, d, a], 1)}
    for k in ("iou", "cpd", "ar"):
        out[k] = seen[k].detach()
    for k, g, x in zip(("dcentre", "dsize", "dobj"), grads, heads):
        out[k] = torch.zeros_like(x) if g is None else g
    out["bce"] = out["loss"] - 0.1 * ((1 - out["iou"]).mean() + out["cpd"].mean() + out["ar"].mean())
    if b.numel() == 0:      # the box terms are NaN: the cross-entropy against the all-zero target itself
        out["bce"] = F.binary_cross_entropy(heads[2].detach(), torch.zeros_like(heads[2]))
    out["m_iou"], out["m_cpd"], out["m_ar"] = (1 - out["iou"]).mean(), out["cpd"].mean(), out["ar"].mean()
    out["target_grad"] = torch.tensor(float(y.requires_grad))
    pa, pb = seen["corners"]
    if pa.shape[0]:
        # corner comparisons of complete_iou_loss, and the positives' distance from the threshold
        m = min(float((pa - pb).abs().min()), float((y[:, 0][b, h, w, d, a] - C.IOU_THRESHOLD).abs().min()))
        assert m >= C.MARGIN, m
        assert float((1 - out["iou"].double()).abs().min()) > 1e-3      # iou = 1 with v = 0: alpha 0 / 0
    neg = y[:, 0][y[:, 0] <= C.IOU_THRESHOLD]
    assert neg.numel() == 0 or float((C.IOU_THRESHOLD - neg).min()) >= C.MARGIN
    return out


def gen_loss():
    out, report = {}, {}
    for name in C.LOSS_CASES:
        case = C.loss_case(name)
        o64, o32 = reference_loss(case, torch.float64), reference_loss(case, torch.float32)
        assert np.array_equal(o64["rows"].numpy(), case["positives"]), name
        for k, v in case.items():
            out[f"{name}:{k}"] = v
        worst = {}
        for k in ("loss", "bce", "m_iou", "m_cpd", "m_ar", "iou", "cpd", "ar", "dcentre", "dsize", "dobj"):
            out[f"{name}:ref:{k}"] = o64[k].double().numpy()
            scale = float(o64[k].double().abs().max()) if o64[k].numel() else 0.0
            if scale > 0 and np.isfinite(scale):
                worst[k] = float((o32[k].double() - o64[k].double()).abs().max()) / scale
        out[f"{name}:fp32_vs_fp64"] = np.array([worst.get(k, 0.0) for k in sorted(worst)])
        out[f"{name}:fp32_vs_fp64_names"] = np.array(sorted(worst))
        report[name] = worst
        # the bound the GPU test holds each quantity to: SUM_BOUND where the reference's own fp32
        # error uses at most a quarter of it, else four times that error
        bounds = {k: (C.SUM_BOUND if e <= 0.25 * C.SUM_BOUND else 4 * e) for k, e in worst.items()}
        out[f"{name}:bound"] = np.array([bounds[k] for k in sorted(bounds)])
        wide = {k: (worst[k], b) for k, b in bounds.items() if b > C.SUM_BOUND}
        if wide:
            print(f"loss {name}: the reference's fp32 error exceeds a quarter of SUM_BOUND for "
                  f"{wide} (error, bound = 4 x error)")
        print(f"loss {name}: loss {float(o64['loss']):.6f}, positives {len(case['positives'])}, "
              f"fp32 vs fp64 (relative to the largest magnitude) max {max(worst.values()) if worst else 0:.2e}")
    np.savez_compressed(os.path.join(OUT, "detection_loss.npz"), **out)
    return report


# ---- boxes: nms, iou, overlap, matching ---------------------------------------------------------------
def corrected_nms():
    src = inspect.getsource(RU.nms_nd)
    assert src.count("excluded[i] is False") == 1
    ns = dict(torch=torch, check_overlap=RU.check_overlap, calculate_iou=RU.calculate_iou)
    exec(src.replace("excluded[i] is False", "not excluded[i]"), ns)
    return ns["nms_nd"]


def gen_boxes():
    out = {}
    fixed = corrected_nms()
    for n in (2, 65, 130):
        boxes, scores = C.nms_case(n)
        tb, ts = torch.from_numpy(boxes), torch.from_numpy(scores)
        out[f"nms{n}:boxes"], out[f"nms{n}:scores"] = boxes, scores
        out[f"nms{n}:as_written"] = RU.nms_nd(tb, ts, 0.1, 0.5).numpy()
        out[f"nms{n}:corrected"] = fixed(tb, ts, 0.1, 0.5).numpy()
        assert np.diff(np.sort(scores.astype(np.float64))).min() >= C.MARGIN      # score order
        assert np.abs(scores.astype(np.float64) - 0.1).min() >= C.MARGIN         # score threshold
        print(f"nms {n}: as written keeps {len(out[f'nms{n}:as_written'])}, corrected "
              f"{len(out[f'nms{n}:corrected'])}")
    # the IoU-0.75 pair
    pair = torch.tensor([[0., 0., 0., 9., 9., 9.], [0., 0., 0., 9., 9., 6.5]])
    out["pair:boxes"], out["pair:iou"] = pair.numpy(), RU.calculate_iou(pair[:1], pair[1:]).numpy()
    out["pair:as_written"] = RU.nms_nd(pair, torch.tensor([0.9, 0.8]), 0.1, 0.5).numpy()
    out["pair:corrected"] = fixed(pair, torch.tensor([0.9, 0.8]), 0.1, 0.5).numpy()
    boxes, _ = C.nms_case(65)
    a, b = torch.from_numpy(boxes[:32]).double(), torch.from_numpy(boxes[32:64]).double()
    out["iou:a"], out["iou:b"] = a.numpy(), b.numpy()
    out["iou:value"] = RU.calculate_iou(a, b).numpy()
    out["iou:overlap"] = RU.check_overlap(a, b).numpy()
    out["iou:volume"] = RU.bb_volume(a).numpy()
    # matching: what compute_image feeds the average precision, image by image
    preds, targets = C.match_case()
    metric = RMAP.mAP(iou_threshold=0.5, n_classes=2)
    for i, (p, t) in enumerate(zip(preds, targets)):
        m = match_margin(p, t)
        assert m >= C.MARGIN, (i, m)
        _Recorder.fed.clear()
        metric.compute_image({k: torch.from_numpy(v) for k, v in p.items()},
                             {k: torch.from_numpy(v) for k, v in t.items()})
        fed = _Recorder.fed
        out[f"match{i}:fed"] = np.int32(len(fed))
        out[f"match{i}:proba"] = fed[0][0].numpy() if fed else np.zeros(0, np.float32)
        out[f"match{i}:classes"] = fed[0][1].numpy() if fed else np.zeros(0, np.int32)
        for k, v in p.items():
            out[f"match{i}:pred:{k}"] = v
        for k, v in t.items():
            out[f"match{i}:target:{k}"] = v
        print(f"match image {i}: fed {len(fed)} update(s), hits {out[f'match{i}:proba'].shape}")
    out["match:hits"] = np.int32(metric.hits)
    np.savez_compressed(os.path.join(OUT, "detection_boxes.npz"), **out)


def gen_anchors():
    out = {}
    for name, (anch, ish, osh, thr, boxes, classes, shape) in C.ANCHOR_CASES.items():
        margin = anchor_margin(anch, ish, osh, thr, boxes, shape)
        assert margin >= C.MARGIN, (name, margin)
        t = BBToAdjustedAnchors(anch, ish, osh, thr)
        m = t(boxes, classes, shape=shape)
        out[f"{name}:map"] = m
        tl, br = t.adjusted_anchors_to_bb_vertices(m)
        for i, (x, y) in enumerate(zip(tl, br)):
            out[f"{name}:tl{i}"], out[f"{name}:br{i}"] = x, y
        set_cells = int(sum((m[1 + 7 * a] > 0).sum() for a in range(len(anch))))
        print(f"anchors {name}: {set_cells} cell(s) set, largest 'iou' {m[1::7].max():.3f}")
    np.savez_compressed(os.path.join(OUT, "detection_anchors.npz"), **out)


# ---- network steps ------------------------------------------------------------------------------------
def run_steps(name, gain, dt):
    seen = []

    def reg(*args):
        seen.append(out := ciou_in_dtype(*args))
        return out

    net = C.build_net(name, RPL.YOLONet3dPL, get_adn_fn, reg_loss_fn=reg,
                      classification_loss_fn=(F.binary_cross_entropy if C.NET_CONFIGS[name]["n_classes"] == 2
                                              else F.cross_entropy), iou_threshold=C.IOU_THRESHOLD)
    keys = list(net.state_dict().keys())
    shapes = [tuple(v.shape) for v in net.state_dict().values()]
    C.fill_net(net, gain)
    net = net.to(dt).train()
    label = C.net_label(name, BBToAdjustedAnchors)
    for bx in C.NET_BOXES:
        m = anchor_margin(C.NET_CONFIGS[name]["anchor_sizes"], C.SHAPE[2:], C.OUT_SH, 0.3, bx)
        assert m >= C.MARGIN, (name, m)
    batch = C.net_batch(name, label, torch, dtype=dt)
    batch["label"] = batch["label"].to(dt)
    opt = torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=C.STEP_LR,
                            weight_decay=C.STEP_WD, amsgrad=True, eps=C.STEP_EPS)
    out = {"label": torch.from_numpy(label)}
    for s in (1, 2):
        opt.zero_grad()
        loss = net.step(batch, 0, {})
        loss.backward()
        for k, v in zip(("iou", "cpd", "ar"), seen[-1]):          # per positive, torch.where's order
            out[f"{k}{s}"] = v.detach()
        out[f"loss{s}"] = loss.detach()
        if s == 1:
            for k, p in net.named_parameters():
                # (the class head of a two-class network takes no part in the loss: no gradient)
                if p.requires_grad and p.grad is not None:
                    out["grad:" + k] = p.grad.clone()
        opt.step()
        for k, v in net.state_dict().items():
            out[f"step{s}:" + k] = v.detach().clone()
    net.eval()
    with torch.no_grad():
        out["val_loss"] = net.step(batch, 0, {}).detach()
        heads = net(batch["image"])
        for k, v in zip(("centre", "size", "obj", "cls"), heads):
            out["val:" + k] = v.detach()
    pos = (batch["label"][:, 1::7] > C.IOU_THRESHOLD).sum()
    assert int(pos) > 0, "no positive cell in the step fixture"
    return out, keys, shapes


class _Grads(dict):
    @property
    def files(self):
        return list(self)


def within_quarter(o32, o64):
    q, worst, ok = 0.25, {"grad": 0.0, "param": 0.0}, True
    for k in ("loss1", "loss2", "val_loss"):
        worst[k] = abs(float(o32[k]) - float(o64[k])) / abs(float(o64[k]))
        ok &= worst[k] <= q * TOL["loss"]
    grads = _Grads({k: v.numpy() for k, v in o64.items() if k.startswith("grad:")})
    for k in o64:
        if k.startswith("grad:"):
            e = grad_rel_err(grads, k[5:], o32[k].double().numpy())
            worst["grad"] = max(worst["grad"], e)
            ok &= e <= q * TOL["grad"]
        elif k.startswith("step") and o64[k].is_floating_point():
            rt, at = TOL["param"]
            a, r = o32[k].double(), o64[k].double()
            e = float(((a - r).abs() / (at + rt * r.abs())).max())
            worst["param"] = max(worst["param"], e)
            ok &= e <= q
    return bool(ok), worst


def gen_steps():
    report = {}
    for name in C.NETS:
        found = None
        for gain in (1.0, 0.75, 0.5, 1.5):
            try:
                o64, keys, shapes = run_steps(name, gain, torch.float64)
            except RuntimeError as e:       # a predicted box that misses its target: "iou" outside [0, 1]
                print(f"step {name}: gain {gain}: {e}")
                worst = str(e)
                continue
            o32 = run_steps(name, gain, torch.float32)[0]
            ok, worst = within_quarter(o32, o64)
            if ok:
                found = gain
                break
        if found is None:
            raise SystemExit(f"{name}: no gain keeps the reference's fp32 steps within a quarter of the "
                             f"tolerances; last worst {worst}")
        out = {"gain": np.float64(found), "state_keys": np.array(keys),
               "state_shapes": np.array([",".join(str(d) for d in s) for s in shapes]),
               "fp32_vs_fp64": np.array([worst[k] for k in sorted(worst)]),
               "fp32_vs_fp64_names": np.array(sorted(worst))}
        for k, v in o64.items():
            if "loss" in k or k == "label":
                out[k] = v.double().numpy()
            elif v.is_floating_point():
                out[k] = v.float().numpy()
            else:
                out[k] = v.numpy()
        # three files, each under the 1 MiB of a committed file: the parameters after the two steps apart
        for step in (1, 2):
            params = {k: out.pop(k) for k in list(out) if k.startswith(f"step{step}:")}
            ppath = os.path.join(OUT, f"detection_step_{name}_params{step}.npz")
            np.savez_compressed(ppath, **params)
            assert os.path.getsize(ppath) < 1 << 20, os.path.getsize(ppath)
        path = os.path.join(OUT, f"detection_step_{name}.npz")
        np.savez_compressed(path, **out)
        report[name] = worst
        print(f"step {name}: gain {found}, losses {float(o64['loss1']):.6f} {float(o64['loss2']):.6f} val "
              f"{float(o64['val_loss']):.6f}; fp32 vs fp64 (1 = the tolerance; loss relative): {worst}; "
              f"{os.path.getsize(path)} bytes")
        assert os.path.getsize(path) < 1 << 20
    return report


def gen_meta():
    from adell_mri.modules.object_detection import nets as RN

    meta = {}
    for cls in (RN.YOLONet3d, RPL.YOLONet3dPL):
        sig = inspect.signature(cls.__init__)
        meta[cls.__name__] = {"signature": [[p.name, str(p.kind), repr(p.default) if p.name not in (
            "adn_fn", "anchor_sizes", "reg_loss_fn", "classification_loss_fn", "object_loss_fn")
            and p.default is not inspect.Parameter.empty else None] for p in sig.parameters.values()]}
    for name in C.NETS:
        net = C.build_net(name, RN.YOLONet3d, get_adn_fn)
        meta[name] = {"state_dict": [[k, list(v.shape)] for k, v in net.state_dict().items()],
                      "parameters": int(sum(p.numel() for p in net.parameters()))}
    with open(os.path.join(OUT, "detection_meta.json"), "w") as f:
        json.dump(meta, f, indent=0)


if __name__ == "__main__":
    gen_meta()
    gen_anchors()
    gen_boxes()
    print(gen_loss())
    print(gen_steps())
    for f in sorted(os.listdir(OUT)):
        if f.startswith("detection_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))
