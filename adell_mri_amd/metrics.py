"""Segmentation metrics on the device, with torchmetrics' surface (``update`` / ``compute`` /
``reset`` / ``to``) and names, for the metric dicts of the segmentation wrappers
(adell_mri/modules/segmentation/pl.py:100-187, 655-671). torchmetrics is not a dependency.

Every metric keeps int64 confusion counts (tp, fp, fn per class) and a bad-target flag on the
device; ``update`` adds the counts of one prediction with two HIP launches
(``csrc/seg_metrics.hip``: a partial pass and a one-block finalize) and never synchronises with
the host. One update may feed several metrics at once (``update_many``): a wrapper's whole dict
costs one pass over the prediction.

Values, from the counts accumulated over every voxel of every update since the last ``reset()``
(torchmetrics' ``multidim_average="global"``, legacy ``mdmc_average="global"``), computed in fp64
and returned as a 0-dim fp32 device tensor:

=========  =========================================  ========================
metric     value                                      zero denominator
=========  =========================================  ========================
IoU        tp / (tp + fp + fn)                        0
Precision  tp / (tp + fp)                             0
F-beta     (1+b^2) tp / ((1+b^2) tp + b^2 fn + fp)    0
Dice       2 tp / (2 tp + fp + fn)                    0
=========  =========================================  ========================

The zero case is torchmetrics 1.6's ``zero_division=0`` (the reference's pin): an update with no
foreground in either tensor gives 0, not 1.

Binary (one prediction channel): a voxel is positive when ``p > 0.5``; when any prediction of an
update lies outside [0, 1] (NaN included) that update uses ``sigmoid(p) > 0.5`` instead
(torchmetrics' rule, checked per update). Targets are rounded half-to-even (``torch.round``) and
must be 0 or 1. The reference feeds Dice ``p.round().long()`` and the other metrics ``p``
(pl.py:139-144); for probabilities both give the mask ``p > 0.5`` (round(0.5) = 0). For
predictions out of range Dice uses the sigmoid mask here too: the one deviation.

Multi-class (C channels, 2 <= C <= 32): the predicted class is ``argmax`` over the channels (the
first maximal index; a NaN wins, as in ``torch.argmax``); targets are class indices in [0, C).
``average="macro"`` is the mean over the classes with tp + fp + fn > 0, and 0 when there are none.
This definition is the package's own: the reference's multi-class branch (pl.py:178-184) cannot
be constructed under its pinned torchmetrics (``JaccardIndex`` / ``Precision`` / ``FBetaScore``
take ``task`` first, legacy ``Dice(nc, ...)`` reads ``nc`` as ``zero_division``).

Bad targets: torchmetrics raises in ``update``; here ``update`` cannot look at the data without a
host synchronisation, so it records a flag and ``compute`` raises ``RuntimeError``.

State: plain tensor attributes moved by an ``_apply`` override (as torchmetrics does), not
registered buffers, so ``parameters()``, ``buffers()`` and ``state_dict()`` of a module holding
metrics are those of the module without them. When ``torch.distributed`` is initialised with
more than one rank, ``compute`` first sums the counts over the ranks (one ``all_reduce`` of the
small int64 vector: torchmetrics' ``sync_dist``); the local counts stay as they are.
"""
import torch

from . import ops

MAX_CLASSES = ops.SEG_MAX_CLASSES


class SegMetric(torch.nn.Module):
    """Base of the metric objects: ``kind`` is one of ops.SEG_METRIC_KINDS."""

    kind = None

    def __init__(self, num_classes: int = 1, beta: float = 1.0):
        super().__init__()
        num_classes = int(num_classes)
        if not 1 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"{type(self).__name__}: num_classes must be in [1, {MAX_CLASSES}] "
                             f"(multi-class needs >= 2), got {num_classes}")
        if not beta > 0:
            raise ValueError(f"{type(self).__name__}: beta must be positive, got {beta}")
        self.num_classes = num_classes
        self.beta = float(beta)
        self.state = torch.zeros(3 * num_classes + 1, dtype=torch.int64)

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.state = fn(self.state)       # device moves; dtype casts leave integer tensors alone
        return self

    @property
    def device(self):
        return self.state.device

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        update_many([self], preds, target)

    def reset(self) -> None:
        self.state.zero_()

    def _synced_state(self):
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            s = self.state.clone()
            dist.all_reduce(s)
            return s
        return self.state

    def compute_async(self):
        """(value, bad-target count) as device tensors: no host synchronisation. ``compute`` and
        the trainer's loops check the count."""
        s = self._synced_state()
        return ops.seg_metric_compute(s, self.kind, self.beta, self.num_classes), s[-1]

    def compute(self) -> torch.Tensor:
        value, bad = self.compute_async()
        if int(bad) > 0:
            raise RuntimeError(bad_target_message(self.num_classes))
        return value

    def extra_repr(self):
        return f"num_classes={self.num_classes}" + (f", beta={self.beta}" if self.kind == "fbeta" else "")


def bad_target_message(num_classes):
    allowed = "{0, 1}" if num_classes == 1 else f"[0, {num_classes})"
    return (f"segmentation metric: a target value (after rounding) lies outside {allowed} "
            f"in an update since the last reset()")


def _as_segmentation(preds, target, num_classes):
    """(pred [B, C, *spatial], target) for ops.seg_confusion_update."""
    if num_classes == 1:
        if preds.shape != target.shape and not (preds.dim() == target.dim() + 1 and preds.shape[1] == 1
                                                and preds.shape[:1] + preds.shape[2:] == target.shape):
            raise ValueError(f"binary metric: preds {tuple(preds.shape)} and target "
                             f"{tuple(target.shape)} do not match")
        if preds.dim() >= 3 and preds.shape[1] == 1:
            return preds, target
        return preds.reshape(1, 1, -1), target.reshape(1, -1)
    if preds.dim() < 2 or preds.shape[1] != num_classes:
        raise ValueError(f"multi-class metric: preds {tuple(preds.shape)} must be [B, {num_classes}, ...]")
    if preds.dim() == 2:
        return preds.unsqueeze(-1), target.reshape(-1, 1)
    return preds, target


def update_many(metrics, preds, target):
    """One fused update of every metric in ``metrics`` (all of the same number of classes) with
    the same prediction and target: two launches per 8 metrics, no host synchronisation."""
    metrics = list(metrics)
    if not metrics:
        return
    C = metrics[0].num_classes
    if any(m.num_classes != C for m in metrics):
        raise ValueError("update_many: the metrics differ in their number of classes")
    if preds.dtype != torch.float32:
        if not preds.is_floating_point():
            raise ValueError(f"segmentation metrics take floating-point predictions, got {preds.dtype}")
        preds = preds.float()
    pred, tgt = _as_segmentation(preds.detach(), target.detach(), C)
    for m in metrics:
        if m.state.device != pred.device:
            m.state = m.state.to(pred.device)
    for i in range(0, len(metrics), 8):
        ops.seg_confusion_update(pred, tgt, [m.state for m in metrics[i:i + 8]])


class BinaryJaccardIndex(SegMetric):
    kind = "iou"

    def __init__(self):
        super().__init__(1)


class BinaryPrecision(SegMetric):
    kind = "precision"

    def __init__(self):
        super().__init__(1)


class BinaryFBetaScore(SegMetric):
    kind = "fbeta"

    def __init__(self, beta: float):
        super().__init__(1, beta)


class Dice(SegMetric):
    """The legacy ``torchmetrics.Dice`` as the reference builds it for two classes
    (pl.py:171): ``Dice(num_classes=1, multiclass=False)``, nothing else."""

    kind = "dice"

    def __init__(self, num_classes: int = 1, multiclass: bool = False, **kwargs):
        if num_classes != 1 or multiclass or kwargs:
            raise NotImplementedError(
                "Dice: only Dice(num_classes=1, multiclass=False), the binary form the reference "
                "builds, is implemented; the reference's multi-class Dice(nc, average='macro') cannot "
                "be constructed under its pinned torchmetrics -- use MulticlassDice(num_classes)")
        super().__init__(1)


class _Multiclass(SegMetric):
    def __init__(self, num_classes: int, average: str = "macro", beta: float = 1.0):
        if average != "macro":
            raise NotImplementedError(f"{type(self).__name__}: only average='macro' is implemented "
                                      f"(the reference's setting), got {average!r}")
        if int(num_classes) < 2:
            raise ValueError(f"{type(self).__name__}: num_classes must be >= 2, got {num_classes}")
        super().__init__(num_classes, beta)
        self.average = average


class MulticlassJaccardIndex(_Multiclass):
    kind = "iou"


class MulticlassPrecision(_Multiclass):
    kind = "precision"


class MulticlassFBetaScore(_Multiclass):
    kind = "fbeta"


class MulticlassDice(_Multiclass):
    kind = "dice"
