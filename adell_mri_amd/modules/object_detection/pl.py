"""``YOLONet3dPL`` (mirror of adell_mri/modules/object_detection/pl.py:38-433): every constructor
argument, ``calculate_loss``, ``retrieve_correct``, ``calculate_correction_factor``, ``step`` and the
three step methods, ``configure_optimizers`` (``FusedAdamW(amsgrad=True)`` for
``torch.optim.AdamW(amsgrad=True)``, the cosine schedule with warm-up) and the three metric dicts under
the reference's names, built from ``classification_metrics`` (torchmetrics is not installed).

Two paths through ``step``. With ``reg_loss_fn is complete_iou_loss``, ``object_loss_fn is
F.binary_cross_entropy``, no ``object_loss_params`` and GPU tensors, the loss is
``functional.detection_loss`` (csrc/detect.hip): positive cells tabulated on the device, the heads and
the anchor map read in place -- no ``split`` / ``stack`` copy --, the dense objectness target never
written, and the cross-entropy's gradient through its un-detached IoU target kept. For ``n_classes ==
2`` that step reads nothing on the host; for more classes the class term (``torch.unique`` over the
cells, the loss on the soft-maxed head, as written) reads the positive count once. The centre / size /
objectness metrics then come from masked sums over the same tensors. Any other callable, or CPU
tensors, take the composite in plain torch ops as the reference writes it (``calculate_loss``), which
is also this package's oracle for the fused path. With no positive cell both give NaN (the means of
empty tensors).

``CoarseDetector3dPL`` raises ``NotImplementedError`` (``nets.CoarseDetector3d``)."""
from typing import Callable, Tuple, Union

import numpy as np
import torch
import torch.nn.functional as F

from ... import classification_metrics as CM
from ... import functional as HF
from ...optim import FusedAdamW
from ..learning_rate import CosineAnnealingWithWarmupLR
from .losses import complete_iou_loss
from .map import mAP
from .nets import CoarseDetector3d, YOLONet3d

try:  # pragma: no cover - lightning is not installed in the build image
    import lightning.pytorch as pl

    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    _Base = torch.nn.Module

OPTIMIZER_EPS_DEFAULT = 1e-8


def real_boxes_from_centres_sizes(centres: torch.Tensor, sizes: torch.Tensor, anchors: torch.Tensor,
                                  h: torch.Tensor, w: torch.Tensor, d: torch.Tensor, a: torch.Tensor,
                                  correction_factor: torch.Tensor
                                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    centres[:, 0] = centres[:, 0] + h
    centres[:, 1] = centres[:, 1] + w
    centres[:, 2] = centres[:, 2] + d
    centres = centres * correction_factor
    anchors = torch.stack(torch.split(anchors.squeeze(), 3))
    sizes = torch.exp(sizes)
    sizes = sizes * anchors[a] / 2
    tl_corner = centres - sizes
    br_corner = centres + sizes
    return tl_corner, br_corner, centres, sizes


class _MeanSquaredError(torch.nn.Module):
    """Mean squared error of real values (torchmetrics' ``MeanSquaredError``): fp64 sum and count on
    the device, the surface of the ``classification_metrics`` classes."""

    num_classes = 2

    def __init__(self):
        super().__init__()
        self.state = torch.zeros(2, dtype=torch.float64)

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.state = fn(self.state).to(torch.float64)     # device moves; the sums stay fp64
        return self

    def update_sums(self, squared_error_sum, count):
        delta = torch.stack([squared_error_sum.double().reshape(()), count.double().reshape(())])
        if self.state.device != delta.device:
            self.state = self.state.to(delta.device)
        self.state = self.state + delta

    def update(self, preds, target):
        diff = preds.detach().double() - target.detach().double()
        self.update_sums((diff * diff).sum(), torch.tensor(float(diff.numel()), device=diff.device))

    def forward(self, preds, target):
        self.update(preds, target)

    def compute_async(self):
        return (self.state[0] / self.state[1]).float(), torch.zeros((), device=self.state.device)

    def compute(self):
        return self.compute_async()[0]

    def reset(self):
        self.state = torch.zeros_like(self.state)


class YOLONet3dPL(YOLONet3d, _Base):
    if _Base is torch.nn.Module:
        def log(self, *args, **kwargs):
            return None

    def __init__(self, image_key: str = "image", label_key: str = "label", boxes_key: str = "boxes",
                 box_label_key: str = "labels", learning_rate: float = 0.001, batch_size: int = 4,
                 weight_decay: float = 0.005, training_dataloader_call: Callable = None,
                 reg_loss_fn: Callable = F.mse_loss,
                 classification_loss_fn: Callable = F.binary_cross_entropy,
                 object_loss_fn: Callable = F.binary_cross_entropy, positive_weight: float = 1.0,
                 classification_loss_params: dict = {}, object_loss_params: dict = {},
                 iou_threshold: float = 0.5, n_epochs: int = 100,
                 warmup_steps: Union[int, float] = 0, start_decay: int = None,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs) -> torch.nn.Module:
        super().__init__(*args, **kwargs)

        self.image_key = image_key
        self.label_key = label_key
        self.boxes_key = boxes_key
        self.box_label_key = box_label_key
        self.learning_rate = learning_rate
        self.batch_size = batch_size
        self.weight_decay = weight_decay
        self.training_dataloader_call = training_dataloader_call
        self.reg_loss_fn = reg_loss_fn
        self.classification_loss_fn = classification_loss_fn
        self.object_loss_fn = object_loss_fn
        self.positive_weight = positive_weight
        self.classification_loss_params = classification_loss_params
        self.object_loss_params = object_loss_params
        self.iou_threshold = iou_threshold
        self.n_epochs = n_epochs
        self.warmup_steps = warmup_steps
        self.start_decay = start_decay
        self.optimizer_eps = optimizer_eps

        self.object_idxs = np.array([0])
        self.center_idxs = np.array([1, 2, 3])
        self.size_idxs = np.array([4, 5, 6])
        self.class_idxs = np.array([7])

        self.setup_metrics()

        self.loss_accumulator = 0.0
        self.loss_accumulator_d = 0.0

    # ---- the composite, as the reference writes it ------------------------------------------------
    def calculate_loss(self, prediction, y, y_class, b, h, w, d, a, correction_factor, weights=None):
        bb_center, bb_size, bb_object, bb_cl = prediction
        pred_centers = bb_center[b, :, h, w, d, a]
        y_centers = y[:, self.center_idxs][b, :, h, w, d, a]
        pred_size = bb_size[b, :, h, w, d, a]
        y_size = y[:, self.size_idxs][b, :, h, w, d, a]

        tl_pred, br_pred, centers_pred, _ = real_boxes_from_centres_sizes(
            pred_centers, pred_size, self.anchor_tensor, h, w, d, a, correction_factor)
        tl_y, br_y, centers_y, _ = real_boxes_from_centres_sizes(
            y_centers, y_size, self.anchor_tensor, h, w, d, a, correction_factor)

        pred_corners = torch.cat([tl_pred, br_pred], 1)
        y_corners = torch.cat([tl_y, br_y], 1)
        iou, cpd, ar = self.reg_loss_fn(pred_corners, y_corners, centers_pred, centers_y)
        y_object = torch.zeros_like(bb_object, device=iou.device)
        y_object[b, :, h, w, d, a] = torch.unsqueeze(iou, 1)

        obj_loss = self.object_loss_fn(bb_object, y_object, **self.object_loss_params)

        obj_weight = 1.0
        box_weight = 0.1
        output = obj_loss.mean() * obj_weight
        output = output + ((1 - iou).mean() + cpd.mean() + ar.mean()) * box_weight
        if self.n_classes > 2:
            output = output + self._class_term(bb_cl, y_class, b, h, w, d)
        return output.mean()

    def _class_term(self, bb_cl, y_class, b, h, w, d):
        b_c, h_c, w_c, d_c = torch.split(torch.unique(torch.stack([b, h, w, d], 1), dim=0), 1, dim=1)
        pred_class_for_loss = bb_cl[b_c, :, h_c, w_c, d_c].squeeze(1)
        y_class_for_loss = y_class[b_c, h_c, w_c, d_c].squeeze()
        y_class_for_loss = y_class_for_loss.long()
        cla_loss = self.classification_loss_fn(pred_class_for_loss, y_class_for_loss,
                                               **self.classification_loss_params)
        return cla_loss.mean()

    def retrieve_correct(self, prediction, target, target_class, typ, b, h, w, d, a,
                         correction_factor=None):
        typ = typ.lower()
        if typ == "center":
            p, t = prediction[0], target[:, self.center_idxs, :, :, :, :]
        elif typ == "size":
            p, t = prediction[1], target[:, self.size_idxs, :, :, :, :]
        elif typ == "obj":
            p, t = prediction[2], target[:, self.object_idxs, :, :, :, :]
            t = (t > self.iou_threshold).int()
        elif typ == "class":
            p, t = prediction[3], target_class
            t = torch.round(t).int()
        elif typ == "map":
            p = self.recover_boxes_batch(*prediction, correction_factor=correction_factor,
                                         to_dict=True)
            t = None
        if typ not in ["obj", "map", "class"]:
            p, t = p[b, :, h, w, d, a], t[b, :, h, w, d, a]
        elif typ == "class":
            p, t = p[b, :, h, w, d], t[b, h, w, d]
        return p, t

    def calculate_correction_factor(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        corr_fac = torch.as_tensor(np.array(x.shape[2:]))
        corr_fac = corr_fac / torch.as_tensor(np.array(y.shape[2:]))
        corr_fac = corr_fac.to(x.device)
        return corr_fac

    def fused_loss(self, x) -> bool:
        """Whether ``step`` takes the fused loss for input ``x`` (the module text's condition)."""
        return (self.reg_loss_fn is complete_iou_loss and self.object_loss_fn is F.binary_cross_entropy
                and not self.object_loss_params and x.is_cuda)

    def _map_targets(self, batch, device):
        cur_target = [{"boxes": batch[self.boxes_key][i], "labels": batch[self.box_label_key][i]}
                      for i in range(len(batch[self.boxes_key]))]
        for t in cur_target:
            t["boxes"] = torch.as_tensor(t["boxes"])
            if len(t["boxes"].shape) == 2:
                t["boxes"] = torch.concat([t["boxes"][:, :3], t["boxes"][:, 3:]], axis=1)
            else:
                t["boxes"] = torch.concat([t["boxes"][:, :, 0], t["boxes"][:, :, 1]], axis=1)
            t["boxes"] = t["boxes"].to(device)
            t["labels"] = torch.as_tensor(t["labels"]).to(device)
        return cur_target

    def step(self, batch, batch_idx, metrics):
        x, y = batch[self.image_key], batch[self.label_key].float()
        if self.fused_loss(x):
            return self._step_fused(batch, x, y, list(self.forward(x)), metrics)
        corr_fac = self.calculate_correction_factor(x, y)
        prediction = list(self.forward(x))
        y_class, y = y[:, 0, :, :, :], y[:, 1:, :, :, :]
        y = torch.stack(self.split(y, self.n_b, 1), -1)
        b, h, w, d, a = torch.where(y[:, 0, :, :, :, :] > self.iou_threshold)
        prediction[:-1] = [torch.stack(self.split(x, self.n_b, 1), -1) for x in prediction[:-1]]

        loss = self.calculate_loss(prediction, y, y_class, b, h, w, d, a, correction_factor=corr_fac)

        for k_typ in metrics:
            k, typ = k_typ.split("_")
            typ = typ.lower()
            if typ != "map":
                cur_pred, cur_target = self.retrieve_correct(prediction, y, y_class, typ, b, h, w, d, a)
                if typ == "obj":
                    cur_pred, cur_target = cur_pred.reshape(-1), cur_target.reshape(-1)
                elif typ == "class" and cur_pred.shape[0] == 0:
                    continue
                metrics[k_typ](cur_pred.detach(), cur_target)
            else:
                cur_pred, _ = self.retrieve_correct(prediction, y, y_class, typ, b, h, w, d, a,
                                                    correction_factor=corr_fac)
                metrics[k_typ](cur_pred, self._map_targets(batch, loss.device))
            self.log(k, metrics[k_typ], on_epoch=True, on_step=False, prog_bar=True, sync_dist=True,
                     batch_size=x.shape[0])
        return loss

    def _step_fused(self, batch, x, y, prediction, metrics):
        centre, size, obj, cls = prediction
        A = self.n_b
        # calculate_correction_factor from the shapes, kept on the host (the kernels take three floats)
        corr = [float(np.float32(i) / np.float32(o)) for i, o in zip(x.shape[2:], y.shape[2:])]
        # The three heads must share one memory layout (all channels last, as the conv and activation
        # kernels leave them, or all channel-major): the kernels take one flag for them, and
        # ops._det_layout raises AdellHipError for a mix rather than copy a head.
        loss, _, box_terms, table, count = HF.detection_loss(centre, size, obj, y, self.anchor_tensor,
                                                             corr, self.iou_threshold, first_channel=1,
                                                             return_parts=True)
        # iou, cpd, ar (rows 0..2) of the positives in the table's order, valid up to ``count``:
        # device tensors, kept for inspection
        self.last_box_terms = (box_terms, count)
        rows = None
        if self.n_classes > 2 or any(k.split("_")[1].lower() == "class" for k in metrics):
            rows = table[:int(count)].long()                 # the one host read of this path
        if self.n_classes > 2:
            b, h, w, d = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
            loss = loss + self._class_term(cls, y[:, 0], b, h, w, d)
        # metrics: masked sums over the heads and the map, anchors as a view (no copy of a head)
        t_map = y[:, 1:].unflatten(1, (A, 7))
        mask = t_map[:, :, 0] > self.iou_threshold
        for k_typ in metrics:
            k, typ = k_typ.split("_")
            typ = typ.lower()
            if typ in ("center", "size"):
                p = (centre if typ == "center" else size).detach().unflatten(1, (A, 3))
                t = t_map[:, :, 1:4] if typ == "center" else t_map[:, :, 4:7]
                se = torch.where(mask[:, :, None], (p - t).double() ** 2, 0.0).sum()
                metrics[k_typ].update_sums(se, mask.sum() * 3)
            elif typ == "obj":
                # both flattened in the head's memory order: a view of the head, no copy of it
                order = (0, 2, 3, 4, 1) if obj.is_contiguous(memory_format=torch.channels_last_3d) \
                    else (0, 1, 2, 3, 4)
                metrics[k_typ](obj.detach().permute(order).reshape(-1),
                               mask.permute(order).int().reshape(-1))
            elif typ == "class":
                if rows.shape[0] > 0:
                    b, h, w, d = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
                    metrics[k_typ](cls.detach()[b, :, h, w, d], torch.round(y[:, 0][b, h, w, d]).int())
            elif typ == "map":
                cur_pred = self.recover_boxes_batch(centre, size, obj, cls, correction_factor=corr,
                                                    to_dict=True)
                metrics[k_typ](cur_pred, self._map_targets(batch, loss.device))
            self.log(k, metrics[k_typ], on_epoch=True, on_step=False, prog_bar=True, sync_dist=True,
                     batch_size=x.shape[0])
        return loss

    def training_step(self, batch, batch_idx):
        batch_size = batch[self.image_key].shape[0]
        loss = self.step(batch, batch_idx, self.train_metrics)
        self.log("loss", loss, prog_bar=True, on_step=True, batch_size=batch_size)
        return loss

    def validation_step(self, batch, batch_idx):
        batch_size = batch[self.image_key].shape[0]
        loss = self.step(batch, batch_idx, self.val_metrics)
        self.log("val_loss", loss, prog_bar=True, on_epoch=True, batch_size=batch_size)
        return loss

    def test_step(self, batch, batch_idx):
        batch_size = batch[self.image_key].shape[0]
        loss = self.step(batch, batch_idx, self.test_metrics)
        self.log("test_loss", loss, on_epoch=True, batch_size=batch_size)
        return loss

    def train_dataloader(self):
        return self.training_dataloader_call()

    def configure_optimizers(self) -> dict:
        optimizer = FusedAdamW(self.parameters(), lr=self.learning_rate,
                               weight_decay=self.weight_decay, amsgrad=True, eps=self.optimizer_eps)
        lr_schedulers = CosineAnnealingWithWarmupLR(optimizer, T_max=self.n_epochs,
                                                    start_decay=self.start_decay,
                                                    n_warmup_steps=self.warmup_steps)
        return {"optimizer": optimizer, "lr_scheduler": lr_schedulers, "monitor": "val_loss"}

    def setup_metrics(self):
        thr = self.iou_threshold
        self.train_metrics = torch.nn.ModuleDict({
            "cMSE_center": _MeanSquaredError(),
            "sMSE_size": _MeanSquaredError(),
            "objF1_obj": CM.BinaryFBetaScore(1.0, threshold=thr),
            "objRec_obj": CM.BinaryRecall(threshold=thr),
        })
        self.val_metrics = torch.nn.ModuleDict({
            "v:cMSE_center": _MeanSquaredError(),
            "v:sMSE_size": _MeanSquaredError(),
            "v:objF1_obj": CM.BinaryFBetaScore(1.0, threshold=thr),
            "v:mAP_mAP": mAP(iou_threshold=thr, n_classes=self.n_classes),
        })
        self.test_metrics = torch.nn.ModuleDict({
            "t:cMSE_center": _MeanSquaredError(),
            "t:sMSE_size": _MeanSquaredError(),
            "t:objRec_obj": CM.BinaryRecall(threshold=thr),
            "t:objPre_obj": CM.BinaryPrecision(threshold=thr),
            "t:objF1_obj": CM.BinaryFBetaScore(1.0, threshold=thr),
            "t:mAP_mAP": mAP(iou_threshold=thr),
        })
        if self.n_classes > 2:
            # no point in including this in the two class scenario
            C = self.n_classes
            self.train_metrics["clF1_class"] = CM.MulticlassFBetaScore(C, average="macro")
            self.val_metrics["v:clF1_class"] = CM.MulticlassFBetaScore(C, average="macro")
            self.test_metrics["t:clF1_class"] = CM.MulticlassFBetaScore(C, average="macro")


class CoarseDetector3dPL(CoarseDetector3d, _Base):
    """Raises ``NotImplementedError`` at construction, as ``CoarseDetector3d`` does."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
