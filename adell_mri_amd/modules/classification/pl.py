"""Classification training-step wrappers (mirror of adell_mri/modules/classification/pl.py):
``ClassPLABC`` (:182-778), ``ClassNetPL`` (:781-928), ``OrdNetPL`` (:931-1174),
``ViTClassifierPL`` (:1762-1845), ``TransformableTransformerPL`` (:1934-2021) and
``MultipleInstanceClassifierPL`` (:2024-2111), with the metric dicts of ``classification_metrics``.

Kept: constructor arguments, the label casts of ``calculate_loss`` (:217-223), ``additional_params``
and ``with_loss_params``, tuple losses averaged element-wise, the steps (``test_step`` returns
``(loss, prediction)``; ``OrdNetPL``'s steps return ``loss + roc_loss``), ``predict_step`` without
the Gaussian-process branch, and ``configure_optimizers`` (:623-702): the no-decay group (empty
here: it holds the Gaussian-process parameters), the ``ordinal_bias`` group at a hundredth of the
weight decay and the normal group, or the head / body split when ``weight_decay`` is a pair;
``FusedAdamW`` with ``weight_decay=base_wd`` and the cosine schedule with warm-up.

``loss_fn`` is called as it is: the classes of ``classification.losses`` (what
``configure_loss_fn`` assigns) run the fused kernels, any other callable runs as given.

``GenericEnsemblePL`` (:1504-1631) and ``AveragingEnsemblePL`` (:1634-1759) read a list of
``image_keys``; the generic one carries the Gaussian-process hooks (``fit_gaussian_process`` /
``on_train_end``, ``predict_step_gp``), and ``optimizer_groups`` puts the trainable parameters of
any ``GaussianProcessLayer`` into the no-decay group.

``DeconfoundedNetPL`` (:2275-2573) wraps ``DeconfoundedNetGeneric``: its four loss terms, Adam over
the confounder / classifier groups (see the class).

``calibrate(dataloader, alpha=0.2)`` and ``predict_calibrated_step`` (:460-479, :597-618) fit and apply
``conformal_prediction.AdaptivePredictionSets`` for every wrapper whose ``predict_step`` returns
``{"prediction": ...}``; ``OrdNetPL`` raises ``NotImplementedError`` (ordinal logits are no class
probabilities). ``calibrate`` runs under ``no_grad``. Deviations from the reference: (a) for two
classes the ``[B, 1]`` probability p is laid out as ``[1 - p, p]`` (the reference indexes a one-column
matrix with label 1 and fails); (b) both methods take ``predict_step(batch, 0)["prediction"]`` and
apply the same activation, sigmoid for two classes and softmax otherwise (the reference hands the
whole dict to the module and fails); (c) there is no tqdm; (d) the labels are flattened and cast to
int64.

Not mirrored: ``on_train_end`` and ``predict_step_gp`` of the single-network wrappers (their
Gaussian-process head is not built), and the hyper-parameter logging of ``on_train_start``.
Lightning is optional as in ``self_supervised/pl.py``.
"""
from abc import ABC
from typing import Callable

import torch

from ... import classification_metrics as CM
from ... import functional as HF
from ...optim import FusedAdam, FusedAdamW
from ..learning_rate import CosineAnnealingWithWarmupLR
from ..conformal_prediction import AdaptivePredictionSets
from ..layers.gaussian_process import GaussianProcessLayer
from .classification import CatNet, OrdNet, ViTClassifier, ordinal_prediction_to_class
from .deconfounded_classification import DeconfoundedNetGeneric
from .ensemble import AveragingEnsemble, GenericEnsemble
from .losses import BCEWithLogitsLoss
from .multiple_instance_learning import MultipleInstanceClassifier, TransformableTransformer

try:  # pragma: no cover - lightning is not installed in the build image
    import lightning.pytorch as pl

    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    _Base = torch.nn.Module

OPTIMIZER_EPS_DEFAULT = 1e-8

get_metric_dict = CM.get_metric_dict
get_ordinal_metric_dict = CM.get_ordinal_metric_dict


class ClassPLABC(_Base, ABC):
    """Abstract classification wrapper (pl.py:182-778)."""

    if _Base is torch.nn.Module:
        def log(self, *args, **kwargs):
            return None

        def save_hyperparameters(self, *args, **kwargs):
            return None

    def __init__(self):
        super().__init__()
        self.raise_nan_loss = False
        self.calibrated = False
        self.gaussian_process = False
        self.net_type = "cat"
        self.optimizer_eps = OPTIMIZER_EPS_DEFAULT

    def calculate_loss(self, prediction, y, additional_params: dict | None = None,
                       with_loss_params: bool = False):
        y = y.to(device=prediction.device)
        if self.n_classes > 2:
            if len(y.shape) > 1:
                y = y.squeeze(1)
            y = y.to(torch.int64)
        else:
            y = y.float()
        params = {}
        if additional_params is not None:
            params.update(additional_params)
        if with_loss_params is True:
            d = y.device
            params.update({k: self.loss_params[k].to(d) for k in self.loss_params})
        loss = self.loss_fn(prediction, y, **params)
        if isinstance(loss, tuple):
            return tuple(loss_element.mean() for loss_element in loss)
        return loss.mean()

    def on_batch_start(self, batch):
        dev = batch[self.image_key].device
        batch[self.label_key] = batch[self.label_key].to(dev)
        return batch

    def training_step(self, batch, batch_idx):
        x, y = batch[self.image_key], batch[self.label_key]
        if getattr(self, "training_batch_preproc", None) is not None:
            x, y = self.training_batch_preproc(x, y)
        prediction = torch.squeeze(self.forward(x), 1)
        loss = self.calculate_loss(prediction, y, with_loss_params=True)
        self.log("train_loss", loss, prog_bar=True)
        return loss

    def validation_step(self, batch, batch_idx):
        x, y = batch[self.image_key], batch[self.label_key]
        prediction = torch.squeeze(self.forward(x), 1)
        loss = self.calculate_loss(prediction, y, with_loss_params=True)
        self.log("val_loss", loss, on_epoch=True, on_step=False, prog_bar=True,
                 batch_size=x.shape[0], sync_dist=True)
        self.update_metrics(prediction, y, self.val_metrics)
        return loss

    def test_step(self, batch, batch_idx):
        x, y = batch[self.image_key], batch[self.label_key]
        prediction = torch.squeeze(self.forward(x), 1)
        loss = self.calculate_loss(prediction, y)
        self.log("test_loss", loss, on_epoch=True, on_step=False, prog_bar=True,
                 batch_size=x.shape[0], sync_dist=True)
        self.update_metrics(prediction, y, self.test_metrics, log=False)
        return loss, prediction

    def on_test_epoch_end(self):
        self.log_metrics_end_epoch(self.test_metrics)

    def predict_step(self, batch, batch_idx, dataloader_idx=0, *args, **kwargs):
        x = batch[self.image_key]
        prediction = self.forward(x, *args, **kwargs)
        if "return_features" in kwargs:
            return {"features": prediction}
        return {"prediction": prediction}

    def calibration_probabilities(self, batch):
        """Class probabilities [B, C] of a batch for the conformal calibration, from
        ``predict_step(batch, 0)["prediction"]``: softmax over the last axis, or for two classes the
        sigmoid p laid out as ``[1 - p, p]``."""
        if self.net_type == "ord":
            raise NotImplementedError(
                "conformal calibration of an ordinal network: its logits are no class probabilities")
        prediction = self.predict_step(batch, 0)["prediction"]
        if self.n_classes == 2:
            p = torch.sigmoid(prediction).reshape(-1, 1)
            return torch.cat([1 - p, p], 1)
        return torch.softmax(prediction, -1)

    def calibrate(self, dataloader, alpha: float = 0.2):
        """Calibrates adaptive prediction sets at miscoverage ``alpha`` on the batches of
        ``dataloader`` (pl.py:460-479; see the module docstring for the deviations)."""
        self.calibration = AdaptivePredictionSets(alpha)
        with torch.no_grad():
            for batch in dataloader:
                prediction = self.calibration_probabilities(batch)
                y = batch[self.label_key].reshape(-1).to(device=prediction.device, dtype=torch.int64)
                self.calibration.update(y, prediction)
            self.calibration.calculate()
        self.calibrated = True

    def predict_calibrated_step(self, batch, batch_idx, *args, **kwargs):
        """``[B, 2 C]``: the prediction set of every item as 0 / 1 floats, then the class
        probabilities (pl.py:597-618). The wrapper must be calibrated."""
        if self.calibrated is not True:
            raise RuntimeError(
                "Model needs to be calibrated before calibrated prediction"
            )
        return self.calibration(self.calibration_probabilities(batch))

    def train_dataloader(self):
        return self.training_dataloader_call()

    def optimizer_groups(self):
        """(parameter groups, base weight decay) of pl.py:632-683. The first group is the
        reference's no-decay group: the trainable parameters of every ``GaussianProcessLayer``
        (empty for a wrapper without one, and kept so that the group indices are the
        reference's)."""
        gp_ids = {id(p) for m in self.modules() if isinstance(m, GaussianProcessLayer)
                  for p in m.parameters() if p.requires_grad}
        no_decay_params, reduced_decay_params, normal_decay_params = [], [], []
        for n, p in self.named_parameters():
            if not p.requires_grad:
                continue
            if id(p) in gp_ids:
                no_decay_params.append(p)
                continue
            (reduced_decay_params if "ordinal_bias" in n else normal_decay_params).append(p)
        if isinstance(self.weight_decay, (list, tuple)):
            wd_body, wd_head = self.weight_decay
            reduced = {id(p) for p in reduced_decay_params} | gp_ids
            head_decay, body_decay = [], []
            for n, p in self.named_parameters():
                if not p.requires_grad or id(p) in reduced:
                    continue
                (head_decay if "classification" in n else body_decay).append(p)
            return [{"params": no_decay_params, "weight_decay": 0},
                    {"params": reduced_decay_params, "weight_decay": wd_body / 100},
                    {"params": head_decay, "weight_decay": wd_head},
                    {"params": body_decay, "weight_decay": wd_body}], wd_body / 100
        wd = float(self.weight_decay)
        return [{"params": no_decay_params, "weight_decay": 0},
                {"params": reduced_decay_params, "weight_decay": wd / 100},
                {"params": normal_decay_params, "weight_decay": wd}], wd / 100

    def configure_optimizers(self) -> dict:
        parameters, base_wd = self.optimizer_groups()
        optimizer = FusedAdamW(parameters, lr=self.learning_rate, weight_decay=base_wd,
                               eps=self.optimizer_eps)
        lr_schedulers = CosineAnnealingWithWarmupLR(
            optimizer, T_max=self.n_epochs, start_decay=self.start_decay,
            n_warmup_steps=self.warmup_steps)
        return {"optimizer": optimizer, "lr_scheduler": lr_schedulers, "monitor": "val_loss"}

    def setup_metrics(self):
        self.train_metrics = get_metric_dict(self.n_classes, [], prefix="")
        self.val_metrics = get_metric_dict(self.n_classes, None, prefix="V_")
        self.test_metrics = get_metric_dict(self.n_classes, None, prefix="T_", average="none")

    def update_metrics(self, prediction, y, metrics, log=True):
        """Softmax (more than two classes) or sigmoid of the logits, then one fused update of the
        dict. The probabilities are a few numbers per item: plain torch."""
        if self.n_classes > 2:
            prediction = torch.softmax(prediction.detach(), 1)
        else:
            prediction = torch.sigmoid(prediction.detach())
        if len(y.shape) > 1:
            y = y.squeeze(1)
        CM.update_many(metrics.values(), prediction, y)
        if log is True:
            for k in metrics:
                self.log(k, metrics[k], on_epoch=True, on_step=False, prog_bar=True, sync_dist=True)

    def log_metrics_end_epoch(self, metrics):
        """pl.py:746-778: a vector metric is logged as ``{key}_{i}``. Returns what it logged."""
        logged = {}
        for k in metrics:
            metric = metrics[k].compute()
            if len(metric.shape) == 0:
                metric = metric.reshape(1)
            if len(metric) > 1:
                for i in range(len(metric)):
                    logged[f"{k}_{i}"] = metric[i]
            else:
                logged[k] = metric
        for k, v in logged.items():
            self.log(k, v, on_epoch=True, on_step=False, prog_bar=True, sync_dist=True)
        return logged


def _store(module, local, names):
    for name in names:
        setattr(module, name, local[name])


_HYPERPARAMETERS = ("image_key", "label_key", "learning_rate", "batch_size", "weight_decay",
                    "training_dataloader_call", "loss_fn", "loss_params", "n_epochs", "warmup_steps",
                    "start_decay", "training_batch_preproc", "optimizer_eps", "args", "kwargs")
_IGNORED = ["training_dataloader_call", "training_batch_preproc", "loss_fn"]


class ClassNetPL(ClassPLABC):
    """pl.py:781-928: holds a ``CatNet`` as ``network`` (``net_type[:3] == "cat"``); ``"vgg"`` raises
    ``NotImplementedError``. The reference's default ``loss_fn`` is ``F.binary_cross_entropy`` on
    logits, which no caller keeps; the default here is ``BCEWithLogitsLoss()``."""

    def __init__(self, net_type: str = "cat", image_key: str = "image", label_key: str = "label",
                 learning_rate: float = 0.001, batch_size: int = 4, weight_decay: float = 0.0,
                 training_dataloader_call: Callable = None, loss_fn: Callable = None,
                 loss_params: dict = {}, n_epochs: int = 100, warmup_steps: int = 0,
                 start_decay: int = None, training_batch_preproc: Callable = None,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        super().__init__()
        loss_fn = BCEWithLogitsLoss() if loss_fn is None else loss_fn
        _store(self, locals(), _HYPERPARAMETERS)
        self.net_type = net_type[:3]
        self.save_hyperparameters(ignore=_IGNORED)
        self.setup_network()
        self.setup_metrics()
        if hasattr(self.network, "forward_features"):
            self.forward_features = self.network.forward_features

    def setup_network(self):
        if self.net_type == "cat":
            self.network = CatNet(*self.args, **self.kwargs)
        elif self.net_type == "vgg":
            raise NotImplementedError("net_type 'vgg': the VGG classifier is not built")
        else:
            raise Exception("net_type '{}' not valid, has to be one of ['cat', 'vgg']".format(
                self.net_type))
        self.forward = self.network.forward
        self.n_classes = self.network.n_classes


class OrdNetPL(ClassPLABC):
    """pl.py:931-1174: holds an ``OrdNet``; every step takes ``(loss, roc_loss)`` from the loss
    (``OrdinalSigmoidalLoss`` with the pre-bias output) and returns their sum."""

    def __init__(self, image_key: str = "image", label_key: str = "label",
                 learning_rate: float = 0.001, batch_size: int = 4, weight_decay: float = 0.0,
                 training_dataloader_call: Callable = None, loss_fn: Callable = None,
                 loss_params: dict = {}, n_epochs: int = 100, warmup_steps: int = 0,
                 start_decay: int = None, training_batch_preproc: Callable = None,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        super().__init__()
        _store(self, locals(), _HYPERPARAMETERS)
        self.net_type = "ord"
        self.save_hyperparameters(ignore=_IGNORED)
        self.setup_network()
        if self.loss_fn is None:
            from .losses import OrdinalSigmoidalLoss

            self.loss_fn = OrdinalSigmoidalLoss(self.n_classes)
        self.setup_metrics()
        if hasattr(self.network, "forward_features"):
            self.forward_features = self.network.forward_features

    def setup_network(self):
        self.network = OrdNet(*self.args, **self.kwargs)
        self.forward = self.network.forward
        self.n_classes = self.network.n_classes

    def setup_metrics(self):
        self.train_metrics = get_ordinal_metric_dict(self.n_classes, prefix="")
        self.val_metrics = get_ordinal_metric_dict(self.n_classes, prefix="V_")
        self.test_metrics = get_ordinal_metric_dict(self.n_classes, prefix="T_")

    def update_metrics(self, prediction, y, metrics, log=True):
        prediction = ordinal_prediction_to_class(torch.sigmoid(prediction.detach()))
        if len(y.shape) > 1:
            y = y.squeeze(1)
        CM.update_many(metrics.values(), prediction, y)
        if log is True:
            for k in metrics:
                self.log(k, metrics[k], on_epoch=True, on_step=False, prog_bar=True, sync_dist=True)

    def _step(self, batch, preprocess=False):
        x, y = batch[self.image_key], batch[self.label_key]
        if preprocess and getattr(self, "training_batch_preproc", None) is not None:
            x, y = self.training_batch_preproc(x, y)
        prediction, pre_bias = self.forward(x, return_pre_bias=True)
        prediction = torch.squeeze(prediction, 1)
        loss, roc_loss = self.calculate_loss(prediction, y, additional_params={"pre_bias": pre_bias},
                                             with_loss_params=True)
        return x, y, prediction, loss, roc_loss

    def training_step(self, batch, batch_idx):
        _, _, _, loss, roc_loss = self._step(batch, preprocess=True)
        self.log("train_loss", loss.detach(), prog_bar=True)
        self.log("train_roc_loss", roc_loss.detach(), prog_bar=True)
        return loss + roc_loss

    def _eval_step(self, batch, name, metrics, log):
        x, y, prediction, loss, roc_loss = self._step(batch)
        kw = dict(on_epoch=True, on_step=False, prog_bar=True, batch_size=x.shape[0], sync_dist=True)
        self.log(f"{name}_loss", loss, **kw)
        self.log(f"{name}_roc_loss", roc_loss, **kw)
        self.update_metrics(prediction, y, metrics, log=log)
        return loss + roc_loss, prediction

    def validation_step(self, batch, batch_idx):
        return self._eval_step(batch, "val", self.val_metrics, True)[0]

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, "test", self.test_metrics, False)


class ViTClassifierPL(ViTClassifier, ClassPLABC):
    """pl.py:1762-1845: the ViT classifier IS the module (its parameters carry no ``network.``
    prefix)."""

    def __init__(self, image_key: str = "image", label_key: str = "label",
                 learning_rate: float = 0.001, batch_size: int = 4, weight_decay: float = 0.0,
                 training_dataloader_call: Callable = None, loss_fn: Callable = None,
                 loss_params: dict = {}, n_epochs: int = 100, warmup_steps: int = 0,
                 start_decay: int = None, training_batch_preproc: Callable = None,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        super().__init__(*args, **kwargs)
        loss_fn = BCEWithLogitsLoss() if loss_fn is None else loss_fn
        _store(self, locals(), _HYPERPARAMETERS)
        # ClassPLABC.__init__ is not reached through ViT's: its attributes
        self.raise_nan_loss, self.calibrated, self.gaussian_process = False, False, False
        self.net_type = "cat"
        self.save_hyperparameters(ignore=_IGNORED)
        self.setup_metrics()


class _SliceClassifierPL(ClassPLABC):
    """What the two multiple-instance wrappers share: the classifier IS the module (its parameters
    carry no ``network.`` prefix, the 2-D module's sit under ``module.``). Parameters with
    ``requires_grad=False`` -- a frozen ``module`` -- stay out of the optimiser's groups
    (``optimizer_groups``). The default ``loss_fn`` is ``BCEWithLogitsLoss()``, as for
    ``ClassNetPL``."""

    def _setup_wrapper(self, local):
        local["loss_fn"] = BCEWithLogitsLoss() if local["loss_fn"] is None else local["loss_fn"]
        _store(self, local, _HYPERPARAMETERS)
        # ClassPLABC.__init__ is not reached through the classifier's: its attributes
        self.raise_nan_loss, self.calibrated, self.gaussian_process = False, False, False
        self.net_type = "cat"
        self.save_hyperparameters(ignore=["module"] + _IGNORED)
        self.setup_metrics()

    def predict_step(self, batch, batch_idx, dataloader_idx=0, *args, **kwargs):
        x = batch[self.image_key]
        output = self.forward(x, *args, **kwargs)
        if kwargs.get("return_attention", False):
            prediction, attention = output
            return {"prediction": prediction, "attention": attention}
        return {"prediction": output}


class TransformableTransformerPL(TransformableTransformer, _SliceClassifierPL):
    """pl.py:1934-2021. ``predict_step(..., return_attention=True)`` also returns the last block's
    attention."""

    def __init__(self, image_key: str = "image", label_key: str = "label",
                 learning_rate: float = 0.001, batch_size: int = 4, weight_decay: float = 0.0,
                 training_dataloader_call: Callable = None, loss_fn: Callable = None,
                 loss_params: dict = {}, n_epochs: int = 100, warmup_steps: int = 0,
                 start_decay: int = None, training_batch_preproc: Callable = None,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._setup_wrapper(locals())


class MultipleInstanceClassifierPL(MultipleInstanceClassifier, _SliceClassifierPL):
    """pl.py:2024-2111. ``predict_step(..., return_attention=True)`` also returns A [B, S, 1]."""

    def __init__(self, image_key: str = "image", label_key: str = "label",
                 learning_rate: float = 0.001, batch_size: int = 4, weight_decay: float = 0.0,
                 training_dataloader_call: Callable = None, loss_fn: Callable = None,
                 loss_params: dict = {}, n_epochs: int = 100, warmup_steps: int = 0,
                 start_decay: int = None, training_batch_preproc: Callable = None,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._setup_wrapper(locals())


_ENSEMBLE_HYPERPARAMETERS = ("image_keys", "label_key", "learning_rate", "batch_size",
                             "weight_decay", "training_dataloader_call", "loss_fn", "loss_params",
                             "n_epochs", "warmup_steps", "start_decay", "optimizer_eps", "args",
                             "kwargs")


class _EnsemblePL(ClassPLABC):
    """What the two ensemble wrappers share (pl.py:1504-1759): the ensemble IS the module, the steps
    read ``[batch[k] for k in image_keys]``, the loss takes no ``loss_params``, and ``test_step``
    returns ``(loss, prediction)`` as the base's does. The default ``loss_fn`` is
    ``BCEWithLogitsLoss()``, as for ``ClassNetPL``."""

    def _setup_wrapper(self, local):
        local["loss_fn"] = BCEWithLogitsLoss() if local["loss_fn"] is None else local["loss_fn"]
        _store(self, local, _ENSEMBLE_HYPERPARAMETERS)
        # ``gaussian_process`` is the generic ensemble's own argument; the averaging one has none
        self.raise_nan_loss, self.calibrated = False, False
        self.gaussian_process = bool(getattr(self, "gaussian_process", False))
        self.net_type = "cat"
        self.save_hyperparameters(ignore=["networks"] + _IGNORED)
        self.setup_metrics()

    def _inputs(self, batch):
        return [batch[k] for k in self.image_keys], batch[self.label_key]

    def training_step(self, batch, batch_idx):
        x, y = self._inputs(batch)
        prediction = torch.squeeze(self.forward(x), 1)
        loss = self.calculate_loss(prediction, y)
        self.log("train_loss", loss.detach())
        return loss

    def validation_step(self, batch, batch_idx):
        x, y = self._inputs(batch)
        prediction = torch.squeeze(self.forward(x), 1)
        loss = self.calculate_loss(prediction, y)
        self.log("val_loss", loss, on_epoch=True, on_step=False, prog_bar=True,
                 batch_size=x[0].shape[0])
        self.update_metrics(prediction, y, self.val_metrics)
        return loss

    def test_step(self, batch, batch_idx):
        x, y = self._inputs(batch)
        prediction = torch.squeeze(self.forward(x), 1)
        loss = self.calculate_loss(prediction, y)
        self.update_metrics(prediction, y, self.test_metrics, log=False)
        return loss, prediction

    def predict_step(self, batch, batch_idx, dataloader_idx=0, *args, **kwargs):
        x = [batch[k] for k in self.image_keys]
        prediction = torch.squeeze(self.forward(x, *args, **kwargs), 1)
        return {"prediction": prediction}


class GenericEnsemblePL(GenericEnsemble, _EnsemblePL):
    """pl.py:1504-1631, with the Gaussian-process hooks of ``ClassPLABC`` (:433-458, :487-595)
    written for this wrapper -- the reference's read ``self.network``, which it does not have:
    ``fit_gaussian_process`` / ``on_train_end``, ``predict_step_gp`` and the dispatch of
    ``predict_step``."""

    def __init__(self, image_keys: list[str] = ["image"], label_key: str = "label",
                 learning_rate: float = 0.001, batch_size: int = 4, weight_decay: float = 0.0,
                 training_dataloader_call: Callable = None, loss_fn: Callable = None,
                 loss_params: dict = {}, n_epochs: int = 100, warmup_steps: int = 0,
                 start_decay: int = None, optimizer_eps: float = OPTIMIZER_EPS_DEFAULT,
                 *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._setup_wrapper(locals())

    def classification_probabilities(self, logits):
        """pl.py:387-410 for a categorical head: sigmoid (two classes) or softmax over the class
        axis, the LAST one (the reference names axis 1, which on samples [S, N, C] is the items')."""
        if self.n_classes == 2:
            return torch.sigmoid(logits)
        return torch.softmax(logits, dim=-1)

    def fit_gaussian_process(self, batches):
        """What the reference's ``on_train_end`` does: in ``eval()`` mode and without autograd the
        precision matrix is reset, updated from every batch (one launch per batch, no host read)
        and inverted (``get_cov``). Single-rank: the precision is not reduced over ranks."""
        if not self.gaussian_process:
            raise RuntimeError("Gaussian process is not enabled for this model")
        head = self.gaussian_process_head
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                head.reset_inv_cov()
                for batch in batches:
                    rows = self.forward_head_features([batch[k] for k in self.image_keys])
                    logits, phi = head.forward_with_phi(rows)
                    head.update_inv_cov_from_phi(phi, self.classification_probabilities(logits))
                head.get_cov()
        finally:
            self.train(was_training)

    def on_train_end(self):
        if self.gaussian_process:
            self.fit_gaussian_process(self.training_dataloader_call(False))

    def predict_step(self, batch, batch_idx, dataloader_idx=0, *args, **kwargs):
        if self.gaussian_process:
            if "return_features" in kwargs:
                raise NotImplementedError(
                    "return_features=True not implemented for Gaussian process models")
            return self.predict_step_gp(batch, batch_idx, *args, **kwargs)
        return super().predict_step(batch, batch_idx, dataloader_idx, *args, **kwargs)

    def predict_step_gp(self, batch, batch_idx, n_samples=100, generator=None, eps=None):
        """The reference's keys (pl.py:514-595). ``eps`` [2, n_samples, N, o]: the standard normal
        draws of ``gp_samples`` and of the samples behind ``epistemic_uncertainty_pred`` (default:
        ``torch.randn`` on the device with ``generator``). The network runs once: in ``eval()``
        mode ``prediction`` is the head's mean. Nothing is read on the host."""
        if not self.gaussian_process:
            raise RuntimeError("Gaussian process is not enabled for this model")
        head = getattr(self, "gaussian_process_head", None)
        if head is None or not hasattr(head, "cov"):
            raise RuntimeError("Gaussian process is not fitted. Call on_fit_end() first.")
        x = [batch[k] for k in self.image_keys]
        with torch.no_grad():
            rows = self.forward_head_features(x)
            gp_mean, var = head.parameters_with_variance(rows)
            if eps is None:
                eps = torch.randn((2, n_samples, *gp_mean.shape), device=gp_mean.device,
                                  dtype=torch.float32, generator=generator)
            gp_samples, predictive_mean, predictive_std = head.sample_statistics(
                rows, n_samples, eps=eps[0], parameters=(gp_mean, var))
            mean_samples = head.sample_statistics(rows, n_samples, eps=eps[1],
                                                  parameters=(gp_mean, var))[0]
            return {
                "prediction": gp_mean,
                "gp_mean": gp_mean,
                "gp_samples": gp_samples,
                "predictive_mean": predictive_mean,
                "predictive_std": predictive_std,
                "epistemic_uncertainty": var[:, None].expand(-1, head.n_outputs),
                "predictive_std_pred": self.classification_probabilities(gp_samples).std(dim=0),
                "epistemic_uncertainty_pred":
                    self.classification_probabilities(mean_samples).std(dim=0),
            }


class AveragingEnsemblePL(AveragingEnsemble, _EnsemblePL):
    """pl.py:1634-1759."""

    def __init__(self, image_keys: list[str] = ["image"], label_key: str = "label",
                 learning_rate: float = 0.001, batch_size: int = 4, weight_decay: float = 0.0,
                 training_dataloader_call: Callable = None, loss_fn: Callable = None,
                 loss_params: dict = {}, n_epochs: int = 100, warmup_steps: int = 0,
                 start_decay: int = None, optimizer_eps: float = OPTIMIZER_EPS_DEFAULT,
                 *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._setup_wrapper(locals())


class DeconfoundedNetPL(DeconfoundedNetGeneric, ClassPLABC):
    """pl.py:2275-2573: the feature deconfounder's training wrapper. The network IS the module (its
    parameters carry no ``network.`` prefix). ``step`` returns the reference's 6-tuple
    ``(classification loss, cat_conf_loss | None, cont_conf_loss | None, feature_loss | None,
    classification, y)``; the training and validation steps return the sum of the terms present.

    On the device: ``correlation_loss`` is ``functional.deconf_correlation_loss``; with the default
    linear heads (empty ``deconfounder_structure``) inside the fused limits and the features on the
    GPU, ``step`` skips the heads' own forward and takes both confounder losses from
    ``functional.deconf_heads_loss``, which reads the feature rows in place
    (``heads_route`` names the route). Otherwise the heads run and ``loss_cat_confounder`` /
    ``loss_cont_confounder`` compose the same values. The embedder runs on the host; its integer
    tensors are stacked and uploaded once as an int64 ``[n_heads, B]`` table. A batch entry that is
    already such a table (a tensor) is taken as it is.

    ``configure_optimizers`` is Adam, not AdamW, as in the reference: ``FusedAdam`` over two groups,
    the parameters whose name contains "confound" at weight decay 0 and the rest at
    ``weight_decay``. The reference's default ``loss_fn`` is ``F.binary_cross_entropy`` on logits,
    which no caller keeps; the default here is ``BCEWithLogitsLoss()``, as for ``ClassNetPL``.
    ``cosine_loss`` is kept as written (torch's ``cosine_similarity`` along axis 1 of the broadcast
    pair); no step calls it."""

    def __init__(self, image_key: str = "image", label_key: str = "label",
                 embedder: torch.nn.Module = None, cat_confounder_key: str = None,
                 cont_confounder_key: str = None, learning_rate: float = 0.001, batch_size: int = 4,
                 weight_decay: float = 0.0, training_dataloader_call: Callable = None,
                 loss_fn: Callable = None, loss_params: dict = {}, n_epochs: int = 100,
                 warmup_steps: int = 0, start_decay: int = None,
                 training_batch_preproc: Callable = None,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        super().__init__(*args, **kwargs)
        loss_fn = BCEWithLogitsLoss() if loss_fn is None else loss_fn
        _store(self, locals(), _HYPERPARAMETERS)
        self.embedder = embedder
        self.cat_confounder_key = cat_confounder_key
        self.cont_confounder_key = cont_confounder_key
        self.loss_str = ["loss", "cat_loss", "cont_loss", "feat_loss"]
        self.conf_mult = 1.0
        self.save_hyperparameters(ignore=_IGNORED)
        self.setup_metrics()

    # ---- the confounder targets -------------------------------------------------------------------
    def cat_confounder_table(self, y, device):
        """The int64 ``[n_heads, B]`` device table of the categorical confounders: a tensor is taken
        as that table, anything else goes through the embedder on the host and is uploaded once."""
        if torch.is_tensor(y):
            return y.to(device=device, dtype=torch.int64)
        table = torch.stack([t.to(torch.int64) for t in self.embedder(y)])
        if torch.device(device).type == "cuda":
            return table.pin_memory().to(device, non_blocking=True)
        return table.to(device)

    # ---- losses -------------------------------------------------------------------------------------
    def loss_cat_confounder(self, pred, y):
        table = self.cat_confounder_table(y, pred[0].device)
        return sum(HF.cross_entropy(p, y_) / len(pred) for p, y_ in zip(pred, table)) * self.conf_mult

    def loss_cont_confounder(self, pred, y):
        return HF.mse_loss(pred, torch.as_tensor(y).to(pred)) * self.conf_mult

    def correlation_loss(self, features):
        return HF.deconf_correlation_loss(features, self.n_features_deconfounder)

    def cosine_loss(self, features):
        conf_f = features[:, :self.n_features_deconfounder, None]
        deconf_f = features[:, None, self.n_features_deconfounder:]
        return torch.nn.functional.cosine_similarity(conf_f, deconf_f).mean()

    def loss_features(self, features):
        if self.n_features_deconfounder > 0:
            return self.correlation_loss(features)

    def heads_route(self, device=None):
        """ "fused" when ``step`` takes the confounder losses from ``deconf_heads_loss`` for tensors
        on ``device`` (default: the parameters'), else "composed"."""
        device = next(self.parameters()).device if device is None else torch.device(device)
        heads = self.linear_heads()
        want_cat = self.cat_confounder_key is not None and len(self.n_cat_deconfounder) > 0
        want_cont = self.cont_confounder_key is not None and self.n_cont_deconfounder > 0
        if heads is None or device.type != "cuda" or not (want_cat or want_cont):
            return "composed"
        return HF.deconf_route(self.n_features_deconfounder,
                               self.n_cat_deconfounder if want_cat else [],
                               self.n_cont_deconfounder if want_cont else 0)

    def fused_confounder_losses(self, batch, features):
        """``(cat_conf_loss | None, cont_conf_loss | None)`` of the linear heads from the feature rows
        in place (``functional.deconf_heads_loss``): the heads whose key is set."""
        cat_heads, cont_head = self.linear_heads()
        table = cont_target = None
        if self.cat_confounder_key is not None and cat_heads:
            table = self.cat_confounder_table(batch[self.cat_confounder_key], features.device)
        else:
            cat_heads = []
        if self.cont_confounder_key is not None and cont_head is not None:
            cont_target = torch.as_tensor(batch[self.cont_confounder_key]).to(features)
        else:
            cont_head = None
        return HF.deconf_heads_loss(features, self.n_features_deconfounder, cat_heads, table,
                                    cont_head, cont_target, self.conf_mult)

    def step(self, batch, with_loss_params: bool):
        x, y = batch[self.image_key], batch[self.label_key]
        if getattr(self, "training_batch_preproc", None) is not None:
            x, y = self.training_batch_preproc(x, y)
        fused = self.heads_route(x.device) == "fused"
        classification, confounder_classification, confounder_regression, features = self.forward(
            x, heads=not fused)
        cat_conf_loss = cont_conf_loss = feature_loss = None
        if fused:
            cat_conf_loss, cont_conf_loss = self.fused_confounder_losses(batch, features)
        else:
            if self.cat_confounder_key is not None:
                cat_conf_loss = self.loss_cat_confounder(confounder_classification,
                                                         batch[self.cat_confounder_key])
            if self.cont_confounder_key is not None:
                cont_conf_loss = self.loss_cont_confounder(confounder_regression,
                                                           batch[self.cont_confounder_key])
        if self.cat_confounder_key or self.cont_confounder_key:
            feature_loss = self.loss_features(features)
        classification_loss = self.calculate_loss(classification.squeeze(1), y,
                                                  with_loss_params=with_loss_params)
        return (classification_loss, cat_conf_loss, cont_conf_loss, feature_loss, classification, y)

    def log_losses(self, losses, prefix: str):
        for loss_val, s in zip(losses, self.loss_str):
            if loss_val is not None:
                self.log(f"{prefix}_{s}", loss_val.detach(), prog_bar=True)

    def _losses(self, batch, with_loss_params, prefix):
        output = self.step(batch, with_loss_params=with_loss_params)
        losses = [loss_val.mean() if loss_val is not None else None for loss_val in output[:4]]
        self.log_losses(losses, prefix)
        return sum(loss_val for loss_val in losses if loss_val is not None), output[4:]

    def training_step(self, batch, batch_idx):
        return self._losses(batch, True, "tr")[0]

    def validation_step(self, batch, batch_idx):
        total, (prediction, y) = self._losses(batch, False, "val")
        self.update_metrics(prediction, y, self.val_metrics, on_epoch=True, prog_bar=True)
        return total

    def test_step(self, batch, batch_idx):
        total, (prediction, y) = self._losses(batch, False, "test")
        self.update_metrics(prediction, y, self.test_metrics, log=False, on_epoch=True, prog_bar=True)
        return total

    def update_metrics(self, prediction, y, metrics, log=True, **kwargs):
        y = y.to(prediction.device).long()
        if self.n_classes == 2:
            prediction = torch.sigmoid(prediction.detach()).squeeze(1)
        else:
            prediction = torch.softmax(prediction.detach(), -1)
        if len(y.shape) > 1:
            y = y.squeeze(1)
        CM.update_many(metrics.values(), prediction, y)
        if log is True:
            for k in metrics:
                self.log(k, metrics[k], **kwargs)

    def confounder_groups(self):
        """pl.py:2531-2547: the parameters whose name contains "confound" at weight decay 0, the
        rest at ``weight_decay``."""
        params_confounder, params_classifier = [], []
        for n, p in self.named_parameters():
            (params_confounder if "confound" in n else params_classifier).append(p)
        return [{"params": params_confounder, "weight_decay": 0},
                {"params": params_classifier, "weight_decay": self.weight_decay}]

    def configure_optimizers(self) -> dict:
        optimizer = FusedAdam(self.confounder_groups(), lr=self.learning_rate, eps=self.optimizer_eps)
        lr_schedulers = CosineAnnealingWithWarmupLR(
            optimizer, T_max=self.n_epochs, start_decay=self.start_decay,
            n_warmup_steps=self.warmup_steps)
        return {"optimizer": optimizer, "lr_scheduler": lr_schedulers, "monitor": "val_loss"}

    def predict_step(self, batch, batch_idx, dataloader_idx=0, *args, **kwargs):
        x = batch[self.image_key]
        prediction = self.forward(x, *args, **kwargs)
        if kwargs.get("return_features", False):
            return {"features": prediction}
        return {"prediction": torch.squeeze(prediction[0], 1)}
