"""Self-supervised training-step wrappers (mirror of
adell_mri/modules/self_supervised/pl.py:170-267 ``SelfSLBasePL`` and :759-985
``SelfSLConvNeXtPL``), VICReg / SimSiam / BYOL on the ConvNeXt backbone.

Kept: constructor arguments, ``step`` arithmetic (which head feeds which loss argument,
stop-gradient, EMA forward and update, loss symmetrisation), ``configure_optimizers``
(AdamW over decay + no-decay parameters in one group, cosine schedule with warm-up).
Lightning is optional as in ``segmentation/pl.py``.

``ssl_method="vicregl"`` (``VICRegLocalLoss`` on the two "representation" feature maps and the
boxes of the batch, csrc/vicregl.hip) is built by ``SelfSLResNetPL`` -- the class the factory
``get_ssl_network`` builds for it -- and by ``SelfSLUNetPL``, whose ``forward(x)`` already is the
feature map. ``SelfSLConvNeXtPL`` still raises ``NotImplementedError`` for it: the reference's
factory never builds the ConvNeXt wrapper with this method, and no fixture pins its feature maps.

``DINOPL`` (pl.py:1168-1282) is the wrapper of the ViT method ``ssl_method="dino"``: both views
stacked through the student in one pass, the EMA teacher under ``no_grad`` on the same stack, the
fused ``DinoLoss`` (csrc/dino.hip) both ways, the EMA update in training only and the centre update
in every step.

``iBOTPL`` (pl.py:1285-1431) is the wrapper of ``ssl_method="ibot"``: the student on both views with
two consecutive masker draws, the EMA teacher under ``no_grad`` without masking, the centre updates
of both losses BEFORE the losses (the lazy ``DinoLoss`` applies them inside the first loss call of
the same step), the global loss across the views on the reduced outputs and the masked-token loss
within each view. The token logits [B, tokens, out_dim] are read in place: per view one fused
function (functional.ibot_view, csrc/ibot.hip) gives the reduced output and the masked-row loss and
writes the whole gradient in one launch; the teacher's logits are read once for its "mean"
reduction and the centre sum.

``IJEPAPL`` (pl.py:987-1165) is the wrapper of ``ssl_method="ijepa"``: one image, no view pair. The
student predicts the features of a few target blocks from the tokens of the context blocks; the EMA
teacher sees the whole image under ``no_grad``. ``step`` takes the smooth-L1 loss of every block
from the teacher's raw output (functional.ijepa_block_loss, csrc/ijepa.hip: layer norm, row gather
and loss in one pass, nothing of the teacher's size written) and never builds the targets;
``calculate_loss(predictions, targets)`` stays, composed, for callers that hold the two lists.

``ViTMaskedAutoEncoderPL`` (pl.py:1434-1611) is the wrapper of ``ssl_method="mae"``: it HOLDS a
``ViTMaskedAutoEncoder`` as ``model`` (no EMA, no ``SelfSLBasePL``). Each step takes the token
predictions (``model.forward_tokens``) and the reconstruction loss through the reference's
view / permute as an index map (functional.mae_reconstruction_loss, csrc/mae.hip): the image-shaped
reconstruction is written only by ``forward``.
"""
import warnings
from typing import Any, Callable

import torch
import torch.distributed as dist

from ... import functional as HF
from ... import ops
from ...optim import FusedAdamW
from ..layers.conv_next import ConvNeXt
from ..layers.res_net import ResNet
from ..segmentation.unet import UNet
from ..learning_rate import CosineAnnealingWithWarmupLR
from .dino import DINO
from .ibot import iBOT
from .autoencoders import ViTMaskedAutoEncoder
from .jepa import IJEPA
from .losses import (DinoLoss, NTXentLoss, VICRegLocalLoss, VICRegLoss, byol_loss,
                     simsiam_loss)

try:  # pragma: no cover - lightning is not installed in the build image
    import lightning.pytorch as pl

    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    _Base = torch.nn.Module

OPTIMIZER_EPS_DEFAULT = 1e-8


class SelfSLBasePL(_Base):
    _supports_vicregl = True   # a wrapper without a pinned feature map for VICRegL turns it off

    def __init__(self):
        super().__init__()
        self.optimizer_eps = OPTIMIZER_EPS_DEFAULT

    if _Base is torch.nn.Module:
        def log(self, *args, **kwargs):
            return None

        def save_hyperparameters(self, *args, **kwargs):
            return None

    def update_metrics(self, y1, y2, metrics, log=True):
        for k in metrics:
            metrics[k].update(y1.flatten(), y2.flatten())

    def init_loss(self):
        """pl.py:202-212: SimSiam by default, BYOL with an EMA target, else by ``ssl_method``."""
        self.loss = simsiam_loss
        if getattr(self, "ema", None) is not None:
            self.loss = byol_loss
        if self.ssl_method == "vicreg":
            self.loss = VICRegLoss(**self.vic_reg_loss_params)
        if self.ssl_method == "vicregl":
            if not self._supports_vicregl:
                raise NotImplementedError(
                    f"ssl_method='vicregl' (VICRegLocalLoss) is not wired for {type(self).__name__}: "
                    "use SelfSLResNetPL (what get_ssl_network builds) or SelfSLUNetPL")
            self.loss = VICRegLocalLoss(**self.vic_reg_loss_params)
        if self.ssl_method == "simclr":
            self.loss = NTXentLoss(temperature=self.temperature)

    def calculate_loss(self, y1, y2, *args):
        if self.stop_gradient is False:
            return self.loss(y1, y2, *args)
        return self.loss(y1, y2.detach(), *args)

    def safe_sum(self, X):
        if isinstance(X, torch.Tensor):
            return X.sum()
        return sum(X)

    def configure_optimizers(self) -> dict:
        if self.n_steps is not None:
            interval, n = "step", self.n_steps
        else:
            interval, n = "epoch", self.n_epochs
        params_no_decay, params_decay = [], []
        for k, p in self.named_parameters():
            (params_no_decay if "normalization" in k else params_decay).append(p)
        optimizer = FusedAdamW(params_decay + params_no_decay, lr=self.learning_rate,
                               weight_decay=self.weight_decay, eps=self.optimizer_eps)
        sched = CosineAnnealingWithWarmupLR(optimizer, T_max=n, start_decay=self.start_decay,
                                            n_warmup_steps=self.warmup_steps, eta_min=0.0)
        return {"optimizer": optimizer,
                "lr_scheduler": {"scheduler": sched, "interval": interval, "frequency": 1},
                "monitor": "val_loss"}

    def setup_metrics(self):
        self.train_metrics = torch.nn.ModuleDict({})
        self.val_metrics = torch.nn.ModuleDict({})
        self.test_metrics = torch.nn.ModuleDict({})


_SSL_HYPERPARAMETERS = (
    "aug_image_key_1", "aug_image_key_2", "box_key_1", "box_key_2", "learning_rate", "batch_size",
    "weight_decay", "training_dataloader_call", "n_epochs", "n_steps", "warmup_steps",
    "start_decay", "ssl_method", "temperature", "vic_reg_loss_params", "stop_gradient",
    "channels_to_batch")


class _TwoViewSSL:
    """What ``SelfSLResNetPL`` (pl.py:312-535) and ``SelfSLConvNeXtPL`` (:759-985) share: two
    augmented views through one network with three heads (``ret`` = representation /
    projection / prediction), an optional EMA or stop-gradient target branch, and a loss that
    returns a list of terms. The backbone class comes first in the MRO of the concrete class."""

    def _init_two_view(self, hp, args, kwargs):
        for k in _SSL_HYPERPARAMETERS:   # plain attributes: set before Module.__init__, as the
            object.__setattr__(self, k, hp[k])   # reference does
        if hp["channels_to_batch"] is True:
            if self._has_heads:
                kwargs["backbone_args"]["in_channels"] = 1
            else:
                kwargs["in_channels"] = 1
        if not self._has_heads:
            kwargs["encoder_only"] = True     # the U-Net encoder alone: forward(x) -> bottleneck
        super().__init__(*args, **kwargs)
        self.optimizer_eps = hp["optimizer_eps"]
        self.ema = hp["ema"]
        if self.ssl_method not in ["vicreg", "vicregl", "simclr"] and self.stop_gradient is False:
            warnings.warn("stop_gradient=False should not (in theory) be used with "
                          "vic_reg=False, vic_reg_local=False or simclr=False")
        self.init_loss()
        if self.ema is not None:
            self.ema.update(self)
        self.loss_str_dict = {"standard": [None], "vicreg": ["inv", "var", "cov"],
                              "vicregl": ["inv", "var", "cov", "local"]}
        self.save_hyperparameters()
        self.setup_metrics()

    _has_heads = True   # forward(x, ret=...) selects representation / projection / prediction

    def _view(self, x, ret):
        return self.forward(x, ret=ret) if self._has_heads else self.forward(x)

    def forward_ema_stop_grad(self, x, ret=None):
        op = self.ema.shadow.forward if self.ema is not None else self.forward
        args = (x, ret) if self._has_heads else (x,)
        if self.stop_gradient is True:
            with torch.no_grad():
                return op(*args)
        return op(*args)

    def _views_share_a_pass(self, ret_1, ret_2):
        """Both views can go through the network as ONE batch of 2B items: same network for both
        (no EMA target, no stop-gradient), heads that nest (projection inside prediction), and no
        layer that couples the items of a batch in training (batch norm). Per item the arithmetic
        is the one of two separate passes; the launches -- this step is bound by the host -- and
        the gradient accumulations of the second pass are halved."""
        if self.ema is not None or self.stop_gradient is True or not self._has_heads:
            return False
        if (ret_1, ret_2) not in (("prediction", "projection"), ("projection", "projection")):
            return False
        if getattr(self, "_batch_coupled", None) is None:
            self._batch_coupled = any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm)
                                      for m in self.modules())
        return not self._batch_coupled

    def _both_views(self, x1, x2, ret_1):
        z = self.forward(torch.cat([x1, x2], 0), ret="projection")
        z1, z2 = z[:x1.shape[0]], z[x1.shape[0]:]
        return (self.prediction_head(z1) if ret_1 == "prediction" else z1), z2

    def _heads_for_method(self, batch):
        """(head of view 1, head of view 2, extra loss arguments), pl.py:457-470."""
        if self.ssl_method == "simclr":
            return "projection", "projection", []
        if self.ssl_method == "vicregl":
            return "representation", "representation", [batch[self.box_key_1],
                                                        batch[self.box_key_2]]
        return "prediction", "projection", []

    def step(self, batch, loss_str: str, metrics: dict, train=False):
        ret_1, ret_2, other_args = self._heads_for_method(batch)
        x1, x2 = batch[self.aug_image_key_1], batch[self.aug_image_key_2]
        if self.channels_to_batch is True:
            x1 = x1.reshape(-1, 1, *x1.shape[2:])
            x2 = x2.reshape(-1, 1, *x2.shape[2:])
        if x1.shape == x2.shape and self._views_share_a_pass(ret_1, ret_2):
            y1, y2 = self._both_views(x1, x2, ret_1)
        else:
            y1 = self._view(x1, ret_1)
            y2 = self.forward_ema_stop_grad(x2, ret=ret_2)
        losses = self.calculate_loss(y1, y2, *other_args)
        self.update_metrics(y1, y2, metrics)
        symmetric_already = self.ssl_method in ("vicreg", "vicregl", "simclr")
        if not symmetric_already:   # SimSiam / BYOL: add the loss with the two views swapped
            y1_ = self.forward_ema_stop_grad(x1, ret=ret_1)
            y2_ = self._view(x2, ret_2)
            losses = losses + self.calculate_loss(y2_, y1_, *other_args)
            self.update_metrics(y2_, y1_, metrics)
        if self.ema is not None and train is True:
            self.ema.update(self)
        loss = self.safe_sum(losses)
        log_kw = dict(batch_size=x1.shape[0], on_epoch=True, on_step=False, prog_bar=True,
                      sync_dist=True)
        self.log(loss_str, loss, **log_kw)
        if self.ssl_method in ("vicregl", "vicreg"):
            for s, loss_value in zip(self.loss_str_dict[self.ssl_method], losses):
                self.log("{}:{}".format(loss_str, s), loss_value, **log_kw)
        self.last_losses = losses
        return loss

    def training_step(self, batch, batch_idx):
        return self.step(batch, "loss", self.train_metrics, train=True)

    def validation_step(self, batch, batch_idx):
        return self.step(batch, "val_loss", self.val_metrics)

    def test_step(self, batch, batch_idx):
        return self.step(batch, "test_loss", self.test_metrics)


class SelfSLConvNeXtPL(_TwoViewSSL, ConvNeXt, SelfSLBasePL):
    """ConvNeXt backbone (pl.py:759-985). ``ssl_method="vicregl"`` raises (module docstring)."""

    _supports_vicregl = False

    def __init__(self, aug_image_key_1: str = "aug_image_1", aug_image_key_2: str = "aug_image_2",
                 box_key_1: str = "box_1", box_key_2: str = "box_2", learning_rate: float = 0.001,
                 batch_size: int = 4, weight_decay: float = 0.005,
                 training_dataloader_call: Callable = None, n_epochs: int = 1000,
                 n_steps: int = None, warmup_steps: int = 0, start_decay: int = None,
                 ema: torch.nn.Module = None, ssl_method: str = "simclr",
                 temperature: float = 1.0, vic_reg_loss_params: dict = {},
                 stop_gradient: bool = True, channels_to_batch: bool = False,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        hp = {k: v for k, v in locals().items() if k not in ("self", "args", "kwargs", "__class__")}
        self._init_two_view(hp, args, kwargs)


class SelfSLResNetPL(_TwoViewSSL, ResNet, SelfSLBasePL):
    """ResNet backbone (pl.py:312-535): what ``get_ssl_network`` builds for simclr / byol /
    vicreg / vicregl, transferable to a U-Net encoder (utils/handoff.py)."""

    def __init__(self, aug_image_key_1: str = "aug_image_1", aug_image_key_2: str = "aug_image_2",
                 box_key_1: str = "box_1", box_key_2: str = "box_2", learning_rate: float = 0.001,
                 batch_size: int = 4, weight_decay: float = 0.005,
                 training_dataloader_call: Callable = None, n_epochs: int = 1000,
                 n_steps: int = None, warmup_steps: int = 0, start_decay: int = None,
                 ema: torch.nn.Module = None, ssl_method: str = "simclr",
                 temperature: float = 1.0, vic_reg_loss_params: dict = {},
                 stop_gradient: bool = True, channels_to_batch: bool = False,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        hp = {k: v for k, v in locals().items() if k not in ("self", "args", "kwargs", "__class__")}
        self._init_two_view(hp, args, kwargs)


class SelfSLUNetPL(_TwoViewSSL, UNet, SelfSLBasePL):
    """U-Net encoder as the self-supervised backbone (pl.py:538-756): ``UNet(encoder_only=True)``
    returns the bottleneck feature map, the VICReg loss takes its spatial means
    (``VICRegLoss.flatten_if_necessary``); the trained encoder transfers to a segmentation U-Net
    by ``state_dict`` (same ``encoding_operations.*`` keys)."""

    _has_heads = False

    def __init__(self, aug_image_key_1: str = "aug_image_1", aug_image_key_2: str = "aug_image_2",
                 box_key_1: str = "box_1", box_key_2: str = "box_2", learning_rate: float = 0.001,
                 batch_size: int = 4, weight_decay: float = 0.005,
                 training_dataloader_call: Callable = None, n_epochs: int = 1000,
                 n_steps: int = None, warmup_steps: int = 0, start_decay: int = None,
                 ema: torch.nn.Module = None, ssl_method: str = "simclr",
                 temperature: float = 1.0, vic_reg_loss_params: dict = {},
                 stop_gradient: bool = True, channels_to_batch: bool = False,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        hp = {k: v for k, v in locals().items() if k not in ("self", "args", "kwargs", "__class__")}
        self._init_two_view(hp, args, kwargs)


class DINOPL(DINO, SelfSLBasePL):
    """DINO on a ViT encoder (pl.py:1168-1282). ``ema`` is the teacher and is required. The centres
    of the loss stay out of the EMA (``exclude_keys=["centers"]``); they are updated from the
    teacher's outputs in every step, training or not, and applied lazily by the next loss call."""

    def __init__(self, aug_image_key_1: str = "aug_image_1", aug_image_key_2: str = "aug_image_2",
                 learning_rate: float = 1e-3, batch_size: int = 1, weight_decay: float = 1e-6,
                 training_dataloader_call: Callable = None, n_epochs: int = 100,
                 n_steps: int = None, warmup_steps: int = 0, start_decay: int = 0,
                 temperature: float = 0.1, stop_gradient: bool = True,
                 channels_to_batch: bool = False, optimizer_eps: float = OPTIMIZER_EPS_DEFAULT,
                 ema: torch.nn.Module = None, centers_m: float = 0.9,
                 teacher_score_method: str = "center", *args, **kwargs):
        hp = dict(aug_image_key_1=aug_image_key_1, aug_image_key_2=aug_image_key_2,
                  learning_rate=learning_rate, batch_size=batch_size, weight_decay=weight_decay,
                  training_dataloader_call=training_dataloader_call, n_epochs=n_epochs,
                  n_steps=n_steps, warmup_steps=warmup_steps, start_decay=start_decay,
                  temperature=temperature, stop_gradient=stop_gradient,
                  channels_to_batch=channels_to_batch, centers_m=centers_m,
                  teacher_score_method=teacher_score_method, ssl_method="dino")
        for k, v in hp.items():   # plain attributes: set before Module.__init__, as the reference does
            object.__setattr__(self, k, v)
        if channels_to_batch is True:
            kwargs["backbone_args"]["in_channels"] = 1
        super().__init__(*args, **kwargs)   # DINO.__init__: raises for a configuration that cannot run
        self.optimizer_eps = optimizer_eps
        self.ema = ema
        if self.ema is None:
            raise ValueError("DINO requires an EMA (teacher) copy of the network "
                             "(`ema` must be an ExponentialMovingAverage module).")
        self.save_hyperparameters()
        self.setup_metrics()
        self.init_loss()
        self.ema.update(self, exclude_keys=["centers"])

    def init_loss(self):
        self.loss = DinoLoss(temperatures=(self.temperature, self.temperature),
                             n_features=self.out_dim, center_m=self.centers_m,
                             teacher_score_method=self.teacher_score_method)

    def calculate_loss(self, y_1, y_2, *args):
        return self.loss(y_1, y_2)

    def step(self, batch, loss_str: str, metrics: dict | None = None, train=False):
        x1, x2 = batch[self.aug_image_key_1], batch[self.aug_image_key_2]
        if self.channels_to_batch is True:
            x1 = x1.reshape(-1, 1, *x1.shape[2:])
            x2 = x2.reshape(-1, 1, *x2.shape[2:])
        stacked_x = torch.cat([x1, x2])
        sh = [x1.shape[0], x2.shape[0]]
        s_1, s_2 = self.forward(stacked_x).split(sh, dim=0)
        with torch.no_grad():
            t_all = self.ema(stacked_x).detach()
        t_1, t_2 = t_all.split(sh, dim=0)
        loss_value = torch.add(self.calculate_loss(s_1, t_2) / 2.0,
                               self.calculate_loss(s_2, t_1) / 2.0)
        if metrics is not None:
            self.update_metrics(torch.cat([s_1, s_2]), t_all, metrics, log=True)
        self.log(loss_str, loss_value, on_step=True, on_epoch=True, prog_bar=True)
        if self.ema is not None and train is True:
            self.ema.update(self, exclude_keys=["centers"])
        self.loss.update_centers(t_all)     # cat([t_1, t_2]) is the teacher's stacked output
        return loss_value

    def training_step(self, batch, batch_idx):
        return self.step(batch, "loss", train=True)

    def validation_step(self, batch, batch_idx):
        return self.step(batch, "val_loss")

    def test_step(self, batch, batch_idx):
        return self.step(batch, "test_loss")


class iBOTPL(iBOT, SelfSLBasePL):
    """iBOT on a ViT encoder (pl.py:1285-1431). ``ema`` is the teacher and is required. Two
    ``DinoLoss`` modules: ``loss_global`` on the reduced outputs, across the views, and ``loss_mask``
    on the masked patch tokens, within a view. Their centres stay out of the EMA and are updated
    from the teacher's outputs -- all of its patch tokens for ``loss_mask``, not only the masked ones
    -- before the losses of the same step, training or not.

    Kept as written: ``calculate_loss_mask(a, b, m)`` indexes the PATCH tokens with the masker's
    coordinates, which still carry the ``+ skip_n`` offset (ibot.py docstring); an index that
    reaches the number of patch tokens raises ``IndexError``, here on the host before any kernel."""

    def __init__(self, aug_image_key_1: str = "aug_image_1", aug_image_key_2: str = "aug_image_2",
                 learning_rate: float = 1e-3, batch_size: int = 1, weight_decay: float = 1e-6,
                 training_dataloader_call: Callable = None, n_epochs: int = 100,
                 n_steps: int = None, warmup_steps: int = 0, start_decay: int = 0,
                 temperature: float = 0.1, stop_gradient: bool = True,
                 channels_to_batch: bool = False, optimizer_eps: float = OPTIMIZER_EPS_DEFAULT,
                 ema: torch.nn.Module = None, centers_m: float = 0.9,
                 teacher_score_method: str = "center", *args, **kwargs):
        hp = dict(aug_image_key_1=aug_image_key_1, aug_image_key_2=aug_image_key_2,
                  learning_rate=learning_rate, batch_size=batch_size, weight_decay=weight_decay,
                  training_dataloader_call=training_dataloader_call, n_epochs=n_epochs,
                  n_steps=n_steps, warmup_steps=warmup_steps, start_decay=start_decay,
                  temperature=temperature, stop_gradient=stop_gradient,
                  channels_to_batch=channels_to_batch, centers_m=centers_m,
                  teacher_score_method=teacher_score_method, ssl_method="ibot")
        for k, v in hp.items():   # plain attributes: set before Module.__init__, as the reference does
            object.__setattr__(self, k, v)
        if channels_to_batch is True:
            kwargs["backbone_args"]["in_channels"] = 1
        super().__init__(*args, **kwargs)   # iBOT.__init__: raises for a configuration that cannot run
        self.optimizer_eps = optimizer_eps
        self.ema = ema
        if self.ema is None:
            raise ValueError("iBOT requires an EMA (teacher) copy of the network "
                             "(`ema` must be an ExponentialMovingAverage module).")
        self.save_hyperparameters()
        self.setup_metrics()
        self.init_loss()
        self.ema.update(self, exclude_keys=["centers"])

    def init_loss(self):
        conf = dict(temperatures=(self.temperature, self.temperature), n_features=self.out_dim,
                    center_m=self.centers_m, teacher_score_method=self.teacher_score_method)
        self.loss_mask = DinoLoss(**conf)
        self.loss_global = DinoLoss(**conf)

    def calculate_loss_global(self, y_red_1: torch.Tensor, y_red_2: torch.Tensor):
        return self.loss_global(a=y_red_1, b=y_red_2.detach())

    def calculate_loss_mask(self, a: torch.Tensor, b: torch.Tensor, m):
        """``loss_mask(a[:, m], b[:, m])`` on the patch tokens a, b [B, T, K] -- the composed path:
        the rows are gathered, then the dense loss. ``step`` computes the same value without the
        gather (functional.ibot_view)."""
        table = HF.patch_rows(m, a.shape[1], 0, a.device)     # IndexError on the host
        return self.loss_mask(a.index_select(1, table.dev), b.detach().index_select(1, table.dev))

    @torch.no_grad()
    def _teacher_view(self, x, sums):
        """(reduced [B, K], token logits [B, c + T, K]) of the teacher; the fp64 sums of its patch
        rows go to ``sums`` [B, K]: one read of the logits for the "mean" reduction and the centre
        sum."""
        shadow = self.ema.shadow
        y = shadow.token_logits(x).detach()
        c = shadow.class_token
        mean, _ = ops.ibot_token_sums(y, c, 1.0 / (y.shape[1] - c), raw_out=sums)
        return (y[:, 0] if shadow.reduce_fn == "cls" else mean), y

    @torch.no_grad()
    def _pending_mask_centers(self, sums, rows):
        """``loss_mask.update_centers(cat[t_1, t_2])`` from the per-item sums of the patch rows,
        [2B, K] in fp64: the column sum over the ``rows`` teacher rows, pending as update_centers
        leaves it."""
        crit = self.loss_mask
        crit.updated = False
        crit.len_teacher_output = rows
        crit.async_batch_center = ops.ibot_center_sum(sums)
        if dist.is_initialized():
            crit.reduce_handle = dist.all_reduce(crit.async_batch_center, async_op=True)

    def _mask_view(self, s, y, m):
        """(s_red, loss_mask) of one view from the token logits of student and teacher."""
        crit, c = self.loss_mask, self.class_token
        if crit.teacher_score_method == "center":
            crit.apply_center_update()
            return HF.ibot_view(s, y, m, crit.centers, crit.t1, crit.t2, c, self.reduce_fn)
        table = HF.patch_rows(m, s.shape[1], c, s.device)
        scores = crit.sinkhorn_knopp_teacher(y.index_select(1, table.dev))
        return HF.ibot_view(s, y, table, scores, crit.t1, crit.t2, c, self.reduce_fn,
                            teacher_is_scores=True)

    def step(self, batch, loss_str: str, metrics: dict | None = None, train=False):
        x1, x2 = batch[self.aug_image_key_1], batch[self.aug_image_key_2]
        if self.channels_to_batch is True:
            x1 = x1.reshape(-1, 1, *x1.shape[2:])
            x2 = x2.reshape(-1, 1, *x2.shape[2:])
        s_1, mc_1 = self.token_logits(x1, mask=True)
        s_2, mc_2 = self.token_logits(x2, mask=True)
        sums = torch.empty((x1.shape[0] + x2.shape[0], self.out_dim), device=x1.device,
                           dtype=torch.float64)
        t_red_1, t_1 = self._teacher_view(x1, sums[:x1.shape[0]])
        t_red_2, t_2 = self._teacher_view(x2, sums[x1.shape[0]:])
        c = self.class_token
        # centre updates first: applied by the first loss call below
        self.loss_global.update_centers(torch.cat([t_red_1, t_red_2]))
        self._pending_mask_centers(
            sums, t_1.shape[0] * (t_1.shape[1] - c) + t_2.shape[0] * (t_2.shape[1] - c))
        s_red_1, mask_1 = self._mask_view(s_1, t_1, mc_1)
        s_red_2, mask_2 = self._mask_view(s_2, t_2, mc_2)
        loss_global = torch.add(self.calculate_loss_global(s_red_1, t_red_2) / 2.0,
                                self.calculate_loss_global(s_red_2, t_red_1) / 2.0)
        loss_mask = torch.add(mask_1 / 2.0, mask_2 / 2.0)
        if metrics is not None:
            self.update_metrics(torch.cat([s_red_1, s_red_2]), torch.cat([t_red_1, t_red_2]),
                                metrics, log=True)
        self.log(loss_str + "_global", loss_global, on_step=True, on_epoch=True, prog_bar=True)
        self.log(loss_str + "_mask", loss_mask, on_step=True, on_epoch=True, prog_bar=True)
        if self.ema is not None and train is True:
            self.ema.update(self, exclude_keys=["centers"])
        self.last_losses = (loss_mask, loss_global)
        return loss_mask + loss_global

    def training_step(self, batch, batch_idx):
        return self.step(batch, "loss", train=True)

    def validation_step(self, batch, batch_idx):
        return self.step(batch, "val_loss")

    def test_step(self, batch, batch_idx):
        return self.step(batch, "test_loss")


class IJEPAPL(IJEPA, SelfSLBasePL):
    """I-JEPA on a ViT encoder (pl.py:987-1165). ``ema`` is the teacher and is required. The
    reference's order in ``__init__``: ``init_loss``, ``ema.update(self)`` (which makes the teacher
    from the initial weights), ``save_hyperparameters``, ``setup_metrics``. Every ``step`` draws new
    context and target blocks, validation included; the EMA moves in training only."""

    def __init__(self, image_key: str = "image", learning_rate: float = 0.001, batch_size: int = 4,
                 weight_decay: float = 0.005, training_dataloader_call: Callable = None,
                 n_epochs: int = 1000, n_steps: int = None, warmup_steps: int = 0,
                 start_decay: int = None, ema: torch.nn.Module = None, ssl_method: str = "simclr",
                 temperature: float = 1.0, vic_reg_loss_params: dict = {},
                 stop_gradient: bool = True, channels_to_batch: bool = False,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT, *args, **kwargs):
        hp = dict(image_key=image_key, learning_rate=learning_rate, batch_size=batch_size,
                  weight_decay=weight_decay, training_dataloader_call=training_dataloader_call,
                  n_epochs=n_epochs, n_steps=n_steps, warmup_steps=warmup_steps,
                  start_decay=start_decay, temperature=temperature,
                  vic_reg_loss_params=vic_reg_loss_params, stop_gradient=stop_gradient,
                  channels_to_batch=channels_to_batch, ssl_method="ijepa")
        for k, v in hp.items():   # plain attributes: set before Module.__init__, as the reference does
            object.__setattr__(self, k, v)
        if channels_to_batch is True:
            kwargs["backbone_args"]["in_channels"] = 1
        super().__init__(*args, **kwargs)
        self.optimizer_eps = optimizer_eps
        self.ema = ema
        if self.ema is None:
            raise ValueError("I-JEPA requires an EMA (teacher) copy of the network "
                             "(`ema` must be an ExponentialMovingAverage module).")
        self.init_loss()
        self.ema.update(self)
        self.save_hyperparameters()
        self.setup_metrics()

    def init_loss(self):
        self.loss = torch.nn.SmoothL1Loss()

    def calculate_loss(self, predictions, targets, *args):
        """The mean over the blocks of ``SmoothL1Loss()(p, t)`` on lists of predictions and
        (normalised, gathered) targets: the composed path. ``step`` computes the same value from
        the teacher's raw output without building the targets."""
        return torch.stack([self.loss(p, t) for p, t in zip(predictions, targets)]).mean()

    def step(self, batch, loss_str: str, train=False):
        x = batch[self.image_key]
        if self.channels_to_batch is True:
            x = x.reshape(-1, 1, *x.shape[2:])
        predictions, h, rows = self.forward_blocks(x, self.ema)
        loss = torch.stack([HF.ijepa_block_loss(p, h, r)
                            for p, r in zip(predictions, rows)]).mean()
        if train is True:
            self.ema.update(self)
        self.log(loss_str, loss, batch_size=x.shape[0], on_epoch=True, on_step=False,
                 prog_bar=True, sync_dist=True)
        return loss

    def training_step(self, batch, batch_idx):
        return self.step(batch, "loss", train=True)

    def validation_step(self, batch, batch_idx):
        return self.step(batch, "val_loss")

    def test_step(self, batch, batch_idx):
        return self.step(batch, "test_loss")

    def configure_optimizers(self) -> dict:
        """pl.py:1129-1165: AdamW over decay + "normalization" parameters in one group (the
        latter last), cosine schedule with warm-up down to 1e-6."""
        conf = super().configure_optimizers()
        conf["lr_scheduler"]["scheduler"] = CosineAnnealingWithWarmupLR(
            conf["optimizer"], T_max=self.n_steps if self.n_steps is not None else self.n_epochs,
            start_decay=self.start_decay, n_warmup_steps=self.warmup_steps, eta_min=1e-6)
        return conf


class ViTMaskedAutoEncoderPL(_Base):
    """Masked-autoencoder pretraining of a ViT (pl.py:1434-1611): ``MSELoss()`` between the
    reconstruction and the WHOLE image, masked and visible patches alike. Every step draws a new
    shuffle from the model's one rng, validation and test included. AdamW with betas (0.9, 0.95);
    with ``warmup_steps > 0`` the optimiser starts at lr 0.0 under a cosine schedule with warm-up
    whose base lr is ``learning_rate``, otherwise ``configure_optimizers`` returns the bare
    optimiser."""

    if _Base is torch.nn.Module:
        def log(self, *args, **kwargs):
            return None

        def save_hyperparameters(self, *args, **kwargs):
            return None

    def __init__(self, image_key: str, image_size, patch_size, in_channels: int,
                 input_dim_size: int, encoder_args: dict[str, Any], decoder_args: dict[str, Any],
                 n_epochs: int = 100, n_steps: int | None = None, embed_method: str = "linear",
                 dropout_rate: float = 0.0, mask_fraction: float = 0.75,
                 learning_rate: float = 1e-3, batch_size: int = 4, weight_decay: float = 1e-6,
                 warmup_steps: int = 0, start_decay: int = 0,
                 training_dataloader_call: Callable | None = None,
                 optimizer_eps: float = OPTIMIZER_EPS_DEFAULT):
        super().__init__()
        self.save_hyperparameters()
        self.model = ViTMaskedAutoEncoder(
            image_size=image_size, patch_size=patch_size, in_channels=in_channels,
            input_dim_size=input_dim_size, encoder_args=encoder_args, decoder_args=decoder_args,
            embed_method=embed_method, dropout_rate=dropout_rate, mask_fraction=mask_fraction)
        self.criterion = torch.nn.MSELoss()     # what the steps compute; they use the fused form
        self.image_key = image_key
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.weight_decay = weight_decay
        self.warmup_steps = warmup_steps
        self.training_dataloader_call = training_dataloader_call
        self.n_steps = n_steps
        self.n_epochs = n_epochs
        self.start_decay = start_decay
        self.optimizer_eps = optimizer_eps

    def forward(self, x: torch.Tensor):
        return self.model(x)

    def step(self, batch, loss_str: str, **log_kwargs):
        x = batch[self.image_key]
        pred, _ = self.model.forward_tokens(x)
        loss = HF.mae_reconstruction_loss(pred, x, self.model.patch_elems)
        self.log(loss_str, loss, on_epoch=True, prog_bar=True, **log_kwargs)
        return loss

    def training_step(self, batch, batch_idx):
        return self.step(batch, "train_loss", on_step=True)

    def validation_step(self, batch, batch_idx):
        return self.step(batch, "val_loss", on_step=False)

    def test_step(self, batch, batch_idx):
        return self.step(batch, "test_loss", on_step=False)

    def configure_optimizers(self):
        if self.n_steps:
            n, interval = self.n_steps, "step"
        else:
            n, interval = self.n_epochs, "epoch"
        initial_lr = 0.0 if self.warmup_steps > 0 else self.learning_rate
        # parameters(): the positional embedding, held under two names, enters the flat buffer once
        optimizer = FusedAdamW(self.parameters(), lr=initial_lr, weight_decay=self.weight_decay,
                               betas=(0.9, 0.95), eps=self.optimizer_eps)
        if self.warmup_steps > 0:
            scheduler = {"scheduler": CosineAnnealingWithWarmupLR(
                optimizer, T_max=n, start_decay=self.start_decay,
                n_warmup_steps=self.warmup_steps, eta_min=1e-6),
                "interval": interval, "frequency": 1}
            scheduler["scheduler"].base_lrs = [self.learning_rate]
            return {"optimizer": optimizer, "lr_scheduler": scheduler}
        return optimizer

    def train_dataloader(self):
        if self.training_dataloader_call is None:
            raise ValueError("training_dataloader_call must be provided for training")
        return self.training_dataloader_call(self.batch_size)
