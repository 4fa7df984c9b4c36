"""``DDPMUNetPL``: the training wrapper of ``DiffusionUNet`` with a ``Diffusion`` process.

This is the package's own wrapper. The reference's ``DiffusionUNetPL`` (adell_mri/modules/diffusion/
pl.py) subclasses a MONAI-generative network with other ``state_dict`` keys and is deliberately not
mirrored; the name differs so that nobody loads the wrong checkpoint. What is taken from it is its
``step`` -- with ``Diffusion`` in place of the MONAI inferer -- its three step methods and its
``configure_optimizers``:

* ``epsilon`` comes from a CPU ``torch.Generator`` seeded ``seed + rank`` and is drawn before the
  timesteps, ``randint(0, noise_steps)`` from the same generator; ``device_noise=True`` draws both on
  the device instead (no host-to-device copy of the noise; another random stream);
* with a ``cls_key``, one ``rng.random() < uncondition_proba`` draw per batch drops ``cls``;
* the loss is ``functional.mse_loss(prediction, epsilon)``;
* ``FusedAdamW`` for ``torch.optim.AdamW`` and the package's cosine schedule with warm-up.

``trainer.StepRunner``, ``fit_steps`` and ``validate_steps`` take it unchanged."""
from typing import Callable

import numpy as np
import torch

from ... import functional as HF
from ...optim import FusedAdamW
from ..learning_rate import CosineAnnealingWithWarmupLR
from .diffusion_process import Diffusion
from .unet import DiffusionUNet

try:  # pragma: no cover - lightning is not installed in the build image
    import lightning.pytorch as pl

    _Base = pl.LightningModule
except Exception:  # noqa: BLE001
    _Base = torch.nn.Module

OPTIMIZER_EPS_DEFAULT = 1e-8


def _global_rank() -> int:
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        return torch.distributed.get_rank()
    return 0


class DDPMUNetPL(DiffusionUNet, _Base):
    if _Base is torch.nn.Module:
        def log(self, *args, **kwargs):
            return None

    def __init__(self, diffusion: Diffusion, image_key: str = "image", cls_key: str = None,
                 uncondition_proba: float = 0.0, n_epochs: int = 100, warmup_steps: int = 0,
                 start_decay: int = 0, training_dataloader_call: Callable = None,
                 batch_size: int = 16, learning_rate: float = 0.001, weight_decay: float = 0.0,
                 seed: int = 42, optimizer_eps: float = OPTIMIZER_EPS_DEFAULT,
                 device_noise: bool = False, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not isinstance(diffusion, Diffusion):
            raise TypeError(f"DDPMUNetPL: diffusion must be a Diffusion, got {type(diffusion).__name__}")

        self.diffusion = diffusion
        self.image_key = image_key
        self.cls_key = cls_key
        self.uncondition_proba = uncondition_proba
        self.n_epochs = n_epochs
        self.warmup_steps = warmup_steps
        self.start_decay = start_decay
        self.training_dataloader_call = training_dataloader_call
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.weight_decay = weight_decay
        self.seed = seed
        self.optimizer_eps = optimizer_eps
        self.device_noise = device_noise

        self.g = torch.Generator()
        self.g.manual_seed(self.seed + _global_rank())
        self._device_g = None
        self.rng = np.random.default_rng(self.seed + _global_rank())
        self.noise_steps = self.diffusion.noise_steps

    def calculate_loss(self, prediction: torch.Tensor, epsilon: torch.Tensor) -> torch.Tensor:
        return HF.mse_loss(prediction, epsilon)

    def _generator_on(self, device):
        if self._device_g is None or self._device_g.device != device:
            self._device_g = torch.Generator(device=device)
            self._device_g.manual_seed(self.seed + _global_rank())
        return self._device_g

    def randn_like(self, x: torch.Tensor) -> torch.Tensor:
        if self.device_noise is True:
            return torch.randn(x.shape, generator=self._generator_on(x.device), dtype=x.dtype,
                               device=x.device)
        return torch.randn(size=x.shape, generator=self.g, dtype=x.dtype,
                           layout=x.layout).contiguous().to(x.device)

    def timesteps_like(self, x: torch.Tensor) -> torch.Tensor:
        if self.device_noise is True:
            return torch.randint(0, self.noise_steps, (x.shape[0],),
                                 generator=self._generator_on(x.device), device=x.device).long()
        return torch.randint(0, self.noise_steps, (x.shape[0],), generator=self.g).to(x.device).long()

    def step(self, x: torch.Tensor, timesteps: torch.Tensor = None, cls: torch.Tensor = None,
             epsilon: torch.Tensor = None) -> torch.Tensor:
        """The noise-prediction loss of one batch. ``epsilon`` and ``timesteps`` are drawn (in this
        order) unless given."""
        if epsilon is None:
            epsilon = self.randn_like(x)
        if timesteps is None:
            timesteps = self.timesteps_like(x)
        else:
            timesteps = timesteps.long()
        prediction = self.diffusion(x, self, epsilon, timesteps, cls)
        if isinstance(prediction, tuple):       # deep supervision: the head alone is trained here
            prediction = prediction[0]
        return self.calculate_loss(prediction, epsilon)

    def unpack_batch(self, batch: dict):
        x = batch[self.image_key]
        cls = None
        if self.cls_key is not None:
            cls = batch[self.cls_key]
            if self.rng.random() < self.uncondition_proba:
                cls = None
        return x, cls

    def training_step(self, batch: dict, batch_idx: int) -> torch.Tensor:
        x, cls = self.unpack_batch(batch)
        loss = self.step(x, cls=cls)
        self.log("loss", loss, on_step=True, prog_bar=True)
        return loss

    def validation_step(self, batch: dict, batch_idx: int) -> torch.Tensor:
        x, cls = self.unpack_batch(batch)
        loss = self.step(x, cls=cls)
        self.log("val_loss", loss, on_epoch=True, prog_bar=True)
        return loss

    def test_step(self, batch: dict, batch_idx: int) -> torch.Tensor:
        x, cls = self.unpack_batch(batch)
        loss = self.step(x, cls=cls)
        self.log("test_loss", loss)
        return loss

    def train_dataloader(self):
        return self.training_dataloader_call(self.batch_size)

    def configure_optimizers(self) -> dict:
        optimizer = FusedAdamW(self.parameters(), lr=self.learning_rate,
                               weight_decay=self.weight_decay, eps=self.optimizer_eps)
        lr_schedulers = CosineAnnealingWithWarmupLR(optimizer, T_max=self.n_epochs,
                                                    start_decay=self.start_decay,
                                                    n_warmup_steps=self.warmup_steps, eta_min=0.0)
        return {"optimizer": optimizer, "lr_scheduler": lr_schedulers, "monitor": "val_loss"}
