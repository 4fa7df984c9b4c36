"""The five beta schedules and ``Diffusion`` (mirror of
adell_mri/modules/diffusion/diffusion_process.py): noising, the DDPM / DDIM / alpha-deblending reverse
steps and ``sample`` with classifier-free guidance.

Mirrored as written: the constructor arguments and ``check_arguments``; the schedules and
``alpha_bar`` (host torch code, bit for bit); ``get_shape``; ``__call__`` hands the model
``t / noise_steps``, a fraction; ``sample_timesteps``; ``sample`` runs ``t = final_t - 1 ... 1`` and
never takes the ``t = 0`` step, sets ``eval()`` then ``train()``, and with a classification and a
positive scale calls the model a second time without ``cls``.

On the device: ``noise_images`` is one launch (``functional.diffusion_noise``; the timesteps are read
by the kernel), every reverse step is one launch (``functional.diffusion_reverse_step``) in place of
the reference's chain of elementwise ops, with the guidance blend folded into it.

Deviations, all deliberate:

* ``beta``, ``alpha`` and ``alpha_bar`` stay host tensors (the reference moves them to the device in
  ``sample`` / ``noise_images``); a device copy of ``alpha_bar`` is kept beside them for the noising
  kernel, and the step coefficients are computed on the host in fp64 from the host tables.
* the step methods take the Python int of ``t`` (a one-element tensor is converted, which is a host
  read): the reference compares a device tensor with 0, a host read per step. ``sample`` passes its
  loop index.
* the step methods take ``epsilon_uncond`` and ``scale``: the guidance blend
  ``epsilon_uncond + scale * (epsilon - epsilon_uncond)`` happens inside the step's launch.
* ``Diffusion.randn_like(x)`` (default ``torch.randn_like``) is the single place the steps' noise is
  drawn, so a test can replay recorded noise. As in the reference the DDIM step draws at every call,
  DDPM only when ``t > 0`` and ``eta > 0``, alpha-deblending never.
"""
from math import sqrt
from typing import List, Tuple, Union

import torch

from ... import functional as HF


def cosine_beta_schedule(timesteps: int, beta_start: float = 0.0001, beta_end: float = 0.02,
                         s: float = 0.008):
    steps = timesteps + 1
    x = torch.linspace(0, timesteps, steps)
    alphas_cumprod = (torch.cos(((x / timesteps) + s) / (1 + s) * torch.pi * 0.5) ** 2)
    alphas_cumprod = alphas_cumprod / alphas_cumprod[0]
    betas = 1 - (alphas_cumprod[1:] / alphas_cumprod[:-1])
    return torch.clip(betas, 0.0001, 0.9999)


def linear_beta_schedule(timesteps: int, beta_start: float = 0.0001, beta_end: float = 0.02,
                         s: float = None):
    return torch.linspace(beta_start, beta_end, timesteps)


def scaled_linear_beta_schedule(timesteps: int, beta_start: float = 0.0001, beta_end: float = 0.02,
                                s: float = None):
    return torch.square(torch.linspace(sqrt(beta_start), sqrt(beta_end), timesteps))


def quadratic_beta_schedule(timesteps: int, beta_start: float = 0.0001, beta_end: float = 0.02,
                            s: float = None):
    return torch.linspace(beta_start**0.5, beta_end**0.5, timesteps) ** 2


def sigmoid_beta_schedule(timesteps: int, beta_start: float = 0.0001, beta_end: float = 0.02,
                          s: float = None):
    betas = torch.linspace(-3, 3, timesteps)
    return torch.sigmoid(betas) * (beta_end - beta_start) + beta_start


def _in_layout_of(t, like):
    """``t`` in the dense layout of ``like`` (row-major or channels-last): itself when it already is,
    else a copy."""
    if like.dim() in (4, 5):
        fmt = torch.channels_last_3d if like.dim() == 5 else torch.channels_last
        if like.is_contiguous(memory_format=fmt) and not like.is_contiguous():
            return t.contiguous(memory_format=fmt)
    return t if (t.is_contiguous() and like.is_contiguous()) else t.contiguous()


class Diffusion:
    """Diffusion process for diffusion models: ``noise_images`` diffuses an image to timestep t,
    ``sample`` reverts the process from noise with a model that predicts the noise."""

    def __init__(self, noise_steps: int = 1000, beta_start: float = 1e-4, beta_end: float = 0.02,
                 img_size: Union[Tuple[int, int], Tuple[int, int, int]] = (256, 256),
                 scheduler: str = "cosine", step_key: str = "ddpm", device: str = "cuda",
                 track_progress: bool = False, clip_sample: bool = True):
        self.noise_steps = noise_steps
        self.beta_start = beta_start
        self.beta_end = beta_end
        self.img_size = img_size
        self.scheduler = scheduler
        self.step_key = step_key
        self.track_progress = track_progress
        self.clip_sample = clip_sample

        self.n_dim = len(img_size)

        self.beta = self.get_noise_schedule()
        self.alpha = 1 - self.beta
        self.alpha_bar = torch.cumprod(self.alpha, 0)
        self.check_arguments()
        self._host_tables = None
        self._alpha_bar_device = None

    def get_noise_schedule(self):
        return self.schedulers[self.scheduler](self.noise_steps, self.beta_start, self.beta_end)

    @property
    def schedulers(self):
        return {
            "linear": linear_beta_schedule,
            "scaled_linear": scaled_linear_beta_schedule,
            "quadratic": quadratic_beta_schedule,
            "sigmoid": sigmoid_beta_schedule,
            "cosine": cosine_beta_schedule,
        }

    def check_arguments(self):
        if isinstance(self.noise_steps, int) is False:
            raise TypeError("noise_steps must be int")
        if isinstance(self.beta_start, float) is False:
            raise TypeError("beta_start must be float")
        if isinstance(self.beta_end, float) is False:
            raise TypeError("beta_end must be float")
        if isinstance(self.img_size, (tuple, list)) is False:
            raise TypeError("img_size must be tuple")
        else:
            if len(self.img_size) not in [2, 3]:
                raise TypeError("img_size must be tuple with size 2 or 3")
            if any([isinstance(x, int) is False for x in self.img_size]) is True:
                raise TypeError("img_size must be tuple of int")

    def get_shape(self, x: torch.Tensor = None) -> List[int]:
        if x is None:
            n_dim = self.n_dim + 2
        else:
            n_dim = len(x.shape)
        new_shape = (-1, *[1 for _ in range(1, n_dim)])
        return new_shape

    # ---- the tables the kernels and the host arithmetic read -----------------------------------
    @property
    def tables(self):
        """Host copies of ``beta``, ``alpha`` and ``alpha_bar`` as fp64 lists: what
        ``functional.diffusion_reverse_step`` computes its coefficients from."""
        if self._host_tables is None:
            self._host_tables = {k: getattr(self, k).detach().cpu().double().tolist()
                                 for k in ("beta", "alpha", "alpha_bar")}
        return self._host_tables

    def alpha_bar_on(self, device):
        """``alpha_bar`` as a dense fp32 tensor on ``device`` (copied there once)."""
        device = torch.device(device)
        if self._alpha_bar_device is None or self._alpha_bar_device.device != device:
            self._alpha_bar_device = self.alpha_bar.detach().to(torch.float32).contiguous().to(device)
        return self._alpha_bar_device

    def randn_like(self, x: torch.Tensor) -> torch.Tensor:
        """The single place the reverse steps draw their noise."""
        return torch.randn_like(x)

    # ---- forward process ---------------------------------------------------------------------------
    def noise_images(self, x: torch.Tensor, epsilon: torch.Tensor, t: torch.Tensor):
        """``sqrt(alpha_bar[t]) * x + sqrt(1 - alpha_bar[t]) * epsilon`` per item, and ``epsilon``."""
        t = t.to(x.device).long().reshape(-1).contiguous()
        epsilon = _in_layout_of(epsilon, x)
        return HF.diffusion_noise(x, epsilon, self.alpha_bar_on(x.device), t), epsilon

    def __call__(self, x: torch.Tensor, model: torch.nn.Module, epsilon: torch.Tensor,
                 t: torch.Tensor, classification: torch.Tensor = None):
        noised_image, epsilon = self.noise_images(x, epsilon=epsilon, t=t)
        prediction = model(noised_image, t / self.noise_steps, classification)
        return prediction

    def sample_timesteps(self, n: int) -> torch.Tensor:
        return torch.randint(1, self.noise_steps, (n,))

    # ---- reverse process -----------------------------------------------------------------------------
    def _reverse(self, kind, x, epsilon, t, eta, noise, epsilon_uncond, scale):
        x = _in_layout_of(x, epsilon)
        if noise is not None:
            noise = _in_layout_of(noise, epsilon)
        if epsilon_uncond is not None:
            epsilon_uncond = _in_layout_of(epsilon_uncond, epsilon)
        return HF.diffusion_reverse_step(kind, x, epsilon, int(t), self.tables, noise=noise,
                                         eps_uncond=epsilon_uncond, scale=scale, eta=eta,
                                         clip=self.clip_sample)

    def ddpm_reverse_step(self, x: torch.Tensor, epsilon: torch.Tensor, t: int, eta: float = 1.0,
                          epsilon_uncond: torch.Tensor = None, scale: float = 0.0):
        t = int(t)
        noise = self.randn_like(x) if t > 0 and eta > 0 else None
        return self._reverse("ddpm", x, epsilon, t, eta, noise, epsilon_uncond, scale)

    def ddim_reverse_step(self, x: torch.Tensor, epsilon: torch.Tensor, t: int, eta: float = 1.0,
                          epsilon_uncond: torch.Tensor = None, scale: float = 0.0):
        noise = self.randn_like(epsilon)
        return self._reverse("ddim", x, epsilon, int(t), eta, noise, epsilon_uncond, scale)

    def alpha_deblending_step(self, x: torch.Tensor, epsilon: torch.Tensor, t: int,
                              eta: float = None, epsilon_uncond: torch.Tensor = None,
                              scale: float = 0.0):
        return self._reverse("alpha_deblending", x, epsilon, int(t), 1.0, None, epsilon_uncond, scale)

    def step(self, x: torch.Tensor, epsilon: torch.Tensor, t: int, eta: float = 1.0,
             epsilon_uncond: torch.Tensor = None, scale: float = 0.0):
        kw = dict(epsilon_uncond=epsilon_uncond, scale=scale)
        if self.step_key == "ddpm":
            return self.ddpm_reverse_step(x, epsilon=epsilon, t=t, eta=eta, **kw)
        elif self.step_key == "ddim":
            return self.ddim_reverse_step(x, epsilon=epsilon, t=t, eta=eta, **kw)
        elif self.step_key == "alpha_deblending":
            return self.alpha_deblending_step(x, epsilon=epsilon, t=t, eta=None, **kw)

    @torch.no_grad()
    def sample(self, model: torch.nn.Module, n: int = 1, in_channels: int = 1,
               x: torch.Tensor = None, classification: torch.Tensor = None,
               classification_scale: float = 3.0, start_from: int = None) -> torch.Tensor:
        """Samples an image from a diffusion model: the arguments of the reference's ``sample``.
        With ``classification`` and a positive ``classification_scale`` the unconditioned prediction
        is shifted towards the conditioned one inside the step's launch."""
        if classification is not None:
            n = classification.shape[0]
        if x is not None:
            n = x.shape[0]
        else:
            # fetch a model parameter to retrieve parameter
            device = next(model.parameters()).device
            x = torch.randn((n, in_channels, *self.img_size)).to(device)
        model.eval()
        final_t = self.noise_steps if start_from is None else start_from
        t_range = reversed(range(1, final_t))
        if self.track_progress is True:
            from tqdm.auto import tqdm

            t_range = tqdm(t_range, total=final_t - 1, desc="Generating...", position=0, leave=True)
        for i in t_range:
            # (a fill kernel: the reference's torch.as_tensor([i], device=...) is a host copy per step)
            t = torch.full((1,), i / self.noise_steps, dtype=torch.float32, device=x.device)
            predicted_noise = model(x, t, classification)
            nonconditional_predicted_noise = None
            if classification is not None and classification_scale > 0:
                nonconditional_predicted_noise = model(x, t)
            x = self.step(x=x, epsilon=predicted_noise, t=i,
                          epsilon_uncond=nonconditional_predicted_noise, scale=classification_scale)
        model.train()
        return x
