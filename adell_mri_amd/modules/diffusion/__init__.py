from .diffusion_process import (Diffusion, cosine_beta_schedule, linear_beta_schedule,  # noqa: F401
                                quadratic_beta_schedule, scaled_linear_beta_schedule,
                                sigmoid_beta_schedule)
from .pl import DDPMUNetPL  # noqa: F401
from .unet import DiffusionUNet, get_timestep_embedding  # noqa: F401
