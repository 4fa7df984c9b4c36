"""Trainer callbacks of the reference's ``utils/pl_callbacks.py`` that the HIP path carries:
``SpectralNorm`` (every entry point's ``--spectral_norm_power_iterations``). Lightning is not
installed, so the class is a plain object with the callback's methods, as the ``*PL`` wrappers are
plain modules; ``trainer.StepRunner(spectral_norm=...)`` calls ``setup``."""
import torch

from ..modules.layers.spectral_norm import spectral_norm


def reshape_weight_to_matrix(weight, dim=0):
    """The weight as a matrix with ``dim`` as its rows (torch's ``_reshape_weight_to_matrix``)."""
    if dim != 0:
        weight = weight.permute(dim, *[d for d in range(weight.dim()) if d != dim])
    return weight.reshape(weight.size(0), -1)


class SpectralNorm:
    """Puts the spectral-norm parametrization on every trainable parameter of rank >= 2 whose name
    contains ``name``, outside the modules whose class name is in ``exclude_modules`` (default: the
    Gaussian-process head, layer norm and the batch norms; ``"_SpectralNorm"`` always). That includes
    ``Embedding`` weights, as in the reference. ``bake_on_save``: ``on_save_checkpoint`` replaces the
    ``.original`` / ``._u`` / ``._v`` keys of the checkpoint's ``state_dict`` by the normalised weight
    under the plain name (such a checkpoint cannot resume spectral-norm training)."""

    def __init__(self, name="weight", exclude_modules=None, n_power_iterations=1, eps=1e-12,
                 bake_on_save=False):
        self.name = name
        self.n_power_iterations = n_power_iterations
        self.eps = eps
        self.bake_on_save = bake_on_save
        self.exclude_modules = exclude_modules
        if self.exclude_modules is None:
            self.exclude_modules = ["GaussianProcessLayer", "LayerNorm", "BatchNorm1d", "BatchNorm2d",
                                    "BatchNorm3d"]
        self.exclude_modules.extend(["_SpectralNorm"])

    def setup(self, trainer, pl_module, stage=None):
        if getattr(pl_module, "_spectral_norm_applied", False):
            return
        if stage == "fit" or stage is None:
            self._apply_spectral_norm(pl_module)

    def _apply_spectral_norm(self, model):
        """Every module's direct parameters; one that cannot be parametrised is reported and skipped."""
        for module in model.modules():
            if module.__class__.__name__ in self.exclude_modules:
                continue
            for param_name, param in list(module.named_parameters(recurse=False)):
                if param.requires_grad is False:
                    continue
                if self.name in param_name and param.ndim >= 2:
                    try:
                        spectral_norm(module, name=param_name,
                                      n_power_iterations=self.n_power_iterations, eps=self.eps)
                    except Exception as e:
                        print(f"Skipping spectral norm on {module.__class__.__name__}.{param_name}: {e}")
        model._spectral_norm_applied = True

    def on_save_checkpoint(self, trainer, pl_module, checkpoint):
        if not self.bake_on_save:
            return
        sd = checkpoint.get("state_dict")
        if sd is None:
            return
        for module_name, module in pl_module.named_modules():
            if not hasattr(module, "parametrizations"):
                continue
            for param_name in list(module.parametrizations.keys()):
                stem = f"{module_name}." if module_name else ""
                prefix = f"{stem}parametrizations.{param_name}"
                if f"{prefix}.original" not in sd:
                    continue
                with torch.no_grad():
                    # (the reference reads ``module.weight`` whatever the parameter is called)
                    sd[f"{stem}{param_name}"] = module.weight.detach().clone()
                for k in (f"{prefix}.original", f"{prefix}.0._u", f"{prefix}.0._v"):
                    sd.pop(k, None)
