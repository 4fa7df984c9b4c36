"""Staged learning rates per parameter group (the reference's
adell_mri/modules/continuous_learning/callbacks.py: constructor and assertions). The reference's hook
body cannot run -- it indexes the Trainer like a dict and asks the callback for the optimisers -- so
``on_validation_epoch_end`` is this package's own: ``trainer`` is anything with ``current_epoch``,
``callback_metrics`` and ``should_stop`` (a Lightning Trainer, or ``trainer.StepRunner``)."""
from typing import List, Union

from .optim import EarlyStopper


class MultiPhaseTraining:
    """Phase ``i`` runs with ``learning_rates[i]`` (one learning rate per parameter group of the
    optimiser, or ``"stop"``) and ends at epoch ``n_epochs[i]`` or, for ``"adaptive"``, once
    ``monitor`` has not improved for ``patience`` epochs. Phase 0 is the optimiser as it was built.

    Args:
        learning_rates (List[Union[List[float],str]]): per phase a list with one learning rate per
            parameter group, or "stop", which stops training.
        n_epochs (List[Union[str,int]]): per phase the epoch at which the NEXT phase begins, or
            "adaptive" (an early-stopping-like check on ``monitor`` ends the phase).
        monitor (str, optional): key of ``trainer.callback_metrics`` watched by "adaptive" phases.
        patience (int, optional): epochs without improvement that end an "adaptive" phase.
            Defaults to 10.
        min_delta (float, optional): see ``EarlyStopper``. Defaults to 0.0.
    """

    def __init__(
        self,
        learning_rates: List[Union[List[float], str]],
        n_epochs: List[Union[str, int]],
        monitor: str = None,
        patience: int = 10,
        min_delta: float = 0.0,
    ):
        self.learning_rates, self.n_epochs = learning_rates, n_epochs
        self.monitor, self.patience, self.min_delta = monitor, patience, min_delta
        self.assertions()
        self.idx = 0                      # the current phase
        self.checker = self._fresh_checker()

    def _fresh_checker(self):
        return EarlyStopper(patience=self.patience, min_delta=self.min_delta)

    def assertions(self):
        """The constructor's checks (AssertionError, with the reference's messages)."""
        phases, ends = self.learning_rates, self.n_epochs
        if len(phases) != len(ends):
            raise AssertionError("len(learning_rates) should be the same as len(n_epochs)")
        for end in ends:
            if end != "adaptive" and not isinstance(end, int):
                raise AssertionError("n_epochs should only have integers or 'adaptive'")
        for lrs in phases:
            if lrs != "stop" and not isinstance(lrs, list):
                raise AssertionError("learning_rates should only contain lists of floats or 'stop'")

    @staticmethod
    def _optimizer(trainer, pl_module):
        opt = getattr(trainer, "optimizer", None)
        if opt is None:
            opt = pl_module.optimizers()
        if isinstance(opt, (list, tuple)):
            opt = opt[0]
        return opt

    def on_validation_epoch_end(self, trainer, pl_module):
        """Move to the next phase if the current one is over: set one ``param_group["lr"]`` per
        entry of the new phase (``trainer.optimizer`` if there is one, else
        ``pl_module.optimizers()``), or ``trainer.should_stop = True`` for "stop". Every phase
        starts a fresh ``EarlyStopper``. In the last phase nothing happens any more (the reference
        would raise IndexError)."""
        if self.idx + 1 >= len(self.learning_rates):
            return
        end = self.n_epochs[self.idx]
        if end == "adaptive":
            metrics = trainer.callback_metrics
            if self.monitor not in metrics:
                raise KeyError(f"MultiPhaseTraining: monitor {self.monitor!r} is not in "
                               f"trainer.callback_metrics ({sorted(metrics)})")
            changed = self.checker(metrics[self.monitor]) is True
        else:
            changed = trainer.current_epoch >= end
        if not changed:
            return
        self.idx += 1
        self.checker = self._fresh_checker()
        phase = self.learning_rates[self.idx]
        if phase == "stop":
            trainer.should_stop = True
            return
        groups = self._optimizer(trainer, pl_module).param_groups
        for i in range(min(len(groups), len(phase))):
            groups[i]["lr"] = phase[i]
