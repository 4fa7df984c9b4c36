"""Parameter groups by name and an early-stopping check, with the semantics of the reference's
adell_mri/modules/continuous_learning/optim.py. The groups are what ``torch.optim`` optimisers and the
fused ones (``adell_mri_amd.optim``) take as ``params``."""
from typing import Dict, List, Union

import torch

ParamGroupDict = Dict[str, Union[List[torch.nn.Parameter], float, int, bool, str]]


def create_param_groups(
    model: torch.nn.Module,
    var_groups: List[Union[List[str], str]],
    kwargs_groups: List[Dict[str, Union[str, int, float, bool]]] = None,
    include_leftovers: bool = True,
) -> List[ParamGroupDict]:
    """One optimiser parameter group per entry of ``var_groups``.

    Args:
        model (torch.nn.Module): the model whose ``named_parameters()`` are sorted into groups.
        var_groups (List[Union[List[str],str]]): per group either a list of exact parameter names
            (names that match nothing are ignored) or a string, which selects every parameter
            whose name contains it. A parameter matching several groups lands in each of them; a
            group may stay empty (the fused optimisers accept that).
        kwargs_groups (List[Dict], optional): per group, further optimiser settings (``lr``, ...),
            same length as ``var_groups``. Defaults to None (no settings).
        include_leftovers (bool, optional): append a last group with the parameters no entry
            matched. Defaults to True.

    Returns:
        the list of group dicts (``{"params": [...], **settings}``).
    """
    if kwargs_groups is None:
        kwargs_groups = [{} for _ in var_groups]
    if len(kwargs_groups) != len(var_groups):
        raise AssertionError("len(kwargs_groups) should be the same as len(var_groups)")
    groups = [{"params": [], **settings} for settings in kwargs_groups]
    leftovers = {"params": []}
    for name, param in model.named_parameters():
        matched = False
        for group, selector in zip(groups, var_groups):
            if isinstance(selector, list):
                hit = name in selector
            elif isinstance(selector, str):
                hit = selector in name
            else:
                hit = False
            if hit:
                group["params"].append(param)
                matched = True
        if not matched:
            leftovers["params"].append(param)
    if include_leftovers is True:
        groups.append(leftovers)
    return groups


class EarlyStopper:
    """Says when the validation loss has not improved for ``patience`` checks in a row.

    Args:
        patience (int, optional): checks without improvement before it says stop. Defaults to 1.
        min_delta (float, optional): how far above the best loss so far a loss has to be to count as
            "not improving". Defaults to 0.
    """

    def __init__(self, patience: int = 1, min_delta: float = 0.0):
        self.patience, self.min_delta = patience, min_delta
        self.counter = 0                              # checks in a row without improvement
        self.min_validation_loss = float("inf")       # the best loss so far

    def __call__(self, validation_loss) -> bool:
        """``validation_loss``: a number or a one-element tensor on any device (read back with one
        ``float()``). Returns whether training (or the current phase) should stop."""
        loss, best = float(validation_loss), self.min_validation_loss
        if loss < best:                 # a new best: the count starts again
            self.min_validation_loss, self.counter = loss, 0
            return False
        if not loss > best + self.min_delta:       # inside the margin (or NaN): neither better nor worse
            return False
        self.counter += 1
        return self.counter >= self.patience
