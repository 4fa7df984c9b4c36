"""Interval calculation by bootstrapping (mirror of adell_mri/utils/bootstrap_metrics.py):
``cat_if_necessary`` and ``bootstrap_metric``, with the reference's arguments, draw and return value
``(mean [K], quantiles [2, K])``, K = 1 for a scalar metric.

The draw is the reference's: a CPU ``torch.Generator`` seeded with ``seed`` unless one is given, and per
resample ``torch.randperm(n, generator=generator)[:sample_size]`` (``int(sample_size * n)`` for a float,
``samples = int(20 / significance - 1)`` when None). The rows are stacked and uploaded once as int32
``[R, m]``. ``sample_idxs`` (an integer tensor ``[R, m]`` of distinct indices per row) replaces the draw.

Fast path: ``metric`` is a ``classification_metrics.BinaryAUROC`` or ``MulticlassAUROC`` whose stored
scores are on the GPU. The scores of each class are sorted ONCE and all R AUCs come from one launch
per class (``ops.boot_auroc_pairs``: exact integer pair counts, bit-reproducible), where the reference
resets, updates and computes the metric once per resample. A resample without a positive or without a
negative is NaN, the metric's own convention, and the NaN reaches the mean and the quantiles as it
would in the reference's loop. The multiclass value is the metric's macro over the classes that have
both in that resample; labels outside ``[0, C)`` are skipped as in ``MulticlassAUROC._value``. The mean
over the resamples is taken in fp64, the quantiles by ``torch.quantile`` at ``[lower, upper]`` on the
fp64 values, and both are cast to fp32. Beyond ``ops.BOOT_MAX_N`` stored samples
(``ops.boot_auroc_route``) the same rows go through one ``cls_auroc_pairs`` per resample and class.

Deviation: the metric's stored state is NOT reset -- the reference leaves the metric holding the last
resample, here it still holds every update.

Generic path: any other object with ``preds`` and ``target`` attributes takes the reference's loop
unchanged (reset, update, compute per resample), on whatever device it lives, except that the rows of
``sample_idxs`` are used when given and there is no progress bar. Anything else raises
``NotImplementedError`` with the reference's message -- a count-based ``ClassMetric`` among them, as a
torchmetrics count metric does in the reference.
"""
import torch

from .. import classification_metrics as CM
from .. import ops


def cat_if_necessary(tensor: torch.Tensor | list[torch.Tensor]) -> torch.Tensor:
    """Concatenates a list into a torch.Tensor if the input is a list."""
    if isinstance(tensor, list):
        tensor = torch.cat(tensor, 0)
    return tensor


def draw_sample_idxs(n: int, samples: int, sample_size: int,
                     generator: torch.Generator) -> torch.Tensor:
    """int64 [samples, sample_size] on the CPU: the reference's draw, one ``randperm`` per row."""
    rows = [torch.randperm(n, generator=generator)[:sample_size] for _ in range(samples)]
    if not rows:
        return torch.zeros((0, sample_size), dtype=torch.int64)
    return torch.stack(rows)


def _one_vs_rest(metric, labels):
    """[(class column | None, labels as 1 / 0 / -1)] of an AUROC metric."""
    if isinstance(metric, CM.BinaryAUROC):
        return [(None, labels)]
    in_range = (labels >= 0) & (labels < metric.num_classes)
    return [(c, torch.where(in_range, (labels == c).to(torch.int64), torch.full_like(labels, -1)))
            for c in range(metric.num_classes)]


def _auroc_counts(scores, one, idx, route):
    """int64 [R, 3]: (2 #{pos > neg} + #{pos == neg}, positives, negatives) per row of idx."""
    if route == "bitmask":
        return ops.boot_auroc_pairs(idx, *ops.boot_auroc_tables(scores, one))[:, :3]
    rows = idx.to(torch.int64)
    if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= scores.shape[0] or bool(
            (torch.sort(rows, 1).values.diff(dim=1) == 0).any())):
        raise ValueError(f"bootstrap_metric: a resample holds an index twice or one outside "
                         f"[0, {scores.shape[0]})")
    return torch.stack([ops.cls_auroc_pairs(scores[r].contiguous(), one[r].contiguous())
                        for r in rows])


def bootstrap_auroc_values(metric, sample_idxs):
    """fp64 [R] on the device: the value of an AUROC metric on every row of ``sample_idxs`` (int32
    [R, m] on the device), from the stored scores, which are left as they are."""
    if not metric.scores:
        raise RuntimeError(f"{type(metric).__name__}: bootstrap before any update()")
    scores = torch.cat(metric.scores)
    labels = torch.cat(metric.labels)
    route = ops.boot_auroc_route(scores.shape[0])
    total = torch.zeros(sample_idxs.shape[0], device=scores.device, dtype=torch.float64)
    classes = torch.zeros_like(total)
    for c, one in _one_vs_rest(metric, labels):
        s = scores if c is None else scores[:, c].contiguous()
        counts = _auroc_counts(s, one, sample_idxs, route).double()
        pairs = counts[:, 1] * counts[:, 2]
        if c is None:
            return counts[:, 0] / (2 * pairs)                      # 0 / 0: NaN
        ok = pairs > 0
        total += torch.where(ok, counts[:, 0] / (2 * torch.where(ok, pairs, torch.ones_like(pairs))),
                             torch.zeros_like(pairs))
        classes += ok.double()
    return total / classes                                         # 0 / 0: NaN


def bootstrap_metric(
    metric,
    samples: int = None,
    sample_size: float = 0.5,
    interval: float = 0.95,
    significance: float = 0.05,
    generator: torch.Generator = None,
    seed: int = 42,
    sample_idxs: torch.Tensor = None,
) -> tuple[torch.Tensor, torch.Tensor]:
    fast = isinstance(metric, (CM.BinaryAUROC, CM.MulticlassAUROC)) and bool(metric.scores) and all(
        s.is_cuda for s in metric.scores)
    if not fast and (hasattr(metric, "preds") is False or hasattr(metric, "target") is False):
        raise NotImplementedError(
            "Bootstrapping only possible if preds and target are defined in \
                metric"
        )
    if generator is None:
        generator = torch.Generator()
        generator.manual_seed(seed)
    lower = (1 - interval) / 2
    upper = interval + lower
    if fast:
        n = sum(int(s.shape[0]) for s in metric.scores)
    else:
        preds = cat_if_necessary(metric.preds)
        target = cat_if_necessary(metric.target)
        n = preds.shape[0]
    if sample_idxs is None:
        if isinstance(sample_size, float):
            sample_size = int(sample_size * n)
        if samples is None:
            # uses the heuristic proposed in [1]
            # [1] https://www.tandfonline.com/doi/abs/10.1080/07474930008800459
            samples = int(20 / significance - 1)
        sample_idxs = draw_sample_idxs(n, samples, sample_size, generator)
    elif sample_idxs.dim() != 2 or sample_idxs.is_floating_point():
        raise ValueError(f"bootstrap_metric: sample_idxs must be an integer tensor [R, m], got "
                         f"{sample_idxs.dtype} {tuple(sample_idxs.shape)}")
    elif sample_idxs.numel() and (int(sample_idxs.min()) < 0 or int(sample_idxs.max()) >= n):
        # before the cast to int32, which would fold a large value into the valid range
        raise ValueError(f"bootstrap_metric: sample_idxs holds an index outside [0, {n})")

    if fast:
        idx = sample_idxs.to(torch.int32).contiguous().to(metric.scores[0].device)
        all_samples = bootstrap_auroc_values(metric, idx)
        mean = all_samples.mean(0).float()
        quantiles = torch.quantile(
            all_samples, torch.as_tensor([lower, upper]).to(all_samples), dim=0).float()
        return mean.unsqueeze(-1), quantiles.unsqueeze(-1)

    all_samples = []
    for row in sample_idxs.to(torch.int64):
        row = row.to(preds.device)
        preds_sample = preds[row]
        target_sample = target[row]
        metric.reset()
        metric.update(preds_sample, target_sample)
        metric_value = metric.compute()
        if len(metric_value.shape) == 0:
            metric_value = metric_value.unsqueeze(0)
        all_samples.append(metric_value)

    all_samples = torch.cat(all_samples, 0)
    mean = all_samples.mean(0)
    quantiles = torch.quantile(
        all_samples, torch.as_tensor([lower, upper]).to(all_samples), dim=0
    )
    if len(mean.shape) == 0:
        mean = mean.unsqueeze(-1)
        quantiles = quantiles.unsqueeze(-1)
    return mean, quantiles
