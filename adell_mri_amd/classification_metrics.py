"""Classification metrics on the device, with the surface of ``metrics.SegMetric`` (``update`` /
``compute`` / ``compute_async`` / ``reset`` / ``_apply`` / ``num_classes``) and torchmetrics' names,
for the metric dicts of the classification wrappers (adell_mri/modules/classification/pl.py:64-160).
torchmetrics is not a dependency and is not installed where this package is built and tested: the
definitions below are the package's own, as for the segmentation metrics; tests pin them to fp64
restatements, and those to scikit-learn and scipy where these are present.

Counts. Every count-based metric keeps an int64 confusion matrix [C, C] (row: label, column:
predicted class) and a bad-target counter on the device; ``update`` adds one batch with one HIP
launch (``csrc/classify.hip``, integer atomics) and never synchronises with the host.
``update_many`` feeds a whole dict from one launch. Predictions: fp32 [N, C] (argmax: the first
maximal index, a NaN wins, as ``metrics.py`` documents), fp32 [N] probabilities (``p > 0.5``, binary
only), or integer classes [N] (the ordinal metrics; floating-point classes are rounded). Labels are
class indices (floating-point labels are rounded half-to-even).

=============  ===========================================  ================
metric         value (per class, from tp, fp, fn, tn)       zero denominator
=============  ===========================================  ================
Recall         tp / (tp + fn)                               0
Specificity    tn / (tn + fp)                               0
Precision      tp / (tp + fp)                               0
F-beta         (1+b^2) tp / ((1+b^2) tp + b^2 fn + fp)      0
=============  ===========================================  ================

Binary metrics report class 1. Multi-class metrics take ``average`` in {"macro", "none"}: "macro" is
the mean over the classes with tp + fp + fn > 0 (0 when there are none), "none" the [C] vector --
the conventions ``metrics.py`` fixes.

Scores. ``BinaryAUROC`` and ``MulticlassAUROC`` keep the scores and labels of every update as a
list of device tensors, concatenated at ``compute``. The value is exact: ``csrc/classify.hip`` counts,
over the pairs of a positive and a negative, 2 for ``pos > neg`` and 1 for a tie; AUC = count /
(2 P Nneg) in fp64 (the Mann-Whitney statistic, what the trapezoidal rule over the ROC curve gives).
No positive or no negative: NaN. ``MulticlassAUROC`` is one-vs-rest, macro over the classes that
have both a positive and a negative; NaN when none has.

Ordinal metrics, all from the counts of (predicted class, label): ``MeanSquaredError``,
``PearsonCorrCoef`` (NaN at zero variance), ``SpearmanCorrCoef`` (average ranks from the marginals)
and ``CohenKappa(weights="quadratic")``.

Bad targets (a label outside [0, C), or an integer prediction outside it): ``update`` records a
count, ``compute`` raises ``RuntimeError``.

State: plain tensor attributes moved by an ``_apply`` override, not registered buffers. With
``torch.distributed`` initialised on more than one rank, ``compute`` first sums the counts over the
ranks (one ``all_reduce``); the stored scores are gathered (lengths exchanged, then one padded
``all_gather``). The gather has been run at world size 1 only.

``"CalErr"`` (calibration error) is not built: it is left out of the default key list of
``get_metric_dict``, and asking for it by key raises ``NotImplementedError``.
"""
import torch

from . import ops


def _as_labels(target):
    target = target.detach().reshape(-1)
    if target.is_floating_point():
        target = torch.round(target)
    return target.to(torch.int64)


def _confusion_delta(preds, target, num_classes):
    """int64 [C * C + 1]: the counts of one update."""
    preds = preds.detach()
    if preds.dim() == 2 and preds.shape[1] == 1:
        preds = preds[:, 0]
    if preds.is_floating_point() and preds.dtype != torch.float32:
        preds = preds.float()
    elif not preds.is_floating_point() and preds.dtype != torch.int64:
        preds = preds.to(torch.int64)
    delta = torch.zeros(num_classes * num_classes + 1, dtype=torch.int64, device=preds.device)
    ops.cls_confusion_update(preds.contiguous(), _as_labels(target).to(preds.device), delta)
    return delta


class ClassMetric(torch.nn.Module):
    """Base of the count-based metrics."""

    ordinal = False      # ordinal metrics take classes, not scores: floating-point input is rounded

    def __init__(self, num_classes: int):
        super().__init__()
        num_classes = int(num_classes)
        if num_classes < 2:
            raise ValueError(f"{type(self).__name__}: num_classes must be >= 2, got {num_classes}")
        self.num_classes = num_classes
        self.state = torch.zeros(num_classes * num_classes + 1, dtype=torch.int64)

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.state = fn(self.state)       # device moves; dtype casts leave integer tensors alone
        return self

    @property
    def device(self):
        return self.state.device

    def _prepare(self, preds):
        if self.ordinal and preds.is_floating_point():
            return torch.round(preds.detach()).to(torch.int64).reshape(-1)
        return preds

    def _add(self, delta):
        if self.state.device != delta.device:
            self.state = self.state.to(delta.device)
        self.state += delta

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self._add(_confusion_delta(self._prepare(preds), target, self.num_classes))

    def forward(self, preds, target):
        self.update(preds, target)

    def reset(self) -> None:
        self.state.zero_()

    def _synced_state(self):
        import torch.distributed as dist

        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            s = self.state.clone()
            dist.all_reduce(s)
            return s
        return self.state

    def bad_target_message(self):
        return (f"classification metric: a label (or an integer prediction) lies outside "
                f"[0, {self.num_classes}) in an update since the last reset()")

    def _value(self, M):
        raise NotImplementedError

    def compute_async(self):
        """(value, bad-target count) as device tensors: no host synchronisation."""
        s = self._synced_state()
        C = self.num_classes
        return self._value(s[:C * C].view(C, C).double()).float(), s[-1]

    def compute(self) -> torch.Tensor:
        value, bad = self.compute_async()
        if int(bad) > 0:
            raise RuntimeError(self.bad_target_message())
        return value

    def extra_repr(self):
        return f"num_classes={self.num_classes}"


def _ratio(num, den):
    """num / den, 0 where den == 0."""
    return torch.where(den > 0, num / torch.where(den > 0, den, torch.ones_like(den)),
                       torch.zeros_like(den))


def _class_counts(M):
    tp = M.diagonal()
    fp = M.sum(0) - tp
    fn = M.sum(1) - tp
    tn = M.sum() - tp - fp - fn
    return tp, fp, fn, tn


_KINDS = {
    "recall": lambda tp, fp, fn, tn, b2: _ratio(tp, tp + fn),
    "specificity": lambda tp, fp, fn, tn, b2: _ratio(tn, tn + fp),
    "precision": lambda tp, fp, fn, tn, b2: _ratio(tp, tp + fp),
    "fbeta": lambda tp, fp, fn, tn, b2: _ratio((1 + b2) * tp, (1 + b2) * tp + b2 * fn + fp),
}


class _Binary(ClassMetric):
    """``threshold``: a probability counts as class 1 when ``p > threshold``. The default 0.5 is the
    update kernel's own comparison; another value thresholds the probabilities first."""

    kind = None

    def __init__(self, beta: float = 1.0, threshold: float = 0.5):
        super().__init__(2)
        if not beta > 0:
            raise ValueError(f"{type(self).__name__}: beta must be positive, got {beta}")
        self.beta = float(beta)
        self.threshold = float(threshold)

    def _prepare(self, preds):
        if self.threshold != 0.5 and preds.is_floating_point() and (
                preds.dim() == 1 or (preds.dim() == 2 and preds.shape[1] == 1)):
            return (preds.detach().reshape(-1) > self.threshold).to(torch.int64)
        return super()._prepare(preds)

    def _value(self, M):
        return _KINDS[self.kind](*_class_counts(M), self.beta ** 2)[1]


class BinaryRecall(_Binary):
    kind = "recall"


class BinarySpecificity(_Binary):
    kind = "specificity"


class BinaryPrecision(_Binary):
    kind = "precision"


class BinaryFBetaScore(_Binary):
    kind = "fbeta"

    def __init__(self, beta: float, threshold: float = 0.5):
        super().__init__(beta, threshold)


class _Multiclass(ClassMetric):
    kind = None

    def __init__(self, num_classes: int, average: str = "macro", beta: float = 1.0):
        super().__init__(num_classes)
        if average not in ("macro", "none"):
            raise NotImplementedError(f"{type(self).__name__}: average must be 'macro' or 'none', "
                                      f"got {average!r}")
        if not beta > 0:
            raise ValueError(f"{type(self).__name__}: beta must be positive, got {beta}")
        self.average, self.beta = average, float(beta)

    def _value(self, M):
        tp, fp, fn, tn = _class_counts(M)
        per_class = _KINDS[self.kind](tp, fp, fn, tn, self.beta ** 2)
        if self.average == "none":
            return per_class
        seen = (tp + fp + fn > 0).double()
        return _ratio((per_class * seen).sum(), seen.sum())


class MulticlassRecall(_Multiclass):
    kind = "recall"


class MulticlassSpecificity(_Multiclass):
    kind = "specificity"


class MulticlassPrecision(_Multiclass):
    kind = "precision"


class MulticlassFBetaScore(_Multiclass):
    kind = "fbeta"


# ---- ordinal metrics: the counts of (label, predicted class) ---------------------------------------
def _weighted_pearson(M, rows, cols):
    """Pearson's r of the value ``rows[l]`` of a label and ``cols[p]`` of a prediction over the
    samples M counts; 0 / 0 = NaN at zero variance."""
    n = M.sum()
    mr = (M.sum(1) * rows).sum() / n
    mc = (M.sum(0) * cols).sum() / n
    dr, dc = rows - mr, cols - mc
    cov = (M * dr[:, None] * dc[None, :]).sum()
    return cov / torch.sqrt((M.sum(1) * dr * dr).sum() * (M.sum(0) * dc * dc).sum())


def _average_ranks(marginal):
    """The average rank (1-based) of each value, from how often each occurs."""
    return marginal.cumsum(0) - marginal + (marginal + 1) / 2


class _Ordinal(ClassMetric):
    ordinal = True


class MeanSquaredError(_Ordinal):
    def _value(self, M):
        c = torch.arange(self.num_classes, device=M.device, dtype=torch.float64)
        return (M * (c[:, None] - c[None, :]) ** 2).sum() / M.sum()


class PearsonCorrCoef(_Ordinal):
    def _value(self, M):
        c = torch.arange(self.num_classes, device=M.device, dtype=torch.float64)
        return _weighted_pearson(M, c, c)


class SpearmanCorrCoef(_Ordinal):
    def _value(self, M):
        return _weighted_pearson(M, _average_ranks(M.sum(1)), _average_ranks(M.sum(0)))


class CohenKappa(_Ordinal):
    def __init__(self, num_classes: int, weights: str = "quadratic"):
        super().__init__(num_classes)
        if weights != "quadratic":
            raise NotImplementedError(f"CohenKappa: weights must be 'quadratic', got {weights!r}")
        self.weights = weights

    def _value(self, M):
        c = torch.arange(self.num_classes, device=M.device, dtype=torch.float64)
        w = (c[:, None] - c[None, :]) ** 2 / (self.num_classes - 1) ** 2
        expected = M.sum(1)[:, None] * M.sum(0)[None, :] / M.sum()
        return 1 - (w * M).sum() / (w * expected).sum()


# ---- AUROC: stored scores ----------------------------------------------------------------------------
def _gather_rows(t):
    """The rows of ``t`` [n, ...] of every rank, in rank order: lengths exchanged, then one padded
    ``all_gather``. (Run at world size 1 only.)"""
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return t
    world = dist.get_world_size()
    n = torch.tensor([t.shape[0]], device=t.device, dtype=torch.int64)
    lengths = [torch.zeros_like(n) for _ in range(world)]
    dist.all_gather(lengths, n)
    lengths = [int(v) for v in torch.cat(lengths).tolist()]
    padded = t.new_zeros((max(lengths),) + tuple(t.shape[1:]))
    padded[:t.shape[0]] = t
    parts = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(parts, padded)
    return torch.cat([p[:k] for p, k in zip(parts, lengths)])


def _auc(scores, labels):
    """(AUC as an fp64 0-d tensor, NaN without a positive or a negative; has-both flag)."""
    c = ops.cls_auroc_pairs(scores.contiguous(), labels.contiguous()).double()
    pairs = c[1] * c[2]
    return c[0] / (2 * pairs), pairs > 0


class _AUROC(torch.nn.Module):
    def __init__(self, num_classes: int):
        super().__init__()
        self.num_classes = int(num_classes)
        self.scores, self.labels = [], []

    def _apply(self, fn, recurse=True):
        super()._apply(fn, recurse)
        self.scores = [fn(s) for s in self.scores]
        self.labels = [fn(t) for t in self.labels]
        return self

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        preds = preds.detach().float()
        if self.num_classes == 2:
            preds = preds.reshape(-1)
        elif preds.dim() != 2 or preds.shape[1] != self.num_classes:
            raise ValueError(f"{type(self).__name__}: scores [N, {self.num_classes}] expected, got "
                             f"{tuple(preds.shape)}")
        labels = _as_labels(target).to(preds.device)
        if labels.shape[0] != preds.shape[0]:
            raise ValueError(f"{type(self).__name__}: {preds.shape[0]} scores for {labels.shape[0]} "
                             "labels")
        self.scores.append(preds.clone())
        self.labels.append(labels)

    def forward(self, preds, target):
        self.update(preds, target)

    def reset(self) -> None:
        self.scores, self.labels = [], []

    def bad_target_message(self):
        return (f"classification metric: a label lies outside [0, {self.num_classes}) in an update "
                f"since the last reset()")

    def _value(self, scores, labels):
        raise NotImplementedError

    def compute_async(self):
        if not self.scores:
            raise RuntimeError(f"{type(self).__name__}.compute() before any update()")
        scores = _gather_rows(torch.cat(self.scores))
        labels = _gather_rows(torch.cat(self.labels))
        bad = ((labels < 0) | (labels >= self.num_classes)).sum()
        return self._value(scores, labels).float(), bad

    def compute(self) -> torch.Tensor:
        value, bad = self.compute_async()
        if int(bad) > 0:
            raise RuntimeError(self.bad_target_message())
        return value


class BinaryAUROC(_AUROC):
    def __init__(self):
        super().__init__(2)

    def _value(self, scores, labels):
        return _auc(scores, labels)[0]


class MulticlassAUROC(_AUROC):
    def __init__(self, num_classes: int):
        super().__init__(num_classes)
        if self.num_classes < 2:
            raise ValueError(f"MulticlassAUROC: num_classes must be >= 2, got {num_classes}")

    def _value(self, scores, labels):
        in_range = (labels >= 0) & (labels < self.num_classes)
        values, flags = [], []
        for c in range(self.num_classes):
            # one-vs-rest: 1 for the class, 0 for every other valid label, -1 (skipped) otherwise
            one = torch.where(in_range, (labels == c).to(torch.int64), torch.full_like(labels, -1))
            v, ok = _auc(scores[:, c], one)
            values.append(torch.where(ok, v, torch.zeros_like(v)))
            flags.append(ok.double())
        return torch.stack(values).sum() / torch.stack(flags).sum()       # 0 / 0: NaN


def update_many(metrics, preds, target):
    """One update of every metric in ``metrics`` with the same prediction and target: the
    count-based ones of one kind of input share ONE confusion launch; the AUROCs keep the scores."""
    shared = {}
    for m in metrics:
        if isinstance(m, ClassMetric):
            key = (m.num_classes, m.ordinal, getattr(m, "threshold", 0.5))
            if key not in shared:
                shared[key] = _confusion_delta(m._prepare(preds), target, m.num_classes)
            m._add(shared[key])
        else:
            m.update(preds, target)


def get_ordinal_metric_dict(nc: int, metric_keys: list[str] = None, prefix: str = ""):
    """pl.py:64-98; keys "Pearson", "Spearman", "MSE", "Kappa" (None: all). Every metric takes the
    number of classes: all are computed from the [nc, nc] counts."""
    md = {"Pearson": lambda: PearsonCorrCoef(nc), "Spearman": lambda: SpearmanCorrCoef(nc),
          "MSE": lambda: MeanSquaredError(nc), "Kappa": lambda: CohenKappa(nc, weights="quadratic")}
    metric_dict = torch.nn.ModuleDict({})
    for k in (list(md.keys()) if metric_keys is None else metric_keys):
        if k in md:
            metric_dict[prefix + k] = md[k]()
    return metric_dict


def get_metric_dict(nc: int, metric_keys: list[str] = None, prefix: str = "", average: str = "macro"):
    """pl.py:101-160; keys "Rec", "Spe", "Pr", "F1", "AUC" (None: all of these). "CalErr" raises
    ``NotImplementedError``; any other unknown key is skipped, as in the reference."""
    if nc == 2:
        md = {"Rec": BinaryRecall, "Spe": BinarySpecificity, "Pr": BinaryPrecision,
              "F1": lambda: BinaryFBetaScore(1.0), "AUC": BinaryAUROC}
    else:
        md = {"Rec": lambda: MulticlassRecall(nc, average=average),
              "Spe": lambda: MulticlassSpecificity(nc, average=average),
              "Pr": lambda: MulticlassPrecision(nc, average=average),
              "F1": lambda: MulticlassFBetaScore(nc, average=average),
              "AUC": lambda: MulticlassAUROC(nc)}
    metric_dict = torch.nn.ModuleDict({})
    for k in (list(md.keys()) if metric_keys is None else metric_keys):
        if k == "CalErr":
            raise NotImplementedError("metric key 'CalErr': the calibration error is not built")
        if k in md:
            metric_dict[prefix + k] = md[k]()
    return metric_dict
