"""Losses of the semi-supervised U-Net (adell_mri/modules/semi_supervised_segmentation/losses.py).
Built: ``LocalContrastiveLoss`` (the one the network factory wires, network_factories.py:602-620),
``LocalContrastiveLossWithAnchors`` (what ``UNetContrastiveSemiSL.step_semi_sl_anchors`` needs),
``NearestNeighbourLoss`` and ``PseudoLabelCrossEntropy``, each on fused HIP kernels (csrc/ssl.hip,
csrc/semisl.hip) for device tensors within the limits ``functional.semisl_route`` states, and in the
same torch ops as the reference for CPU tensors and beyond those limits. The helpers ``swap``,
``derangement`` and ``anchors_from_derangement`` draw what the reference draws.
``AnatomicalContrastiveLoss`` raises: see its message. World size 1 only: the losses see the local
batch, neither queues nor softmax statistics are reduced across ranks."""
from collections.abc import Sequence
from queue import Queue

import numpy as np
import torch
import torch.nn.functional as F

from ... import functional as HF
from ... import ops


def swap(xs: Sequence, a: int, b: int) -> None:
    """Swaps element ``a`` of ``xs`` with element ``b`` (losses.py:14-23)."""
    xs[a], xs[b] = xs[b], xs[a]


def derangement(n: int, rng: np.random.Generator = None, seed: int = 42) -> list[int]:
    """A permutation of 0 .. n-1 without a fixed point (losses.py:26-51): ``rng.choice(range(a))`` for
    a = 1 .. n-1 in that order, each followed by a swap (Sattolo's algorithm)."""
    if rng is None:
        rng = np.random.default_rng(seed)
    if n < 2:
        raise ValueError("A derangement requires at least 2 elements (n >= 2)")
    xs = [i for i in range(n)]
    for a in range(1, n):
        b = rng.choice(range(a))
        swap(xs, a, b)
    return xs


def anchors_from_derangement(X: torch.Tensor, rng: np.random.Generator | None = None) -> torch.Tensor:
    """``X`` with its items deranged (losses.py:54-74): one index op where the reference stacks a Python
    loop of ``X[idx]``; same values, and the gradient reaches ``X`` through the gather."""
    if rng is None:
        rng = np.random.default_rng()
    idx = torch.as_tensor(derangement(X.shape[0], rng=rng), dtype=torch.int64, device=X.device)
    return X.index_select(0, idx)


class LocalContrastiveLoss(torch.nn.Module):
    """losses.py:480-526: per voxel, the B x B cosine similarities between the features of view 2
    (rows) and view 1 (columns) / temperature, soft-maxed over the columns; the loss of item i is
    the mean over voxels of -log(max(softmax[i, i], 1e-8)). Returns [B]."""

    def __init__(self, temperature: float = 0.1, seed: int = 42):
        super().__init__()
        self.temperature = temperature
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.eps = torch.as_tensor(1e-8)

    def forward(self, X_1: torch.Tensor, X_2: torch.Tensor,
                anchors: torch.Tensor = None) -> torch.Tensor:
        if X_1.dim() == 4:  # 2-D network: depth-1 volume
            X_1, X_2 = X_1.unsqueeze(2), X_2.unsqueeze(2)
        return HF.loco_loss(X_1, X_2, self.temperature, float(self.eps))


class LocalContrastiveLossWithAnchors(torch.nn.Module):
    """losses.py:529-585, mirrored as written: ``sim_k[b, v] = cos(X[b, :, v], anchors_k[b, :, v]) /
    temperature``, ``p = softmax(sim_1)`` and ``q = softmax(sim_2)`` over the VOXELS of an item, and
    ``F.kl_div(p, q, reduction="none").sum(-1)``, whose ``input`` is expected to be a log-probability
    but is handed the probability ``p``: the loss of item b is ``sum_v (xlogy(q_v, q_v) - q_v p_v)``.
    That is kept. ``self.eps`` is stored and never used, as in the reference. Missing anchors are
    drawn from ``self.rng`` by derangement of ``X``, ``anchors_1`` first. 2-D inputs [B, C, H, W] are
    accepted. Returns [B]."""

    def __init__(self, temperature: float = 0.1, seed: int = 42):
        super().__init__()
        self.temperature = temperature
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.eps = torch.as_tensor(1e-8)

    def forward(self, X: torch.Tensor, anchors_1: torch.Tensor | None = None,
                anchors_2: torch.Tensor | None = None) -> torch.Tensor:
        anchors_1 = anchors_from_derangement(X, self.rng) if anchors_1 is None else anchors_1
        anchors_2 = anchors_from_derangement(X, self.rng) if anchors_2 is None else anchors_2
        return HF.loco_anchor_loss(X, anchors_1, anchors_2, self.temperature)


class AnatomicalContrastiveLoss(torch.nn.Module):
    """losses.py:77-251. Not built, on purpose (the ruling made for Barlow Twins): the reference writes
    its buffers ``average_representations`` and ``hard_examples`` in place from tensors that carry
    autograd history, so the backward of the SECOND training step fails with "Trying to backward
    through the graph a second time" (checked against the reference on the CPU: batch 2, three
    classes, top_k = 5; step 0 runs, steps 1 and 2 raise). There is no training behaviour to mirror."""

    def __init__(self, *args, **kwargs):
        raise NotImplementedError(
            "AnatomicalContrastiveLoss (losses.py:77-251) is not built: the reference updates its "
            "buffers in place from tensors with autograd history, so the backward of the second "
            "training step raises 'Trying to backward through the graph a second time'; a loss that "
            "cannot train past its first step is not mirrored")


class NearestNeighbourLoss(torch.nn.Module):
    """losses.py:254-444 (after Frosst 2019): per-class FIFO queues of past embeddings; the loss pulls
    the embedding of every voxel towards queued samples of its classes. The per-class ``queue.Queue``
    objects and every numpy draw are the reference's, in its order: ``put`` draws
    ``rng.choice(n_elements, max_elements_per_batch)`` -- WITH replacement -- only when a class has
    more than ``max_elements_per_batch`` positives; ``get_from_class`` draws ``rng.choice(n_elements, n)``
    and uses only its length. The queue holds detached tensors [n, C] on the device of ``X``.
    ``forward`` drains the queue and returns a 0-d zero when it is empty.

    Device tensors: ``put`` counts ``y > 0`` per (item, class) on the device, reads that small table
    (its one host read) and gathers only the selected rows (``ops.nn_queue_put``); ``forward`` is
    ``functional.nn_queue_loss``, which never writes a [B, V, Q] tensor."""

    def __init__(self, maxsize: int, n_classes: int, max_elements_per_batch: int,
                 n_samples_per_class: int, temperature: float = 0.1, seed: int = 42):
        super().__init__()
        self.maxsize = maxsize
        self.n_classes = n_classes
        self.max_elements_per_batch = max_elements_per_batch
        self.n_samples_per_class = n_samples_per_class
        self.temperature = temperature
        self.seed = seed

        self.q = [Queue(maxsize=self.maxsize) for _ in range(self.n_classes)]
        self.rng = np.random.default_rng(seed)

    def _select(self, counts):
        """Per class: None (nothing to queue) or the ranks to keep, drawn as the reference draws."""
        ranks = []
        for cl in range(self.n_classes):
            n_elements = int(counts[:, cl].sum()) if cl < counts.shape[1] else 0
            if n_elements > self.max_elements_per_batch:
                ranks.append(self.rng.choice(n_elements, self.max_elements_per_batch))
            elif n_elements > 0:
                ranks.append(np.arange(n_elements))
            else:
                ranks.append(None)
        return ranks

    def put(self, X: torch.Tensor, y: torch.Tensor):
        """Adds the embeddings of the voxels with ``y > 0`` to the queues, by class."""
        if X.is_cuda:
            y = y if y.dtype == torch.float32 else y.float()
            X = X if X.dtype == torch.float32 else X.float()
            for cl, rows in enumerate(ops.nn_queue_put(X, y, self._select)[:self.n_classes]):
                if rows is not None:
                    self.q[cl].put(rows)
            return
        X = X.flatten(start_dim=2)
        y = y.flatten(start_dim=2)
        b, c, v = torch.where(y > 0)
        for cl in range(self.n_classes):
            idx = c == cl
            elements = X[b[idx], :, v[idx]]
            n_elements = elements.shape[0]
            if n_elements > self.max_elements_per_batch:
                elements = elements[self.rng.choice(n_elements, self.max_elements_per_batch)]
            if n_elements > 0:
                self.q[cl].put(elements.detach())

    def get_from_class(self, n: int, cl: int) -> list[torch.Tensor]:
        """Up to ``n`` entries of the queue of class ``cl``, oldest first."""
        q = self.q[cl]
        n_elements = q.qsize()
        if n_elements == 0 or n <= 0:
            return []
        n = min(n, n_elements)
        return [q.get() for _ in self.rng.choice(n_elements, n)]

    def get(self, n: int, cl: int | None = None) -> torch.Tensor:
        """``n`` entries of class ``cl``, or of classes drawn at random when ``cl`` is None."""
        if cl is not None:
            output = self.get_from_class(n, cl)
        else:
            output = []
            sample = self.rng.choice(self.n_classes, size=n)
            un, count = np.unique(sample, return_counts=True)
            for c, cnt in zip(un, count):
                output.extend(self.get_from_class(cnt, c))
        if len(output) == 0:
            return torch.empty(0)
        return torch.cat(output, 0)

    def __len__(self) -> int:
        return sum([q.qsize() for q in self.q])

    def _past_samples(self):
        """(samples [Q, C] or None, their classes as a numpy int64 array): drains the queue."""
        n_samples = [np.minimum(self.n_samples_per_class, self.q[cl].qsize())
                     for cl in range(self.n_classes)]
        past_samples = [self.get(n, cl) for cl, n in zip(range(self.n_classes), n_samples)]
        non_empty = [(cl, ps) for cl, ps in enumerate(past_samples) if ps.shape[0] > 0]
        if len(non_empty) == 0:
            return None, None
        classes = np.concatenate([np.repeat(cl, ps.shape[0]) for cl, ps in non_empty], 0)
        return torch.cat([ps for _, ps in non_empty]), classes

    def get_past_samples(self, device="cuda") -> tuple[torch.Tensor, torch.Tensor]:
        """The same number of queue entries for every class and their one-hot labels (int64)."""
        past_samples, classes = self._past_samples()
        if past_samples is None:
            return torch.empty(0, device=device), torch.empty(0, self.n_classes, device=device)
        past_sample_labels = F.one_hot(torch.as_tensor(classes, device=device), self.n_classes)
        return past_samples, past_sample_labels

    def forward(self, X: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        past_samples, classes = self._past_samples()
        if past_samples is None:
            return torch.zeros([], device=X.device)
        past_class = torch.as_tensor(classes.astype(np.int32), device=X.device)
        return HF.nn_queue_loss(X, y, past_samples.to(X.device), past_class, self.temperature)


class PseudoLabelCrossEntropy(torch.nn.Module):
    """losses.py:447-477: the cross entropy between the logits ``pred`` and the pseudo-labels
    ``proba > threshold`` (strict) as probability targets. ``self.ce`` is a real
    ``torch.nn.CrossEntropyLoss(*args, **kwargs)``: its attributes and ``state_dict`` are the
    reference's, and it is what runs for CPU tensors and on the composed route."""

    def __init__(self, threshold: float, *args, **kwargs):
        super().__init__()
        self.threshold = threshold

        self.ce = torch.nn.CrossEntropyLoss(*args, **kwargs)

    def forward(self, pred: torch.Tensor, proba: torch.Tensor) -> torch.Tensor:
        ce = self.ce
        if not pred.is_cuda or pred.dim() < 2 or HF.semisl_route(
                "pseudo_label", K=pred.shape[1], reduction=ce.reduction,
                ignore_index=ce.ignore_index) == "composed":
            pseudo_y = proba > self.threshold
            return ce(pred, pseudo_y.float())
        return HF.pseudo_label_ce(pred, proba, self.threshold, ce.weight, ce.label_smoothing,
                                  ce.reduction)
