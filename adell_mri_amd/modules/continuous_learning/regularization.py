"""Elastic weight consolidation as the reference defines it
(adell_mri/modules/continuous_learning/regularization.py): the sum over the selected parameter
tensors of the p-norm of their distance to the weights the model started from. Here the whole term
-- however many tensors -- is three HIP launches over flat buffers (csrc/ewc.hip): per-chunk partial
sums, a one-block finalize, and one gradient launch.

Two routes:

* ``loss = loss + ewc(model)``: an ``autograd.Function`` (forward: partials + finalize; backward:
  one gradient launch that WRITES a fresh flat buffer, whose slices are the parameters' gradients);
* ``trainer.StepRunner(ewc=..., ewc_weight=...)``: ``add_to_optimizer`` ADDS the gradient straight
  into the flat gradient slots of a fused optimiser, one launch per parameter group, and autograd
  never sees the term.

On purpose unlike the reference: the result lives on the parameters' device (the reference starts from
a CPU ``torch.zeros([1])`` and fails on a GPU model); the anchor copy never receives a gradient; the
name -> anchor dict is ``anchor_parameters`` (the reference assigns it to ``self.named_parameters``,
which breaks ``.parameters()`` of the penalty and of every module that holds it); ``p`` must be a
finite number >= 1; CPU tensors raise (no eager-torch fallback)."""
import math
import numbers
from copy import deepcopy
from typing import List

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from ... import ops
from ..._lib import AdellHipError


def _chunk_rows(cols, num, chunk):
    """One row per ``chunk``-element piece of every tensor, without a Python loop. ``cols``: per-tensor
    int64 arrays; a column given as (array, stride) advances by ``stride`` per element of the piece's
    start (4 for byte addresses, 1 for element offsets). Returns (rows [R, len(cols) + 1] with the
    piece's element count as the LAST column, first row of every tensor [T + 1])."""
    k = (num + chunk - 1) // chunk
    first = np.concatenate([[0], np.cumsum(k)]).astype(np.int64)
    ix = np.repeat(np.arange(len(k)), k)
    start = (np.arange(int(k.sum()), dtype=np.int64) - first[:-1][ix]) * chunk
    out = []
    for col in cols:
        if isinstance(col, tuple):
            base, stride = col
            out.append(base[ix] + stride * start)
        else:
            out.append(col[ix])
    out.append(np.minimum(chunk, num[ix] - start))
    return np.stack(out, 1).astype(np.int64), first


class _Plan:
    """The device tables of one (parameter addresses, anchor buffer) state."""

    def __init__(self, owner, names, params):
        dev = owner._anchor.device
        for k, q in zip(names, params):
            ops._require_cuda(q)          # raises for CPU / non-fp32 tensors: there is no fallback
            a = owner.anchor_parameters[k]
            if q.device != dev:
                raise ValueError(f"ElasticWeightConsolidation: {k} is on {q.device}, its anchor on {dev}")
            if q.shape != a.shape:
                raise ValueError(f"ElasticWeightConsolidation: {k} has shape {tuple(q.shape)}, its "
                                 f"anchor {tuple(a.shape)}")
            if not q.is_contiguous():
                raise ValueError(f"ElasticWeightConsolidation: {k} is not contiguous")
        self.names, self.params = names, params
        self.keep = [q.detach() for q in params]      # the storages the table points into stay alive
        self.index = {id(q): i for i, q in enumerate(params)}
        self.tensors = len(params)
        self.num = np.array([q.numel() for q in params], dtype=np.int64)
        self.ptr = np.array([q.data_ptr() for q in params], dtype=np.int64)
        self.off = np.array([owner._anchor_offsets[k] for k in names], dtype=np.int64)
        self.anchor_ptr = owner._anchor.data_ptr() + 4 * self.off
        self.shapes = [q.shape for q in params]
        # the destination offsets of the forward table are the anchor's: the autograd route writes a
        # fresh buffer of the anchor's layout
        rows, first = self._rows(np.arange(self.tensors), self.off)
        self.chunks = rows.shape[0]
        self.table = torch.from_numpy(rows).to(dev)
        self.first = torch.from_numpy(first).to(dev)
        self.workspace = ops.ewc_workspace(self.chunks, self.tensors, dev)
        self.copy_table = None
        self.fused_key, self.fused = None, None

    def _rows(self, sel, dst_off):
        """Chunk rows (parameter, anchor, count, tensor index, destination offset) of the tensors
        ``sel`` with destination offsets ``dst_off``, and the first row of each."""
        sel = np.asarray(sel, dtype=np.int64)
        rows, first = _chunk_rows([(self.ptr[sel], 4), (self.anchor_ptr[sel], 4), sel,
                                   (np.asarray(dst_off, dtype=np.int64), 1)], self.num[sel],
                                  ops.ewc_chunk())
        return np.ascontiguousarray(rows[:, [0, 1, 4, 2, 3]]), first


class _EWCPenalty(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, plan, *params):
        norms, total = owner._evaluate(plan)
        ctx.owner, ctx.plan, ctx.epoch = owner, plan, owner._epoch
        # the backward pass reads the parameters again through the table: only the norms are saved, so
        # autograd's own check of saved tensors does not cover them
        ctx.versions = [q._version for q in params]
        ctx.save_for_backward(norms)
        return total

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        owner, plan = ctx.owner, ctx.plan
        if ctx.epoch != owner._epoch:
            raise RuntimeError("ElasticWeightConsolidation: the anchor was changed (consolidate / .to()) "
                               "between the forward and the backward pass")
        if ctx.versions != [q._version for q in plan.params]:
            raise RuntimeError("ElasticWeightConsolidation: a parameter was modified in place between the "
                               "forward and the backward pass of the penalty")
        (norms,) = ctx.saved_tensors
        gout = gout.to(torch.float32).contiguous()
        buf = torch.empty(owner._anchor.numel(), dtype=torch.float32, device=norms.device)
        ops.ewc_grad(plan.table, plan.chunks, owner.p, norms, 1.0, gout, False, buf)
        grads = [buf[o:o + n].view(s) if need else None
                 for o, n, s, need in zip(plan.off.tolist(), plan.num.tolist(), plan.shapes,
                                          ctx.needs_input_grad[2:])]
        return (None, None, *grads)


class ElasticWeightConsolidation(torch.nn.Module):
    """``ewc = ElasticWeightConsolidation(model, keys)``, then ``loss = loss + ewc(model)`` (or
    ``StepRunner(ewc=ewc)``).

    Args:
        model (torch.nn.Module): input model; ``self.model`` is a deep copy whose selected parameters
            live, with ``requires_grad=False``, in one flat 16-byte-slotted anchor buffer.
        keys (List[str], optional): names of the parameters which will be regularized. Defaults to
            None (all parameters).
        p (int, optional): order of the norm, a finite number >= 1. Defaults to 2.
    """

    def __init__(self, model: torch.nn.Module, keys: List[str] = None, p: int = 2):
        super().__init__()
        if (isinstance(p, bool) or not isinstance(p, numbers.Real) or not math.isfinite(p) or p < 1):
            raise NotImplementedError(f"ElasticWeightConsolidation: p must be a finite number >= 1, "
                                      f"got p={p!r}")
        self.model = deepcopy(model)
        self.keys = keys
        self.p = p
        if self.keys is None:
            self.keys = [k for k, _ in self.model.named_parameters()]
        self._epoch = 0
        self.table_rebuilds = 0
        self._rehome()

    # ---- the anchor --------------------------------------------------------------------------------
    def _rehome(self):
        """(Re)build the flat anchor buffer from the copy's selected parameters and point them at it."""
        named = dict(self.model.named_parameters())
        keys = set(self.keys)
        sel = [(k, q) for k, q in named.items() if k in keys]
        offsets, n = {}, 0
        for k, q in sel:
            if q.dtype != torch.float32 or q.device != sel[0][1].device:
                raise ValueError(f"ElasticWeightConsolidation: the selected parameters must be fp32 on "
                                 f"one device ({k}: {q.dtype} on {q.device})")
            offsets[k] = n
            n += (q.numel() + 3) // 4 * 4          # every slot 16-byte aligned
        dev = sel[0][1].device if sel else next((q.device for q in named.values()), torch.device("cpu"))
        flat = torch.zeros(n, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for k, q in sel:
                view = flat[offsets[k]:offsets[k] + q.numel()].view(q.shape)
                view.copy_(q.data)
                q.data = view
                q.requires_grad_(False)
        self.anchor_parameters = named
        self._anchor, self._anchor_offsets = flat, offsets
        self._plan, self._plan_key = None, None
        self._epoch += 1

    def _apply(self, fn, *args, **kwargs):
        # .to() / .cuda() / .float() replace every parameter's storage one by one
        out = super()._apply(fn, *args, **kwargs)
        self._rehome()
        return out

    def _plan_for(self, model):
        """The cached tables of ``model``'s selected parameters, rebuilt whenever one of their
        addresses has changed (building a fused optimiser re-homes ``p.data``). None: nothing to do."""
        keys, offsets = set(self.keys), self._anchor_offsets
        names, params = [], []
        for k, q in model.named_parameters():
            if k in keys:
                if k not in offsets:
                    raise ValueError(f"ElasticWeightConsolidation: {k} is selected but the anchor copy "
                                     "has no such parameter")
                if q.numel():
                    names.append(k)
                    params.append(q)
        if not params:
            return None
        key = (self._anchor.data_ptr(), self._epoch, tuple(q.data_ptr() for q in params))
        if key != self._plan_key:
            self._plan = _Plan(self, names, params)
            self._plan_key = key
            self.table_rebuilds += 1
        return self._plan

    # ---- value ------------------------------------------------------------------------------------
    def _evaluate(self, plan):
        dev = self._anchor.device
        norms = torch.empty(plan.tensors, dtype=torch.float32, device=dev)
        total = torch.empty(1, dtype=torch.float32, device=dev)
        ops.ewc_partials(plan.table, plan.chunks, self.p, plan.workspace)
        ops.ewc_finalize(plan.first, plan.tensors, plan.chunks, self.p, plan.workspace, norms, total)
        return norms, total

    def _empty(self, model):
        q = next(iter(model.parameters()), None)
        dev = self._anchor.device if q is None else q.device
        if dev.type != "cuda":
            raise AdellHipError("adell_mri_amd kernels run on MI355X only: got a CPU model (no CPU fallback)")
        return torch.zeros([1], dtype=torch.float32, device=dev)

    def forward(self, model):
        """The penalty as a ``[1]`` fp32 tensor on the parameters' device, differentiable once with
        respect to ``model``'s selected parameters. The backward pass takes ``param - anchor`` from the
        parameters as they are THEN: an in-place torch operation on a parameter between forward and
        backward raises (tensor version counters), a changed anchor raises; a write by a kernel of this
        library (a fused optimiser's step) does not move a version counter and is not noticed -- step
        after the backward pass, as every training loop does."""
        plan = self._plan_for(model)
        if plan is None:
            return self._empty(model)
        return _EWCPenalty.apply(self, plan, *plan.params)

    # ---- fused route --------------------------------------------------------------------------------
    @torch.no_grad()
    def add_to_optimizer(self, model, optimizer, weight=1.0):
        """Evaluate the penalty and ADD ``weight / group["grad_scale"]`` times its gradient into the
        flat gradient slots of the fused ``optimizer`` (one launch per parameter group that holds a
        selected parameter), so that the step applies ``weight * d penalty``. Call it once the task
        gradients are in their slots (after ``collect_grads()`` / the gradient exchange). A selected
        parameter without a task gradient gets ``.grad`` pointed at its slot and is stepped; one the
        optimiser does not hold, or that does not require grad (now: frozen after the optimiser was
        built included), contributes to the value only. Returns the ``[1]`` penalty (no gradient
        attached)."""
        plan = self._plan_for(model)
        if plan is None:
            return self._empty(model)
        norms, total = self._evaluate(plan)
        flats = optimizer.flat_groups
        key = (id(optimizer), tuple(f.grad.data_ptr() for f in flats),
               tuple(q.requires_grad for f in flats for q in f.params))
        if plan.fused_key != key:
            fused = []
            for gi, flat in enumerate(flats):
                idx = [i for i, q in enumerate(flat.params) if id(q) in plan.index and q.requires_grad]
                if not idx:
                    continue
                rows, _ = plan._rows([plan.index[id(flat.params[i])] for i in idx],
                                     [flat.offsets[i] for i in idx])
                fused.append((gi, flat, idx, torch.from_numpy(rows).to(flat.grad.device), rows.shape[0]))
            plan.fused_key, plan.fused = key, fused
        for gi, flat, idx, table, chunks in plan.fused:
            scale = float(optimizer.param_groups[gi].get("grad_scale", 1.0))
            ops.ewc_grad(table, chunks, self.p, norms, float(weight) / scale, None, True, flat.grad)
            for i in idx:
                q = flat.params[i]
                if q.grad is None:
                    q.grad = flat.slot(i)
            flat._has = None         # the mask of the last collect() no longer says who has a gradient
        return total

    # ---- next task --------------------------------------------------------------------------------
    @torch.no_grad()
    def consolidate(self, model):
        """Re-anchor at ``model``'s current weights (one multi-copy launch)."""
        from ...optim import FlatParameters

        plan = self._plan_for(model)
        if plan is None:
            return
        if plan.copy_table is None:
            rows, _ = _chunk_rows([(plan.ptr, 4), (plan.off, 1)], plan.num, FlatParameters.CHUNK)
            plan.copy_table = (torch.from_numpy(rows).to(self._anchor.device), rows.shape[0])
        ops.multi_copy(plan.copy_table[0], plan.copy_table[1], self._anchor)
        self._epoch += 1
        # the addresses are unchanged: the cached tables stay valid under the new epoch
        self._plan_key = (self._plan_key[0], self._epoch, self._plan_key[2])
