"""Minimal optimisation loop for the HIP path when Lightning is not installed:
the part of ``lightning.Trainer.fit`` the reference's training step relies on
(adell_mri/entrypoints/segmentation/train.py:799-819): zero_grad ->
training_step -> backward -> gradient exchange -> optimizer.step, with the
Trainer's ``gradient_clip_val`` and ``accumulate_grad_batches`` (train.py:807,811,
ssl/train_3d.py:354-355); ``validate_steps`` / ``test_steps`` are the part of
``Trainer.validate`` / ``Trainer.test`` the reference uses (train.py:819-830)."""
import itertools
import os

from .parallel import (GradSync, _has_sync_bn, convert_sync_batchnorm, sync_bn_communicates,
                       sync_bn_group)

# ADELL_GRAD_COLLECT=0: keep p.grad as views of the flat buffer (autograd accumulates into them)
_SET_TO_NONE = os.environ.get("ADELL_GRAD_COLLECT", "1") != "0"


def _offsets_drawn():
    """The next dropout offset an eager step would draw (functional._dropout_counter, left as found)."""
    from . import functional as HF

    v = next(HF._dropout_counter)
    HF._dropout_counter = itertools.count(v)
    return v


class StepRunner:
    """One training step per ``train_step(batch)``, with Lightning's meaning of

    * ``gradient_clip_val`` (None / 0: off): ``clip_grad_norm_(gradient_clip_val, 2.0)`` of the fused
      optimiser between the gradient exchange and ``optimizer.step()``; the norm is that of the
      gradient the optimiser applies. ``gradient_clip_algorithm="value"`` is not supported (the
      reference never sets it);
    * ``accumulate_grad_batches`` N: ``train_step`` runs ONE micro-batch. Micro-batches 1..N-1 run
      backward without exchanging anything (``GradSync.no_sync``) and fold their gradients into
      the flat buffers; the N-th runs backward, the exchange, clipping and the step with 1/N folded
      into the optimiser's ``grad_scale`` (Lightning divides the loss instead: same update).
      ``flush()`` steps a partial window (end of an epoch) with the same 1/N;
    * ``sync_batchnorm``: ``parallel.convert_sync_batchnorm(module)`` before the parameters are
      broadcast -- batch statistics over the items of all ranks (one all-reduce per batch-norm site
      and direction, on a process group of their own). A no-op in effect at world size 1. A module
      that already holds ``torch.nn.SyncBatchNorm`` modules (torch's converter) is synchronised either
      way; its batch-norm group is created here.

    * ``spectral_norm`` (None: off): an int ``n`` stands for ``utils.pl_callbacks.SpectralNorm(
      n_power_iterations=n)`` (the entry points' ``--spectral_norm_power_iterations``), a
      ``SpectralNorm`` instance is used as given. Its ``setup(None, module, "fit")`` runs BEFORE
      ``configure_optimizers()``, so that the ``parametrizations.<name>.original`` parameters are the
      ones the optimiser's flat buffers hold; an explicit ``optimizer`` that still holds a replaced
      plain weight is refused.

    * ``ewc`` (None: off): a ``modules.continuous_learning.ElasticWeightConsolidation`` over
      ``module``; every optimiser step applies ``ewc_weight * d penalty`` on top of the task gradient
      without autograd seeing the term. After the gradient exchange and before clipping the penalty is
      evaluated and its gradient ADDED into the optimiser's flat gradient slots, scaled by
      ``ewc_weight / grad_scale`` as in force at that moment (one launch per parameter group), so the
      amount applied does not depend on the world size or on ``accumulate_grad_batches``. For full
      accumulation windows that is what ``loss + ewc_weight * ewc(module)`` in every micro-batch gives
      (the parameters do not move inside a window); ``flush()`` of a partial window applies the same
      ``ewc_weight * d penalty``, where the loss route would apply it scaled by the window's share.
      Clipping sees task plus penalty gradient. ``train_step`` returns
      ``loss + ewc_weight * penalty`` for the micro-batch that steps (a device-side add; the other
      micro-batches of a window return the plain loss) and ``last_ewc_penalty`` holds the ``[1]``
      penalty.

    ``step_idx`` counts micro-batches (the ``batch_idx`` of ``training_step``), ``optimizer_steps``
    the optimiser steps, ``last_grad_norm`` is the device tensor of the last clip. ``current_epoch``,
    ``callback_metrics`` and ``should_stop`` are plain attributes kept by whoever owns the epoch loop:
    with them a StepRunner is the ``trainer`` of ``MultiPhaseTraining.on_validation_epoch_end``."""

    def __init__(self, module, optimizer=None, sync=None, gradient_clip_val=None,
                 gradient_clip_algorithm="norm", accumulate_grad_batches=1, sync_batchnorm=False,
                 spectral_norm=None, ewc=None, ewc_weight=1.0):
        if gradient_clip_val is not None and float(gradient_clip_val) < 0:
            raise ValueError(f"gradient_clip_val should be >= 0, got {gradient_clip_val}")
        if gradient_clip_algorithm == "value":
            raise NotImplementedError("StepRunner: gradient_clip_algorithm='value' is not supported "
                                      "(the reference clips by norm)")
        if gradient_clip_algorithm != "norm":
            raise ValueError(f"gradient_clip_algorithm must be 'norm', got {gradient_clip_algorithm!r}")
        if int(accumulate_grad_batches) != accumulate_grad_batches or accumulate_grad_batches < 1:
            raise ValueError(f"accumulate_grad_batches should be an integer >= 1, got "
                             f"{accumulate_grad_batches}")
        if not isinstance(sync_batchnorm, bool):
            raise TypeError(f"sync_batchnorm must be a bool, got {sync_batchnorm!r}")
        self.gradient_clip_val = float(gradient_clip_val) if gradient_clip_val else None
        self.accumulate_grad_batches = int(accumulate_grad_batches)
        if sync_batchnorm:
            # (in place below the root: every batch norm of these modules is a child of something)
            converted = convert_sync_batchnorm(module)
            if converted is not module:
                raise TypeError("StepRunner(sync_batchnorm=True): the module itself is a batch norm; "
                                "convert it with parallel.convert_sync_batchnorm and pass the result")
        elif _has_sync_bn(module):
            sync_bn_group()      # collective: the dedicated batch-norm group, on every rank here
        self.sync_batchnorm = sync_batchnorm
        self.spectral_norm = _apply_spectral_norm(module, spectral_norm, optimizer)
        self.module = module
        if optimizer is None:
            # a dict with "optimizer", or the bare optimiser (ViTMaskedAutoEncoderPL without warm-up)
            optimizer = module.configure_optimizers()
            if isinstance(optimizer, dict):
                optimizer = optimizer["optimizer"]
        self.optimizer = optimizer
        if (self.gradient_clip_val or self.accumulate_grad_batches > 1) and not (
                hasattr(optimizer, "clip_grad_norm_") and hasattr(optimizer, "fold_grads")):
            raise TypeError("StepRunner: gradient clipping / accumulation need a fused optimiser "
                            "(adell_mri_amd.optim)")
        self.ewc, self.ewc_weight = _check_ewc(module, optimizer, ewc), float(ewc_weight)
        self.last_ewc_penalty = None
        self.sync = sync if sync is not None else GradSync(optimizer)
        self.sync.broadcast_parameters(module=module)
        self.step_idx = 0
        self.optimizer_steps = 0
        self.last_grad_norm = None
        # the epoch loop's state, as a Lightning Trainer names it (MultiPhaseTraining reads and sets it)
        self.current_epoch = 0
        self.callback_metrics = {}
        self.should_stop = False
        self._micro = 0                  # micro-batches of the current accumulation window so far
        self._graph = None

    def reserve_memory(self, main_bytes=None, side_bytes=None):
        """Pre-size the caching allocator's pools after the first steps of a workload: one large
        block is allocated and released again on the training stream and on the weight-gradient
        stream (functional.side_run), so that later steps split cached memory instead of asking
        the driver for more. A fresh device allocation inside a step is cleared by the driver at
        ~65 GB/s on some boxes (4-7 GB of pool growth = a 60-110 ms stall in one step, round 3's
        driver record); with 288 GB of HBM per GPU the head-room is free. Defaults: half of what
        is reserved now (>= 4 GiB) for the main pool, a quarter (>= 2 GiB) for the side pool.
        Returns (main_bytes, side_bytes)."""
        import torch

        from . import functional as HF

        dev = next(self.module.parameters()).device
        if dev.type != "cuda":
            return 0, 0
        reserved = torch.cuda.memory_stats(dev).get("reserved_bytes.all.current", 0)
        free, _ = torch.cuda.mem_get_info(dev)
        if main_bytes is None:
            main_bytes = max(4 << 30, reserved // 2)
        if side_bytes is None:
            side_bytes = max(2 << 30, reserved // 4)
        # never more than half of what the device still has free
        main_bytes = int(min(main_bytes, free // 2))
        side_bytes = int(min(side_bytes, max(0, free // 2 - main_bytes)))
        if main_bytes > 0:
            t = torch.empty(main_bytes, dtype=torch.uint8, device=dev)
            del t
        side = HF._SIDE["stream"]
        if side is not None and side.device == dev and side_bytes > 0:
            with torch.cuda.stream(side):
                t = torch.empty(side_bytes, dtype=torch.uint8, device=dev)
                del t
        else:
            side_bytes = 0
        return main_bytes, side_bytes

    # ---- one captured HIP graph per step ------------------------------------------------------------
    def enable_graph(self, batch, warmup=3):
        """Capture zero_grad -> training_step -> backward -> gradient gather of ONE step in a HIP
        graph (torch.cuda.CUDAGraph) and replay it from then on: the ~800 launches of a UNETR /
        ConvNeXt step cost the host nothing (the reference's loop is host-paced the same way:
        Lightning over eager torch ops, train.py:799-819). What stays outside the graph, eager, is
        what carries host-side scalars: the gradient exchange and ``optimizer.step()`` (learning
        rate, step counts) -- a handful of launches.

        * ``batch`` gives the shapes: its tensors become the static inputs (``train_step`` copies a
          different batch into them);
        * ``warmup`` eager steps run first on the capture stream (allocator pools, packed weights,
          launch plans);
        * dropout: the (seed, offset) words of the kernels are frozen in the graph; the graph's last
          node advances the library's replay counter by the number of offsets a step draws
          (ops.rng_advance), so replay r draws the masks eager step r would have drawn -- losses are
          bit-identical to the eager loop (tests/test_graph_step_gpu.py);
        * data-parallel runs: the bucketed all-reduce is issued from backward hooks, which a replay
          does not run -- refused unless the exchange is the single all-reduce after backward.
        Returns the static loss tensor (updated in place by every replay)."""
        import torch

        from . import functional as HF
        from . import ops

        if self.accumulate_grad_batches > 1:
            raise RuntimeError("StepRunner.enable_graph: one graph is one whole step; with "
                               "accumulate_grad_batches > 1 a step is several micro-batches -- "
                               "run them eagerly")
        if self.sync.overlap:
            raise RuntimeError("StepRunner.enable_graph: gradient buckets are sent from backward hooks "
                               "(GradSync(overlap=True)); build GradSync(optimizer, overlap=False)")
        if sync_bn_communicates(self.module):
            raise RuntimeError("StepRunner.enable_graph: synchronised batch norm all-reduces its "
                               "statistics inside the step (world size > 1); collectives are not "
                               "captured in a HIP graph -- run eager steps")
        if getattr(self.module, "ema", None) is not None:
            raise RuntimeError("StepRunner.enable_graph: the module's EMA update takes its decay from a "
                               "host-side schedule inside training_step; a replay would freeze it")
        if getattr(self.module, "compute_train_metrics", False):
            raise RuntimeError("StepRunner.enable_graph: compute_train_metrics is on; metrics are not "
                               "captured in a HIP graph -- set module.compute_train_metrics = False "
                               "or run eager steps")
        if warmup < 1:
            raise ValueError("StepRunner.enable_graph: at least one warm-up step (it leaves the packed "
                             "weight tables, staging rings and launch plans the capture may not build)")
        import gc
        gc.collect()      # dead modules leave the weight-pack registry NOW, not inside the capture
        dev = next(self.module.parameters()).device
        self._static = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in batch.items()}
        stream = torch.cuda.Stream(dev)
        stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(stream):
            for _ in range(warmup):
                self._eager_step(self._static)
        torch.cuda.current_stream(dev).wait_stream(stream)
        torch.cuda.synchronize(dev)
        c0 = _offsets_drawn()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            self.optimizer.zero_grad(set_to_none=_SET_TO_NONE)
            loss = self.module.training_step(self._static, self.step_idx)
            loss.backward()
            collect = getattr(self.optimizer, "collect_grads", None)
            if collect is not None:
                collect()
            drawn = _offsets_drawn() - c0                   # offsets one step draws
            if drawn > 0:
                ops.rng_advance(drawn)                      # last node: the next replay's masks
        HF._dropout_counter = itertools.count(c0)           # the capture executed nothing
        self._graph, self._graph_loss, self._graph_draws = graph, loss, drawn
        return loss

    def disable_graph(self):
        """Back to eager steps (the replay counter returns to zero: eager offsets are absolute)."""
        from . import ops

        if getattr(self, "_graph", None) is not None:
            ops.rng_advance(0, set_value=True)
            # the replays advanced the device word by step * draws: the eager counter takes over there
        self._graph = None

    def _eager_step(self, batch):
        if self.accumulate_grad_batches > 1:
            return self._micro_step(batch)
        self.optimizer.zero_grad(set_to_none=_SET_TO_NONE)
        loss = self.module.training_step(batch, self.step_idx)
        loss.backward()
        self._exchange_and_step()
        self.step_idx += 1
        return self._with_penalty(loss)

    def _micro_step(self, batch):
        if self._micro == 0:
            self.optimizer.zero_grad(set_to_none=_SET_TO_NONE)
        loss = self.module.training_step(batch, self.step_idx)
        self._micro += 1
        if self._micro < self.accumulate_grad_batches:
            with self.sync.no_sync():
                loss.backward()
            self.optimizer.fold_grads()
        else:
            loss.backward()
            self._exchange_and_step()
            loss = self._with_penalty(loss)
        self.step_idx += 1
        return loss

    def _with_penalty(self, loss):
        """``loss + ewc_weight * penalty`` of the step just taken (the loss itself without ``ewc``)."""
        if self.ewc is None:
            return loss
        return loss.detach() + (self.ewc_weight * self.last_ewc_penalty).reshape(loss.shape)

    def _add_penalty(self):
        """The penalty's gradient into the flat gradient slots, under the grad_scale now in force."""
        self.last_ewc_penalty = self.ewc.add_to_optimizer(self.module, self.optimizer, self.ewc_weight)

    def _exchange_and_step(self):
        """all-reduce -> penalty gradient -> clip -> step of the current window (1/N folded into
        grad_scale)."""
        self.sync.all_reduce()
        n = self.accumulate_grad_batches
        if n == 1 and not self.gradient_clip_val:
            if self.ewc is not None:
                self._add_penalty()
            self.optimizer.step()
        else:
            groups = self.optimizer.param_groups
            kept = [g.get("grad_scale", 1.0) for g in groups]
            try:
                for g, s in zip(groups, kept):
                    g["grad_scale"] = s / n
                if self.ewc is not None:
                    self._add_penalty()
                if self.gradient_clip_val:
                    self.last_grad_norm = self.optimizer.clip_grad_norm_(self.gradient_clip_val, 2.0)
                self.optimizer.step()
            finally:
                for g, s in zip(groups, kept):    # world-size state (optim.load_state_dict)
                    g["grad_scale"] = s
        self.optimizer_steps += 1
        self._micro = 0

    def flush(self):
        """Step the micro-batches of an unfinished accumulation window (Lightning does at the end
        of an epoch), with the same 1/accumulate_grad_batches. Returns whether it stepped."""
        if self._micro == 0:
            return False
        self._exchange_and_step()
        return True

    def train_step(self, batch):
        if getattr(self, "_graph", None) is None:
            return self._eager_step(batch)
        import torch

        from . import functional as HF

        for k, v in batch.items():
            st = self._static.get(k)
            if torch.is_tensor(v) and v is not st and v.data_ptr() != st.data_ptr():
                st.copy_(v, non_blocking=True)
        self._graph.replay()
        if self._graph_draws:
            # the host counter stays where an eager loop would be (disable_graph continues there)
            HF._dropout_counter = itertools.count(_offsets_drawn() + self._graph_draws)
        self._exchange_and_step()
        self.step_idx += 1
        return self._with_penalty(self._graph_loss)


def _apply_spectral_norm(module, spectral_norm, optimizer):
    """The ``SpectralNorm`` callback of a ``spectral_norm`` argument (None: nothing), set up on
    ``module``; raises for an optimiser built over the plain weights it has replaced."""
    if spectral_norm is None:
        return None
    from .utils.pl_callbacks import SpectralNorm

    if isinstance(spectral_norm, bool) or not isinstance(spectral_norm, (int, SpectralNorm)):
        raise TypeError(f"spectral_norm must be None, a number of power iterations or a SpectralNorm "
                        f"callback, got {spectral_norm!r}")
    callback = spectral_norm if isinstance(spectral_norm, SpectralNorm) \
        else SpectralNorm(n_power_iterations=spectral_norm)
    callback.setup(None, module, "fit")
    if optimizer is not None:
        live = {id(p) for p in module.parameters()}
        stale = [p for g in optimizer.param_groups for p in g["params"] if id(p) not in live]
        if stale:
            raise ValueError(f"StepRunner(spectral_norm=...): the optimiser holds {len(stale)} parameters "
                             "that are no longer the module's: spectral normalisation replaced the "
                             "plain weights by parametrizations.<name>.original -- build the optimiser "
                             "after the callback's setup, or leave optimizer=None")
    return callback


def _check_ewc(module, optimizer, ewc):
    """``ewc`` as given (None: off), refused unless it is a penalty over ``module``'s parameters and
    the optimiser keeps flat gradient slots."""
    if ewc is None:
        return None
    from .modules.continuous_learning import ElasticWeightConsolidation

    if not isinstance(ewc, ElasticWeightConsolidation):
        raise TypeError(f"StepRunner: ewc must be an ElasticWeightConsolidation, got {type(ewc).__name__}")
    if not hasattr(optimizer, "flat_groups"):
        raise TypeError("StepRunner(ewc=...): the fused route needs a fused optimiser "
                        "(adell_mri_amd.optim); add ewc(module) to the loss instead")
    own = {k: p.shape for k, p in module.named_parameters()}
    keys = set(ewc.keys)
    selected = [k for k in ewc.anchor_parameters if k in keys]
    wrong = [k for k in selected if k not in own or own[k] != ewc.anchor_parameters[k].shape]
    if wrong or not selected:
        raise ValueError(f"StepRunner(ewc=...): the penalty's selected parameters are not the module's "
                         f"({len(wrong)} of {len(selected)} missing or of another shape, e.g. "
                         f"{wrong[:3]}): build it with ElasticWeightConsolidation(module, ...)")
    return ewc


def fit_steps(module, batches, optimizer=None, gradient_clip_val=None, accumulate_grad_batches=1,
              sync_batchnorm=False, spectral_norm=None, ewc=None, ewc_weight=1.0):
    runner = StepRunner(module, optimizer, gradient_clip_val=gradient_clip_val,
                        accumulate_grad_batches=accumulate_grad_batches,
                        sync_batchnorm=sync_batchnorm, spectral_norm=spectral_norm, ewc=ewc,
                        ewc_weight=ewc_weight)
    module.train()
    losses = [runner.train_step(b).detach() for b in batches]
    runner.flush()
    return losses


def _batch_size(module, batch):
    """Items in a batch: those of the image (``image_key`` / the first ``image_keys`` entry, inside
    a semi-supervised batch's "supervised" part), else of its first tensor."""
    import torch

    if isinstance(batch, dict) and "supervised" in batch:
        batch = batch["supervised"]
    key = getattr(module, "image_key", None) or (getattr(module, "image_keys", None) or [None])[0]
    if isinstance(batch, dict) and key in batch and torch.is_tensor(batch[key]):
        return int(batch[key].shape[0])
    stack = [batch]
    while stack:
        b = stack.pop(0)
        if torch.is_tensor(b):
            return int(b.shape[0])
        if isinstance(b, dict):
            stack.extend(b.values())
        elif isinstance(b, (list, tuple)):
            stack.extend(b)
    return 1


def _evaluate(module, batches, step_name, loss_key, metrics_attr):
    import torch
    import torch.distributed as dist

    from .metrics import bad_target_message

    metrics = getattr(module, metrics_attr, None) or {}
    picai = module.picai_accumulator() if hasattr(module, "picai_accumulator") else None
    if picai is not None:
        picai.reset()
    was_training = module.training
    module.eval()
    try:
        with torch.no_grad():
            total, count = None, 0
            for i, batch in enumerate(batches):
                loss = getattr(module, step_name)(batch, i)
                if isinstance(loss, tuple):       # a classification test_step: (loss, prediction)
                    loss = loss[0]
                loss = loss.detach().double().reshape(())
                bs = _batch_size(module, batch)
                total = loss * bs if total is None else total + loss * bs
                count += bs
            if total is None:
                raise ValueError(f"{step_name}s: no batches")
            mean = total / count
            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                dist.all_reduce(mean)             # Lightning's sync_dist: the mean over ranks
                mean = mean / dist.get_world_size()
            values, flags = [mean], []
            for m in metrics.values():
                v, bad = m.compute_async()
                values.append(v.double())
                flags.append(bad.double())
            host = torch.stack(values + flags).cpu().tolist()    # the one host synchronisation
        keys = list(metrics.keys())
        for k, bad in zip(keys, host[1 + len(keys):]):
            if bad > 0:
                own = getattr(metrics[k], "bad_target_message", None)
                raise RuntimeError(f"{k}: " + (own() if own is not None
                                               else bad_target_message(metrics[k].num_classes)))
        out = {loss_key: host[0]}
        out.update(zip(keys, host[1:1 + len(keys)]))
        if picai is not None and len(picai):
            # pl.py:609-652: the test epoch logs the same V_ keys (sic); mean over ranks
            lesion = picai.compute()
            out.update({"V_AP": lesion["AP"], "V_R": lesion["R"], "V_AUC": lesion["AUC"]})
        return out
    finally:
        for m in metrics.values():
            m.reset()
        if picai is not None:
            picai.reset()
        module.train(was_training)


def validate_steps(module, batches):
    """``validation_step`` over ``batches`` in eval mode without autograd, then
    ``{"val_loss": batch-size-weighted mean of the step losses (averaged over ranks), "V_IoU": ...,
    ...}`` from ``module.val_metrics``, which are reset. One host synchronisation, at the end; with
    ``picai_eval``, also one per micro-batch (the sizes of its lesion tables), and ``"V_AP"``,
    ``"V_R"`` and ``"V_AUC"`` of the PI-CAI evaluation (averaged over ranks)."""
    return _evaluate(module, batches, "validation_step", "val_loss", "val_metrics")


def test_steps(module, batches):
    """``test_step`` over ``batches``: ``{"test_loss": ..., "T_IoU": ..., ...}`` from
    ``module.test_metrics``, as ``validate_steps``."""
    return _evaluate(module, batches, "test_step", "test_loss", "test_metrics")


test_steps.__test__ = False     # a loop, not a pytest test, wherever it is imported
