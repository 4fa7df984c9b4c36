"""Continual learning without a GPU: the penalty's construction and refusals, the library's argument
checks, parameter groups and early stopping against the reference fixture, and the phase callback."""
import ctypes
import json
import math
import types

import numpy as np
import pytest
import torch

import continual_cases as C
from adell_mri_amd import _lib, ops
from adell_mri_amd.modules.continuous_learning import (EarlyStopper, ElasticWeightConsolidation,
                                                       MultiPhaseTraining, create_param_groups)


@pytest.fixture(scope="module")
def gold():
    return np.load(C.GOLD)


# ---- ElasticWeightConsolidation --------------------------------------------------------------------
def test_constructor_and_attributes():
    model = C.Named(C.anchors())
    ewc = ElasticWeightConsolidation(model)
    assert ewc.keys == list(C.SHAPES) and ewc.p == 2
    assert ewc.model is not model
    assert list(ewc.state_dict()) == ["model." + k for k in C.SHAPES]
    assert list(ewc.anchor_parameters) == list(C.SHAPES)
    for k, q in model.named_parameters():
        a = ewc.anchor_parameters[k]
        assert torch.equal(a, q) and a.data_ptr() != q.data_ptr()
        assert not a.requires_grad and q.requires_grad
        assert a.data_ptr() % 16 == 0                      # one flat 16-byte-slotted buffer
    sub = ElasticWeightConsolidation(model, keys=["vector.bias"], p=1.5)
    assert sub.keys == ["vector.bias"] and sub.p == 1.5
    assert sub.anchor_parameters["matrix.weight"].requires_grad      # not selected: left as copied
    assert not sub.anchor_parameters["vector.bias"].requires_grad


def test_state_dict_round_trip_reaches_the_flat_anchor():
    ewc = ElasticWeightConsolidation(C.Named(C.anchors()))
    other = {"model." + k: torch.from_numpy(v) + 1.0 for k, v in C.anchors().items()}
    ewc.load_state_dict(other)
    for k in C.SHAPES:
        o = ewc._anchor_offsets[k]
        flat = ewc._anchor[o:o + other["model." + k].numel()]
        assert torch.equal(flat, other["model." + k].reshape(-1))


def test_parameters_work_on_the_penalty_and_on_a_module_holding_it():
    ewc = ElasticWeightConsolidation(C.Named(C.anchors()))
    assert len(list(ewc.parameters())) == len(C.SHAPES)
    assert [k for k, _ in ewc.named_parameters()] == ["model." + k for k in C.SHAPES]

    class Holder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.net = torch.nn.Linear(2, 2)
            self.ewc = ElasticWeightConsolidation(self.net)

    assert len(list(Holder().parameters())) == 4


@pytest.mark.parametrize("p", [0, 0.5, -1, math.inf, -math.inf, math.nan, "fro", None, True])
def test_invalid_p_raises_naming_p(p):
    with pytest.raises(NotImplementedError, match=r"\bp\b"):
        ElasticWeightConsolidation(C.Named(C.anchors()), p=p)


def test_cpu_model_fails_loudly():
    model = C.Named(C.state("moved"))
    ewc = ElasticWeightConsolidation(C.Named(C.anchors()))
    with pytest.raises(_lib.AdellHipError, match="CPU"):
        ewc(model)
    with pytest.raises(_lib.AdellHipError, match="CPU"):
        ewc.consolidate(model)


# ---- the library ------------------------------------------------------------------------------------
def test_chunk_query_and_workspace():
    h = _lib.lib()
    chunk = h.adell_ewc_chunk()
    assert chunk > 0 and chunk % 4 == 0 and ops.ewc_chunk() == chunk
    assert h.adell_ewc_workspace_doubles(7, 3) >= 10
    assert h.adell_ewc_workspace_doubles(0, 1) == 0 and h.adell_ewc_workspace_doubles(3, 0) == 0


def test_library_refuses_bad_arguments_before_a_launch():
    h = _lib.lib()
    buf = (ctypes.c_double * 64)()                 # never dereferenced: the calls fail before a launch
    q = ctypes.cast(buf, ctypes.c_void_p)
    bad_p = [0.5, 0.0, -2.0, math.inf, -math.inf, math.nan]
    assert h.adell_ewc_partials(None, 1, 2.0, q, None) == _lib.E_BADARG
    assert h.adell_ewc_partials(q, 0, 2.0, q, None) == _lib.E_BADARG
    assert h.adell_ewc_partials(q, 1, 2.0, None, None) == _lib.E_BADARG
    assert h.adell_ewc_finalize(None, 1, 1, 2.0, q, q, q, None) == _lib.E_BADARG
    assert h.adell_ewc_finalize(q, 0, 1, 2.0, q, q, q, None) == _lib.E_BADARG
    assert h.adell_ewc_finalize(q, 1, 0, 2.0, q, q, q, None) == _lib.E_BADARG
    assert h.adell_ewc_finalize(q, 1, 1, 2.0, q, None, q, None) == _lib.E_BADARG
    assert h.adell_ewc_grad(None, 1, 2.0, q, 1.0, None, 0, q, None) == _lib.E_BADARG
    assert h.adell_ewc_grad(q, 0, 2.0, q, 1.0, None, 1, q, None) == _lib.E_BADARG
    assert h.adell_ewc_grad(q, 1, 2.0, q, 1.0, None, 0, None, None) == _lib.E_BADARG
    for p in bad_p:
        assert h.adell_ewc_partials(q, 1, p, q, None) == _lib.E_BADARG, p
        assert b"p must be" in h.adell_last_error()
        assert h.adell_ewc_finalize(q, 1, 1, p, q, q, q, None) == _lib.E_BADARG, p
        assert h.adell_ewc_grad(q, 1, p, q, 1.0, None, 0, q, None) == _lib.E_BADARG, p
    with pytest.raises(_lib.AdellHipError):
        _lib.check(h.adell_ewc_partials(q, 1, 0.5, q, None))


# ---- create_param_groups / EarlyStopper --------------------------------------------------------------
@pytest.mark.parametrize("case", list(C.GROUP_CASES))
@pytest.mark.parametrize("leftovers", [True, False])
def test_param_groups_match_the_reference(gold, case, leftovers):
    model = C.group_model()
    names = {id(q): k for k, q in model.named_parameters()}
    groups = create_param_groups(model, C.GROUP_CASES[case], include_leftovers=leftovers)
    got = [[names[id(q)] for q in g["params"]] for g in groups]
    assert got == json.loads(str(gold[f"groups:{case}:{int(leftovers)}"]))
    assert all(list(g) == ["params"] for g in groups)


def test_param_groups_settings_and_length_assertion():
    model = C.group_model()
    groups = create_param_groups(model, ["0.", "3."], [{"lr": 0.1}, {"lr": 0.2, "weight_decay": 0.0}])
    assert groups[0]["lr"] == 0.1 and groups[1] == {"params": groups[1]["params"], "lr": 0.2,
                                                    "weight_decay": 0.0}
    assert len(groups) == 3 and list(groups[2]) == ["params"]
    torch.optim.SGD(groups, lr=1.0)                               # what torch takes as ``params``
    with pytest.raises(AssertionError, match="len\\(kwargs_groups\\)"):
        create_param_groups(model, ["0.", "3."], [{"lr": 0.1}])


@pytest.mark.parametrize("tag", list(C.STOPPERS))
def test_early_stopper_matches_the_reference(gold, tag):
    patience, min_delta = C.STOPPERS[tag]
    want = gold["stop:" + tag].tolist()
    for wrap in (float, torch.tensor, lambda v: torch.tensor([v], dtype=torch.float64)):
        stopper = EarlyStopper(patience, min_delta)
        assert [stopper(wrap(v)) for v in C.LOSSES] == want
    assert any(want)


# ---- MultiPhaseTraining --------------------------------------------------------------------------------
def _trainer_and_optimizer():
    model = C.group_model()
    opt = torch.optim.SGD(create_param_groups(model, [["0.weight", "0.bias"], "2."]), lr=1.0)
    return types.SimpleNamespace(current_epoch=0, callback_metrics={}, should_stop=False, optimizer=opt), opt


def _lrs(opt):
    return [g["lr"] for g in opt.param_groups]


def test_phase_assertions():
    with pytest.raises(AssertionError, match="same as len"):
        MultiPhaseTraining([[0.1]], [1, 2])
    with pytest.raises(AssertionError, match="integers or 'adaptive'"):
        MultiPhaseTraining([[0.1]], ["soon"])
    with pytest.raises(AssertionError, match="integers or 'adaptive'"):
        MultiPhaseTraining([[0.1]], [1.5])
    with pytest.raises(AssertionError, match="lists of floats or 'stop'"):
        MultiPhaseTraining([0.1], [1])
    with pytest.raises(AssertionError, match="lists of floats or 'stop'"):
        MultiPhaseTraining(["halt"], [1])


def test_integer_phases_switch_at_their_epochs_and_stop():
    trainer, opt = _trainer_and_optimizer()
    cb = MultiPhaseTraining([[1.0, 1.0, 1.0], [0.5, 0.25, 0.125], [0.01, 0.02, 0.03], "stop"],
                            [2, 4, 5, 99])
    seen = []
    for epoch in range(8):
        trainer.current_epoch = epoch
        cb.on_validation_epoch_end(trainer, None)
        seen.append((cb.idx, _lrs(opt), trainer.should_stop))
    assert seen[0] == seen[1] == (0, [1.0, 1.0, 1.0], False)
    assert seen[2] == seen[3] == (1, [0.5, 0.25, 0.125], False)
    assert seen[4] == (2, [0.01, 0.02, 0.03], False)
    # "stop" leaves the learning rates alone; afterwards the list is exhausted: nothing happens
    assert seen[5] == seen[6] == seen[7] == (3, [0.01, 0.02, 0.03], True)


def test_exhausted_list_is_a_no_op():
    trainer, opt = _trainer_and_optimizer()
    cb = MultiPhaseTraining([[1.0, 1.0, 1.0], [0.5, 0.5, 0.5]], [0, 0])
    for epoch in range(4):       # the reference would raise IndexError at the second call
        trainer.current_epoch = epoch
        cb.on_validation_epoch_end(trainer, None)
    assert cb.idx == 1 and _lrs(opt) == [0.5, 0.5, 0.5] and not trainer.should_stop


def test_adaptive_phases_use_a_fresh_stopper_each():
    trainer, opt = _trainer_and_optimizer()
    del trainer.optimizer                       # then the optimiser comes from pl_module.optimizers()
    module = types.SimpleNamespace(optimizers=lambda: opt)
    cb = MultiPhaseTraining([[1.0, 1.0, 1.0], [0.1, 0.1, 0.1], "stop"], ["adaptive", "adaptive", 0],
                            monitor="val_loss", patience=2, min_delta=0.0)
    idx = []
    # phase 0: best 1.0, then two non-improving epochs -> switch at the third call; phase 1 must start
    # from a fresh stopper: 3.0 is its first (best) loss although it is worse than everything before
    for loss in [1.0, 2.0, 2.0, 3.0, 2.5, 4.0, 4.0, 0.0]:
        trainer.callback_metrics = {"val_loss": torch.tensor(loss)}
        cb.on_validation_epoch_end(trainer, module)
        idx.append((cb.idx, _lrs(opt)[0], trainer.should_stop))
    assert idx == [(0, 1.0, False), (0, 1.0, False), (1, 0.1, False), (1, 0.1, False), (1, 0.1, False),
                   (1, 0.1, False), (2, 0.1, True), (2, 0.1, True)]
    assert cb.checker.counter == 0 and cb.checker.min_validation_loss == math.inf
    with pytest.raises(KeyError, match="val_loss"):
        trainer.callback_metrics = {}
        MultiPhaseTraining([[1.0], [0.1]], ["adaptive", 1], monitor="val_loss").on_validation_epoch_end(
            trainer, module)


def test_step_runner_has_the_trainer_attributes():
    import inspect

    from adell_mri_amd.trainer import StepRunner, fit_steps

    sig = inspect.signature(StepRunner.__init__).parameters
    assert sig["ewc"].default is None and sig["ewc_weight"].default == 1.0
    assert {"ewc", "ewc_weight"} <= set(inspect.signature(fit_steps).parameters)
    # a StepRunner is the ``trainer`` of the phase callback
    module = torch.nn.Linear(2, 2)
    opt = torch.optim.SGD(module.parameters(), lr=1.0)
    runner = StepRunner(module, opt)
    assert (runner.current_epoch, runner.callback_metrics, runner.should_stop) == (0, {}, False)
    assert runner.ewc is None and runner.last_ewc_penalty is None
    cb = MultiPhaseTraining([[1.0], [0.5], "stop"], [1, "adaptive", 0], monitor="v", patience=1)
    seen = []
    for epoch, v in enumerate([1.0, 1.0, 2.0, 3.0]):
        runner.current_epoch, runner.callback_metrics = epoch, {"v": torch.tensor(v)}
        cb.on_validation_epoch_end(runner, module)
        seen.append((cb.idx, opt.param_groups[0]["lr"], runner.should_stop))
    assert seen == [(0, 1.0, False), (1, 0.5, False), (1, 0.5, False), (2, 0.5, True)]
