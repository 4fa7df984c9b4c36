"""Optimiser and EMA kernels of csrc/loss_optim.hip against fp64 torch.optim on the cases of
tests/loss_optim_cases.py: a group beyond the 4096 x 256 launch cap with ragged tails, padded slices, a
parameter that joins late (runs at non-zero offsets, split by step count), grad_scale on the last step.
Parameters AND state buffers are compared, after step 1 and after the last step.

Tolerance: per compared tensor, 4 x the error of fp32 torch.optim on the CPU against the same fp64
reference (max |difference| / largest reference magnitude), never below one fp32 ulp (1.19e-07).
Measured on an MI355X, worst tensor of each configuration (yardstick = fp32 torch.optim, kernel = the
fused class), parameters / state buffers:

    configuration     parameters: yardstick  kernel      state buffers: yardstick  kernel
    sgd_plain_nowd                1.26e-07   1.26e-07                   -          -
    sgd_plain                     1.11e-07   1.11e-07                   -          -
    sgd_momentum                  1.10e-07   1.10e-07                   1.26e-07   1.01e-07
    sgd_nesterov                  1.18e-07   1.18e-07                   1.16e-07   8.00e-08
    adam                          9.04e-08   1.40e-07                   1.44e-07   1.48e-07
    adamw                         1.89e-07   1.89e-07                   1.54e-07   1.54e-07
    adamw_amsgrad                 1.89e-07   1.89e-07                   1.54e-07   1.54e-07
    adamax                        8.21e-08   8.21e-08                   1.07e-07   1.26e-07
    adagrad                       1.14e-07   1.14e-07                   1.25e-07   1.25e-07
    nadam                         1.46e-07   1.46e-07                   1.46e-07   1.46e-07
    radam (7 steps)               2.23e-07   2.23e-07                   2.28e-07   4.29e-07
    rmsprop                       7.37e-07   7.37e-07                   1.53e-07   1.53e-07
    ops.sgd_step (10 cases)       4.2e-08 .. 4.7e-08, kernel == yardstick in every case
    ops.ema_update 0.999 / 0 / 1  4.83e-08 / 5.91e-08 / 0    5.95e-08 / 5.91e-08 / 0

No rule needs more than 4 x. Before the betas reached the library as doubles the kernels formed 1 - beta
from the fp32 rounding of beta: exp_avg_sq was 1.29e-05 off after one step (yardstick 1.20e-07; Adam,
NAdam, RAdam), square_avg 9.87e-07 (RMSprop), exp_avg 2.48e-07 (every rule with a first moment); this
test is what found it. It also found exp_inf = eps in the padding of Adamax' state.
"""
import pytest
import torch

import loss_optim_cases as LC
from adell_mri_amd import ops

pytestmark = pytest.mark.gpu

_LAUNCHERS = ("sgd_step", "adamw_step", "adamw_amsgrad_step", "optim_step")


def _padding_nonzero(flat, buf):
    """Number of non-zero padding elements of a flat buffer (between a slice's end and its padded end)."""
    bad = 0
    for p, o, e in zip(flat.params, flat.offsets, flat.ends):
        bad += int(torch.count_nonzero(buf[o + p.numel():e]))
    return bad


@pytest.mark.parametrize("name", list(LC.OPTIM_CONFIGS))
def test_fused_optimiser_matches_fp64_torch_optim(cuda, name, monkeypatch):
    ref64 = LC.reference_snapshots(name, torch.float64)
    ref32 = LC.reference_snapshots(name, torch.float32)
    last = LC.n_steps(name)

    launches = []
    for fn in _LAUNCHERS:
        def counted(*a, _f=getattr(ops, fn), _param=1 if fn == "optim_step" else 0, **k):
            launches.append(a[_param].numel())
            return _f(*a, **k)
        monkeypatch.setattr(ops, fn, counted)
    per_step, late_state = {}, {}

    def after_step(step, opt):
        per_step[step] = list(launches)
        del launches[:]
        if step == 1:       # the late parameter's slice of every state buffer, and what lies before it
            flat = opt.flat_groups[0]
            o, e = flat.offsets[LC.LATE[1]], flat.ends[LC.LATE[1]]
            for key, buf in opt._flat_state[0].items():
                if torch.is_tensor(buf):
                    late_state[key] = (int(torch.count_nonzero(buf[o:e])), int(torch.count_nonzero(buf[:o])))

    got, opt, params = LC.run_schedule(name, device=cuda, fused=True, after_step=after_step)
    torch.cuda.synchronize()

    # exactly one launch per run, covering the run's padded elements
    shapes = LC.group_shapes(name)
    for step in range(1, last + 1):
        assert len(per_step[step]) == sum(LC.expected_launches(name, step)), (step, per_step[step])
    assert LC.expected_launches(name, last)[1] == 1       # the usual case: the whole group in one run
    active_last = sum(LC.padded(int(torch.Size(s).numel())) for g in shapes for s in g)
    assert sum(per_step[last]) == active_last

    worst = {"param": [0.0, 0.0], "state": [0.0, 0.0]}
    for step in (1, last):
        want, yard, have = (LC.compared_tensors(s[step]) for s in (ref64, ref32, got))
        have = dict(have)
        for (label, w), (_, y) in zip(want, yard):
            if label not in have:
                # torch.optim.Adagrad creates its (zero) state up front; the fused classes once stepped
                assert label.startswith("state") and not bool(w.any()), (step, label)
                continue
            k = have[label]
            assert k.shape == w.shape and k.dtype == torch.float32, (step, label)
            y_err, k_err = LC.rel_err(y, w), LC.rel_err(k, w)
            kind = "param" if label.startswith("param") else "state"
            worst[kind][0] = max(worst[kind][0], y_err)
            worst[kind][1] = max(worst[kind][1], k_err)
            assert k_err <= LC.optim_allowed(y_err), (name, step, label, k_err, y_err)
        assert set(have) <= {label for label, _ in want}, (step, sorted(set(have) - {l for l, _ in want}))
        # per-parameter step counts
        pid = 0
        for gi, group in enumerate(LC.expected_steps(name, step)):
            for i, n in enumerate(group):
                ent = got[step]["state"].get(pid)
                if "step" in (ref64[step]["state"].get(pid) or {}):
                    assert float(ref64[step]["state"][pid]["step"]) == n
                    assert (float(ent["step"]) if ent is not None else 0) == n, (step, pid)
                if step == last:
                    assert int(opt._flat_state[gi]["steps"][i]) == n, (gi, i)
                pid += 1
    print(f"OPTIM {name:16s} params: yardstick {worst['param'][0]:.2e} kernel {worst['param'][1]:.2e}   "
          f"state: yardstick {worst['state'][0]:.2e} kernel {worst['state'][1]:.2e}")

    # the parameter without a gradient (step 1) and the zero-element parameter are bit-for-bit untouched
    p0 = LC.optim_tensors(name)[0]
    gi, i = LC.LATE
    assert torch.equal(got[1]["params"][gi][i], p0[gi][i])
    assert i not in got[1]["state"]
    assert got[last]["params"][0][4].numel() == 0
    # ... and so is its slice of every state buffer, though the launches on both sides of it ran
    for key, (inside, before) in late_state.items():
        assert inside == 0 and before > 0, (key, inside, before)
    # every padding element of the parameters and of each state buffer is exactly 0 after the last step
    for gi, flat in enumerate(opt.flat_groups):
        assert any(e - o - p.numel() > 0 for p, o, e in zip(flat.params, flat.offsets, flat.ends))
        assert _padding_nonzero(flat, flat.data) == 0, ("data", gi)
        for key, buf in opt._flat_state[gi].items():
            if torch.is_tensor(buf):
                assert _padding_nonzero(flat, buf) == 0, (key, gi)


# ---- ops.sgd_step / ops.ema_update directly -------------------------------------------------------------
@pytest.mark.parametrize("n", LC.SGD_DIRECT_SIZES)
@pytest.mark.parametrize("variant", list(LC.SGD_DIRECT_VARIANTS))
def test_sgd_step_vector_body_wrap_and_tail(cuda, n, variant):
    v = LC.SGD_DIRECT_VARIANTS[variant]
    p, g, b = LC.direct_tensors(n)
    lr, wd, scale = 1e-2, 5e-3, 0.5
    args = (lr, v["momentum"], wd, v["nesterov"], v["first"], scale)
    p64, b64 = LC.sgd_reference(p.double(), g.double(), b.double(), *args)
    p32, b32 = LC.sgd_reference(p, g, b, *args)
    pd, gd = p.to(cuda), g.to(cuda)
    # first step: whatever the buffer holds must not be read
    bd = None if v["momentum"] == 0.0 else (torch.full((n,), float("nan"), device=cuda) if v["first"]
                                            else b.to(cuda))
    ops.sgd_step(pd, gd, bd, lr, v["momentum"], wd, v["nesterov"], v["first"], scale)
    torch.cuda.synchronize()
    assert torch.equal(gd.cpu(), g)
    k_err, y_err = LC.rel_err(pd.cpu(), p64), LC.rel_err(p32, p64)
    print(f"SGD-DIRECT {variant} n={n}: param yardstick {y_err:.2e} kernel {k_err:.2e}")
    assert k_err <= LC.optim_allowed(y_err)
    if bd is not None:
        kb, yb = LC.rel_err(bd.cpu(), b64), LC.rel_err(b32, b64)
        assert kb <= LC.optim_allowed(yb), (kb, yb)
    # the bound is an absolute one (of the largest magnitude): a tail or a wrapped vector left unstepped
    # cannot hide behind it, the reference moves those elements by far more
    tol = LC.optim_allowed(y_err) * float(p64.abs().max())
    moved = (p64 - p.double()).abs() > 4 * tol
    assert bool(moved[-3:].any()) and bool(moved[LC.SGD_VEC * LC.OPTIM_CAP:].any()) and moved.float().mean() > 0.5


@pytest.mark.parametrize("decay", LC.EMA_DECAYS)
def test_ema_update_beyond_the_launch_cap(cuda, decay):
    n = LC.EMA_SIZE
    shadow, p, _ = LC.direct_tensors(n)
    s64 = shadow.double() - (1.0 - decay) * (shadow.double() - p.double())
    s32 = shadow - (1.0 - decay) * (shadow - p)
    sd, pd = shadow.to(cuda), p.to(cuda)
    ops.ema_update(sd, pd, decay)
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu(), p)
    k_err, y_err = LC.rel_err(sd.cpu(), s64), LC.rel_err(s32, s64)
    print(f"EMA decay={decay}: yardstick {y_err:.2e} kernel {k_err:.2e}")
    assert k_err <= LC.optim_allowed(y_err)
    if decay == 1.0:
        assert torch.equal(sd.cpu(), shadow)            # bit-for-bit unchanged
    if decay == 0.0:
        # the shadow becomes the parameter up to the rounding of s - (s - p), tail and wrap included
        assert float((sd.cpu() - p).abs().max()) <= 2 * LC.ULP32 * max(float(shadow.abs().max()), float(p.abs().max()))
