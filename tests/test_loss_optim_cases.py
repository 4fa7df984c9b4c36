"""The cases of tests/loss_optim_cases.py checked without a GPU: the reference losses are finite at every
special value, RAdam's rectification switches on inside the schedule, every size crosses the launch
constant it is meant to cross, and the step schedule gives the same result on torch.optim in fp32 and
in fp64 (so it is expressed identically on both sides before any kernel is involved)."""
import numpy as np
import pytest
import torch

import loss_optim_cases as LC


# ---- losses ---------------------------------------------------------------------------------------
def test_special_values_are_what_they_claim():
    v, eps = LC.SPECIAL_VALUES.astype(np.float64), float(LC.EPS32)
    assert v.dtype == np.float64 and len(v) == 12 and np.all(np.diff(v) > 0)
    assert v[0] == 0.0 and v[1] == 2.0 ** -149 and 0 < v[2] < 2.0 ** -126 and v[-1] == 1.0
    # either side of the clamp, in fp32 and against the fp64 reference's eps = 1e-6 alike; never on it
    assert v[3] < eps < v[4] and v[3] < 1e-6 < v[4]
    q = 1.0 - v                                      # exact for p in [0.5, 1]
    assert q[8] > eps > q[9] and q[8] > 1e-6 > q[9]
    assert not np.any(v == eps) and not np.any(q == eps)
    assert q[10] == 2.0 ** -24
    for C in (1, 2, 5):
        case = LC.special_case(C)
        p = case["p"].view(LC.SPECIAL_B, C, -1)
        assert np.array_equal(p[1, 0, :LC.N_SPECIAL].numpy(), np.tile(LC.SPECIAL_VALUES, 2))
        assert int(case["special"].sum()) == LC.SPECIAL_B * C * LC.N_SPECIAL
        assert LC.N_SPECIAL < p.shape[-1]            # ordinary voxels remain: the sums are not degenerate
        if C > 1:
            t = case["t"].view(LC.SPECIAL_B, C, -1)
            assert torch.equal(t.sum(1), torch.ones_like(t[:, 0]))


def _finite_cases():
    for name in LC.FINITE_BINARY:
        yield (1, name)
    for C in (2, 5):
        for name in LC.FINITE_MC:
            yield (C, name)


@pytest.mark.parametrize("C,name", list(_finite_cases()))
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_reference_is_finite_at_every_special_value(C, name, dtype):
    fn, kw = (LC.BINARY_ENTRIES if C == 1 else LC.mc_entries(C))[name]
    value, grad = LC.ref_loss(fn, kw, LC.special_case(C), dtype)
    assert torch.isfinite(value).all()
    assert torch.isfinite(grad).all()
    assert float(grad[LC.special_case(C)["special"]].abs().max()) > 0


def test_reference_clamp_zeroes_the_focal_gradient():
    """Where the GPU test demands an exact zero the fp64 reference has one."""
    case = LC.special_case(1)
    _, grad = LC.ref_loss("binary_focal_loss", dict(gamma=0.5), case, torch.float64)
    p, t, sp = case["p"].double(), case["t"], case["special"]
    assert int((grad[sp & (p < 1e-6)] != 0).sum()) == 0
    assert int((grad[sp & (1 - p < 1e-6) & (t < 0.5)] != 0).sum()) == 0
    assert int((sp & (p < 1e-6)).sum()) == 2 * 2 * 4 and int((sp & (1 - p < 1e-6)).sum()) == 2 * 2 * 3


def test_loss_sizes_cross_their_launch_constants():
    V = LC.LARGE_V
    assert V == 704_880
    slabs = -(-V // LC.LOSS_SLAB)
    assert slabs == 87 > LC.FINALIZE_THREADS and V % LC.LOSS_SLAB == 368
    assert 3 * V == 2_114_640 > LC.SEGLOSS_BWD_SPAN          # the backward of the C = 3 kinds loops
    assert V < LC.SEGLOSS_BWD_SPAN                           # ... and BCE (C = 1) does not
    assert LC.large_case(1)["p"].shape == (2, 1, 88, 90, 89)
    assert LC.large_case(3)["p"].shape == (2, 3, 88, 90, 89)
    assert float(LC.large_case(1)["r"][0]) != float(LC.large_case(1)["r"][1])
    assert LC.c32_case()["p"].shape == (2, LC.SEGLOSS_MAX_C, 5, 6, 7)


# ---- optimisers -----------------------------------------------------------------------------------
def test_radam_rectification_switches_on_at_step_six():
    assert LC.radam_rho(5) < 5.0 < LC.radam_rho(6)
    assert abs(LC.radam_rho(5) - 4.99) < 0.01 and abs(LC.radam_rho(6) - 5.99) < 0.01
    # the late parameter takes its 5th step while the others take their 6th; both sides are in the case
    steps = LC.n_steps("radam")
    assert steps == 7 and LC.expected_steps("radam", 6)[0][:4] == [6, 6, 6, 5]
    assert LC.expected_steps("radam", 7)[0][3] == 6


def test_optimiser_sizes_cross_their_launch_constants():
    cap = LC.OPTIM_CAP
    assert cap == 1_048_576
    for name in LC.OPTIM_CONFIGS:
        g0, g1 = LC.group_shapes(name)
        sizes = [int(np.prod(s)) for s in g0]
        assert sizes[:5] == [cap + 259, 5, 1, 70_001, 0] and [tuple(s) for s in g1] == [(33, 17), (7,)]
        assert sizes[0] > cap and sizes[0] % 4 != 0 and LC.padded(5) == 8
        total = sum(LC.padded(n) for n in sizes)
        if LC.OPTIM_CONFIGS[name]["cls"] == "SGD":
            assert total > LC.SGD_VEC * cap                  # second trip of the float4 loop
        else:
            assert cap < total
        # the late parameter splits group 0 into runs, at non-zero offsets from step 2 on (by step count);
        # the run behind it is the zero-element parameter alone (no launch) unless SGD's extra follows
        sgd = len(g0) > 5
        assert LC.expected_launches(name, 1) == [2 if sgd else 1, 1]
        assert LC.expected_launches(name, 2) == [3 if sgd else 2, 1]
        assert LC.expected_launches(name, LC.n_steps(name))[1] == 1
    small, wrap = LC.SGD_DIRECT_SIZES
    assert small == 4 * cap + 3 and small % 4 == 3
    assert (wrap >> 2) > cap and wrap % 4 == 3               # vector body wraps, scalar tail of 3
    assert LC.EMA_SIZE == cap + 259
    assert len({bool(v["first"]) for v in LC.SGD_DIRECT_VARIANTS.values()}) == 2


def test_gradients_spread_over_three_decades_with_exact_zeros():
    _, grads = LC.optim_tensors("adam")
    g = grads[0][0][0]
    assert int((g == 0).sum()) >= 3
    mags = g[g != 0].abs().log10()
    assert float(mags.quantile(0.9) - mags.quantile(0.1)) > 2.0


@pytest.mark.parametrize("name", list(LC.OPTIM_CONFIGS))
def test_schedule_agrees_between_fp32_and_fp64_torch_optim(name):
    """The yardstick of the GPU test: fp32 torch.optim against fp64 torch.optim on the same schedule.
    A rounding-level difference (1e-7 ... 1e-6 of the largest magnitude, a few times that on second
    moments whose inputs span six decades) is sane; a schedule expressed differently on the two sides
    (the late parameter, the grad_scale step) would be off by whole gradients."""
    ref64 = LC.reference_snapshots(name, torch.float64)
    ref32 = LC.reference_snapshots(name, torch.float32)
    last = LC.n_steps(name)
    worst = 0.0
    for step in (1, last):
        a, b = LC.compared_tensors(ref32[step]), LC.compared_tensors(ref64[step])
        assert [k for k, _ in a] == [k for k, _ in b]
        for (label, x), (_, y) in zip(a, b):
            assert x.dtype == torch.float32 and y.dtype == torch.float64
            worst = max(worst, LC.rel_err(x, y))
            assert LC.rel_err(x, y) < 2e-5, (name, step, label)
        for pid, ent in ref64[step]["state"].items():
            if "step" in ent:
                gi, i = (0, pid) if pid < len(LC.group_shapes(name)[0]) else (1, pid - len(LC.group_shapes(name)[0]))
                assert float(ent["step"]) == LC.expected_steps(name, step)[gi][i]
    # after step 1 the late parameter is untouched and has no state (Adagrad: its initial zero state)
    p0 = LC.optim_tensors(name)[0]
    assert torch.equal(ref32[1]["params"][0][3], p0[0][3])
    assert 3 not in ref32[1]["state"] or float(ref32[1]["state"][3]["step"]) == 0
    assert not torch.equal(ref32[last]["params"][0][3], p0[0][3])
    print(f"{name}: fp32 torch.optim vs fp64, worst tensor {worst:.2e}")
