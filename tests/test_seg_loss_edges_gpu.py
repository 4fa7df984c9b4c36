"""Segmentation-loss kernels of csrc/loss_optim.hip (adell_dice_focal_*, adell_class_sums_*,
adell_seg_loss_*) at their edges, against oracle/torch_ref/losses.py evaluated in fp64 on the CPU
(autograd for the gradients) on the cases of tests/loss_optim_cases.py:

* probabilities that are 0, 1, denormal or on either side of the clamp eps, with target 0 and 1;
* a volume of 704 880 voxels per item (87 slabs for the 64-thread fp64 folds, a backward that loops);
* C = 32, the limit of the per-class accumulator (C = 33 is refused before any launch).

Tolerances. Special voxels, element by element: |kernel - ref64| <= 4 |ref32 - ref64| + 2^-20 |ref64|,
ref32 the same restatement in fp32 on the CPU; plus the suite's whole-tensor check (max error against
the largest gradient). Large volume and C = 32, whole tensors: max error / largest magnitude <=
max(4 x that of ref32, 2^-20). Measured on an MI355X (yardstick = ref32, kernel), values / gradients:

    large volume        values: yardstick  kernel      gradients: yardstick  kernel
    bce                         9.28e-08   3.40e-08               4.41e-08   8.27e-08
    cat_ce                      4.65e-08   4.65e-08               3.68e-08   6.23e-08
    mc_focal (gamma 3)          1.28e-07   1.62e-07               9.41e-08   9.41e-08
    mc_dice                     2.54e-08   2.54e-08               2.52e-08   8.54e-08
    fused pair, dice            5.22e-08   5.22e-08               1.10e-07   1.02e-07
    fused pair, focal           3.37e-08   3.37e-08               (the same gradient)
    class sums                  7.11e-08   2.36e-08               4.81e-08   4.81e-08
    C = 32 cat_ce               6.77e-08   4.66e-08               6.22e-08   6.22e-08
    C = 32 mc_focal (gamma 3)   8.21e-08   8.21e-08               8.52e-08   2.20e-08
    C = 32 mc_dice              2.38e-08   2.38e-08               1.20e-07   3.79e-08

Special voxels: the worst element of every entry sits at 0.07 ... 0.37 of its bound; the whole-tensor error
is 3e-08 ... 2.5e-07 of the largest gradient, except mc_focal_loss with gamma 0.4: 1.5e-05 (C = 2) and
9.2e-05 (C = 5), where the fp32 restatement is as far off (see _check_special).

What this file found: at p == 0 on a positive voxel the dice gradients of the fused pair and of
mc_generalized_dice_loss took clip(t p, 0) as clipped (d/dp = 0) where the reference passes the gradient
(d/dp = t): the whole-tensor error was 0.65 ... 1.35 of the largest gradient.
"""
import functools

import pytest
import torch

import loss_optim_cases as LC
from adell_mri_amd import ops
from adell_mri_amd._lib import AdellHipError
from adell_mri_amd.modules.segmentation import losses as HL
from adell_mri_amd.utils.utils import loss_factory

pytestmark = pytest.mark.gpu

WHOLE_REL, WHOLE_ABS = 3e-5, 1e-10      # the whole-tensor gradient check of tests/test_losses_gpu.py
_FACTORY = {fn.__name__ for family in loss_factory.values() for fn in family.values()}


def _entries(C):
    return LC.BINARY_ENTRIES if C == 1 else LC.mc_entries(C)


@functools.lru_cache(maxsize=None)
def _ref_special(C, name, dtype):
    fn, kw = _entries(C)[name]
    return LC.ref_loss(fn, kw, LC.special_case(C), dtype)


def _hip_loss(fn, kw, case, cuda):
    p = case["p"].to(cuda).requires_grad_(True)
    v = getattr(HL, fn)(p, case["t"].to(cuda), **kw).reshape(p.shape[0])
    (v * case["r"].to(cuda)).sum().backward()
    torch.cuda.synchronize()
    return v.detach().cpu(), p.grad.cpu()


def _hip_pair(dice_kw, focal_kw, case, cuda):
    loss = HL.CompoundLoss([(HL.binary_generalized_dice_loss, dict(dice_kw)),
                            (HL.binary_focal_loss, dict(focal_kw))])
    assert loss._fused_pair() is not None
    p = case["p"].to(cuda).requires_grad_(True)
    dice, focal = loss(p, case["t"].to(cuda))
    ((dice * case["r"].to(cuda)).sum() + (focal * case["r2"].to(cuda)).sum()).backward()
    torch.cuda.synchronize()
    return (dice.detach().cpu(), focal.detach().cpu()), p.grad.cpu()


def _check_special(tag, case, val, grad, val32, grad32, val64, grad64):
    assert torch.isfinite(grad).all() and torch.isfinite(val).all()
    verr = (val.double() - val64).abs()
    assert bool((verr <= LC.elementwise_bound(val32, val64)).all()), (tag, val, val64, val32)
    sp = case["special"]
    err = (grad.double() - grad64).abs()
    bound = LC.elementwise_bound(grad32, grad64)
    bad = sp & (err > bound)
    worst = float((err[sp] / bound[sp].clamp_min(1e-300)).max())
    print(f"LOSS-SPECIAL {tag}: worst special element at {worst:.2f} of its bound; whole tensor "
          f"{float(err.max()) / float(grad64.abs().max()):.2e} of the largest gradient")
    assert not bool(bad.any()), (tag, [(tuple(i), float(case["p"][tuple(i)]), float(case["t"][tuple(i)]),
                                        float(grad[tuple(i)]), float(grad64[tuple(i)]), float(grad32[tuple(i)]))
                                       for i in bad.nonzero().tolist()[:6]])
    # whole tensor: the suite's figure, or 4 x what the fp32 restatement itself reaches where that is more
    # (mc_focal_loss forms 1 - (1 - p) + eps: for p of a few 1e-7 the fp32 rounding of 1 - p is percents
    # of q, on an element that carries one of the larger gradients)
    whole = max(WHOLE_REL, 4 * LC.rel_err(grad32, grad64))
    assert float(err.max()) <= whole * float(grad64.abs().max()) + WHOLE_ABS, tag
    # the special voxels carry the largest gradients (1 / eps): the ordinary ones against their own
    assert float(err[~sp].max()) <= WHOLE_REL * float(grad64[~sp].abs().max()) + WHOLE_ABS, tag


@pytest.mark.parametrize("C,name", [(C, n) for C in (1, 2, 5) for n in _entries(C)])
def test_special_values_match_fp64(cuda, C, name):
    fn, kw = _entries(C)[name]
    assert fn in _FACTORY
    case = LC.special_case(C)
    val, grad = _hip_loss(fn, kw, case, cuda)
    _check_special(f"C={C} {name}", case, val, grad, *_ref_special(C, name, torch.float32),
                   *_ref_special(C, name, torch.float64))
    if fn == "binary_focal_loss":
        # exactly 0 where the reference's clamp makes them 0: p < eps, and 1 - p < eps for the negative term
        p, t, sp = case["p"], case["t"], case["special"]
        lo, hi = sp & (p < LC.EPS32), sp & (1 - p < LC.EPS32) & (t < 0.5)
        assert int(lo.sum()) == 16 and int(hi.sum()) == 6
        assert int(torch.count_nonzero(grad[lo])) == 0 and int(torch.count_nonzero(grad[hi])) == 0
        g64 = _ref_special(C, name, torch.float64)[1]
        assert int(torch.count_nonzero(g64[lo])) == 0 and int(torch.count_nonzero(g64[hi])) == 0


@pytest.mark.parametrize("name", list(LC.PAIR_ENTRIES))
def test_special_values_fused_pair_through_compound_loss(cuda, name):
    dice_kw, focal_kw = LC.PAIR_ENTRIES[name]
    case = LC.special_case(1)
    (dice, focal), grad = _hip_pair(dice_kw, focal_kw, case, cuda)
    (d32, f32), g32 = LC.ref_pair(dice_kw, focal_kw, case, torch.float32)
    (d64, f64), g64 = LC.ref_pair(dice_kw, focal_kw, case, torch.float64)
    _check_special(name, case, torch.cat([dice, focal]), grad, torch.cat([d32, f32]), g32,
                   torch.cat([d64, f64]), g64)


# ---- large volume ---------------------------------------------------------------------------------------
def _check_whole(tag, val, grad, val32, grad32, val64, grad64):
    v_y, v_k = LC.rel_err(val32, val64), LC.rel_err(val, val64)
    g_y, g_k = LC.rel_err(grad32, grad64), LC.rel_err(grad, grad64)
    print(f"LOSS-WHOLE {tag}: values yardstick {v_y:.2e} kernel {v_k:.2e}   "
          f"gradients yardstick {g_y:.2e} kernel {g_k:.2e}")
    assert torch.isfinite(grad).all()
    assert v_k <= max(4 * v_y, LC.REL_FLOOR), (tag, val, val64)
    assert g_k <= max(4 * g_y, LC.REL_FLOOR), tag


LARGE_KINDS = {"bce": 1, "cat_ce": 3, "mc_focal_g3": 3, "mc_dice": 3}


@pytest.mark.parametrize("name", list(LARGE_KINDS))
def test_large_volume_seg_loss_kinds(cuda, name):
    C = LARGE_KINDS[name]
    fn, kw = _entries(C)[name]
    case = LC.large_case(C)
    assert C * LC.LARGE_V > LC.SEGLOSS_BWD_SPAN or C == 1
    val, grad = _hip_loss(fn, kw, case, cuda)
    _check_whole(f"large {name}", val, grad, *LC.ref_loss(fn, kw, case, torch.float32),
                 *LC.ref_loss(fn, kw, case, torch.float64))
    again = _hip_loss(fn, kw, case, cuda)
    assert torch.equal(again[0], val) and torch.equal(again[1], grad)      # fixed-order folds


def test_large_volume_fused_pair(cuda):
    dice_kw, focal_kw = LC.PAIR_ENTRIES["pair_g2"]
    case = LC.large_case(1)
    assert -(-LC.LARGE_V // LC.LOSS_SLAB) > LC.FINALIZE_THREADS
    (dice, focal), grad = _hip_pair(dice_kw, focal_kw, case, cuda)
    (d32, f32), g32 = LC.ref_pair(dice_kw, focal_kw, case, torch.float32)
    (d64, f64), g64 = LC.ref_pair(dice_kw, focal_kw, case, torch.float64)
    _check_whole("large pair dice", dice, grad, d32, g32, d64, g64)
    _check_whole("large pair focal", focal, grad, f32, g32, f64, g64)
    (dice2, focal2), grad2 = _hip_pair(dice_kw, focal_kw, case, cuda)
    assert torch.equal(dice2, dice) and torch.equal(focal2, focal) and torch.equal(grad2, grad)


def test_large_volume_class_sums(cuda):
    case = LC.large_case(3)
    B, C = case["p"].shape[:2]
    p3, t3 = HL._as_bvc(case["p"]), HL._as_bvc(case["t"])           # [B, V, C]
    gs = torch.randn((B, C, 3), generator=torch.Generator().manual_seed(3))

    def ref(dtype):
        p, t, g = p3.to(dtype), t3.to(dtype), gs.to(dtype)
        sums = torch.stack([(p * t).sum(1), p.sum(1), t.sum(1)], -1)
        return sums, g[:, None, :, 0] * t + g[:, None, :, 1]

    def run():
        p = p3.to(cuda).requires_grad_(True)
        sums = HL._ClassSumsFn.apply(p, t3.to(cuda))
        sums.backward(gs.to(cuda))
        torch.cuda.synchronize()
        return sums.detach().cpu(), p.grad.cpu()

    sums, grad = run()
    assert sums.shape == (B, C, 3)
    _check_whole("large class sums", sums, grad, *ref(torch.float32), *ref(torch.float64))
    # sum t is a count: exact
    assert torch.equal(sums[..., 2].double(), ref(torch.float64)[0][..., 2])
    again = run()
    assert torch.equal(again[0], sums) and torch.equal(again[1], grad)


# ---- C = 32 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cat_ce", "mc_focal_g3", "mc_dice"])
def test_thirty_two_classes(cuda, name):
    fn, kw = LC.mc_entries(LC.SEGLOSS_MAX_C)[name]
    case = LC.c32_case()
    val, grad = _hip_loss(fn, kw, case, cuda)
    _check_whole(f"C=32 {name}", val, grad, *LC.ref_loss(fn, kw, case, torch.float32),
                 *LC.ref_loss(fn, kw, case, torch.float64))


def test_thirty_three_classes_are_refused(cuda):
    C = LC.SEGLOSS_MAX_C + 1
    p = torch.full((2, 210, C), 1.0 / C, device=cuda)
    t = torch.zeros_like(p)
    cw = torch.ones(C, device=cuda)
    sums = torch.zeros((2, C, 2), device=cuda)
    for kind in (1, 2, 3):
        with pytest.raises(AdellHipError):
            ops.seg_loss_fwd(kind, p, t, cw, 1e-6, 1.0, 0.0, 2.0, 1.0, 1.0)
        with pytest.raises(AdellHipError):
            ops.seg_loss_bwd(kind, p, t, cw, 1e-6, 1.0, 0.0, 2.0, 1.0, 1.0, sums, torch.ones(2, device=cuda))
    with pytest.raises(AdellHipError):
        HL.cat_cross_entropy(p.permute(0, 2, 1).reshape(2, C, 5, 6, 7), t.permute(0, 2, 1).reshape(2, C, 5, 6, 7))
    torch.cuda.synchronize()


# ---- the two backward entries of the fused pair -----------------------------------------------------------
@pytest.mark.parametrize("gamma", [2.0, 0.5])
@pytest.mark.parametrize("which", ["special", "large"])
def test_scalar_and_per_item_backward_agree_bitwise(cuda, which, gamma):
    case = LC.special_case(1) if which == "special" else LC.large_case(1)
    p, t = case["p"].to(cuda), case["t"].to(cuda)
    B = p.shape[0]
    conf = (1e-5, 1e-6, gamma, 1e-6)
    _, _, sums = ops.dice_focal_fwd(p, t, *conf, 0.7)
    gd, gf = 0.7, 1.3
    scalar = ops.dice_focal_bwd(p, t, sums, *conf, gd, gf, 0.7)
    per_item = ops.dice_focal_bwd_dev(p, t, sums, *conf, torch.full((B,), gd, device=cuda),
                                      torch.full((B,), gf, device=cuda), 0.7)
    torch.cuda.synchronize()
    assert torch.isfinite(scalar).all() and float(scalar.abs().max()) > 0
    assert torch.equal(scalar, per_item)
