"""Cases of the edge tests of csrc/loss_optim.hip (optimiser, EMA and segmentation-loss kernels), shared
by tests/test_loss_optim_cases.py (CPU), tests/test_optim_kernels_gpu.py and
tests/test_seg_loss_edges_gpu.py. Everything is seeded; inputs are fp32 and every fp64 reference reads
the same fp32 values cast up."""
import functools

import numpy as np
import torch

from oracle.torch_ref import losses as RL

# ---- launch constants of adell_mri_amd/csrc/loss_optim.hip (and optim.py) the sizes below must cross ----
OPTIM_THREADS = 256          # every optimiser / EMA kernel: __launch_bounds__(256), loss_optim.hip:293
OPTIM_MAX_BLOCKS = 4096      # "if (blocks > 4096) blocks = 4096": :343 (sgd) :387 (adam) :448 (amsgrad)
#                              :468 (ema) :799 (optim_step)
SGD_VEC = 4                  # adell_sgd_kernel steps float4 (n >> 2, :299), scalar tail n % 4 (:320)
FLAT_ALIGN = 4               # optim.py FlatParameters: every slice is rounded up to 4 floats
LOSS_SLAB = 8192             # ADELL_LOSS_SLAB :9 -- voxels per partial-sum block (dice+focal, class sums)
FINALIZE_THREADS = 64        # the fp64 folds stride over the slabs with 64 threads, :73 and :232
DICE_FOCAL_BWD_SPAN = 2048 * 1024   # adell_dice_focal_bwd: (S + 1023) / 1024 blocks capped at 2048, :160
CLASS_SUMS_BWD_SPAN = 4096 * 1024   # adell_class_sums_bwd, :282
SEGLOSS_BWD_SPAN = 8192 * 256       # adell_seg_loss_bwd: one element per thread up to 8192 blocks, :704
SEGLOSS_MAX_C = 32           # acc[32][2] of adell_segloss_finalize_kernel :570, checked at :659

ULP32 = 2.0 ** -23           # one fp32 ulp, relative
REL_FLOOR = 2.0 ** -20       # "a handful of ulps": the floor of the loss comparisons


# =====================================================================================================
# Optimisers
# =====================================================================================================
OPTIM_CAP = OPTIM_MAX_BLOCKS * OPTIM_THREADS           # elements one trip of the grid-stride loop covers
GROUP0_SHAPES = ((OPTIM_CAP + 259,), (5,), (1,), (70_001,), (0,))
GROUP1_SHAPES = ((33, 17), (7,))
SGD_EXTRA_SHAPE = (3_200_000,)                         # SGD: group 0 beyond 4 x OPTIM_CAP elements
LATE = (0, 3)                # (group, index) of the parameter without a gradient on step 1
LATE_FROM = 2
GRAD_SCALE_LAST = 0.25       # param_groups[0]["grad_scale"] on the last step (a power of two: the
#                              scaled reference gradient is exact in fp32 as well)

_ADAPTIVE = dict(lr=(1e-3, 4e-3), wd=(1e-2, 5e-2))
OPTIM_CONFIGS = {
    "sgd_plain_nowd": dict(cls="SGD", kw=dict(momentum=0.0), lr=(1e-2, 3e-2), wd=(0.0, 0.0)),
    "sgd_plain": dict(cls="SGD", kw=dict(momentum=0.0), lr=(1e-2, 3e-2), wd=(5e-3, 2e-2)),
    "sgd_momentum": dict(cls="SGD", kw=dict(momentum=0.9), lr=(1e-2, 3e-2), wd=(5e-3, 2e-2)),
    "sgd_nesterov": dict(cls="SGD", kw=dict(momentum=0.99, nesterov=True), lr=(1e-2, 3e-2),
                         wd=(5e-3, 2e-2)),
    "adam": dict(cls="Adam", kw={}, **_ADAPTIVE),
    "adamw": dict(cls="AdamW", kw={}, **_ADAPTIVE),
    "adamw_amsgrad": dict(cls="AdamW", kw=dict(amsgrad=True), **_ADAPTIVE),
    "adamax": dict(cls="Adamax", kw={}, **_ADAPTIVE),
    "adagrad": dict(cls="Adagrad", kw=dict(lr_decay=0.05), lr=(1e-2, 3e-2), wd=(1e-2, 5e-2)),
    "nadam": dict(cls="NAdam", kw={}, **_ADAPTIVE),
    "radam": dict(cls="RAdam", kw={}, steps=7, **_ADAPTIVE),
    "rmsprop": dict(cls="RMSprop", kw={}, **_ADAPTIVE),
}


def n_steps(name):
    return OPTIM_CONFIGS[name].get("steps", 3)


def group_shapes(name):
    g0 = GROUP0_SHAPES + ((SGD_EXTRA_SHAPE,) if OPTIM_CONFIGS[name]["cls"] == "SGD" else ())
    return [g0, GROUP1_SHAPES]


def padded(n):
    return (n + FLAT_ALIGN - 1) // FLAT_ALIGN * FLAT_ALIGN


def radam_rho(t, beta2=0.999):
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    return rho_inf - 2.0 * t * beta2 ** t / (1.0 - beta2 ** t)


@functools.lru_cache(maxsize=3)
def _optim_tensors(sgd, steps):
    """(params[group][i], grads[step][group][i]) as fp32 CPU tensors. Gradient magnitudes spread over
    three decades, with a few exact zeros."""
    shapes = [GROUP0_SHAPES + ((SGD_EXTRA_SHAPE,) if sgd else ()), GROUP1_SHAPES]
    gen = torch.Generator().manual_seed(20241 + steps)
    params = [[torch.randn(s, generator=gen) for s in group] for group in shapes]
    grads = []
    for _ in range(steps):
        step = []
        for group in shapes:
            row = []
            for s in group:
                g = torch.randn(s, generator=gen) * 10.0 ** (-3.0 * torch.rand(s, generator=gen))
                flat = g.view(-1)
                if flat.numel() > 8:
                    flat[::1009] = 0.0
                    flat[-1] = 0.0
                row.append(g)
            step.append(row)
        grads.append(step)
    return params, grads


def optim_tensors(name):
    return _optim_tensors(OPTIM_CONFIGS[name]["cls"] == "SGD", n_steps(name))


def make_optimizer(name, params, fused):
    cfg = OPTIM_CONFIGS[name]
    groups = [dict(params=list(ps), lr=cfg["lr"][gi], weight_decay=cfg["wd"][gi])
              for gi, ps in enumerate(params)]
    if fused:
        from adell_mri_amd import optim as FO
        return getattr(FO, "Fused" + cfg["cls"])(groups, **cfg["kw"])
    return getattr(torch.optim, cfg["cls"])(groups, **cfg["kw"])


def has_grad(gi, i, step):
    return (gi, i) != LATE or step >= LATE_FROM


def expected_steps(name, step):
    """Per-parameter step counts after ``step`` steps of the schedule."""
    return [[step - (0 if (gi, i) != LATE else LATE_FROM - 1) for i in range(len(group))]
            for gi, group in enumerate(group_shapes(name))]


def expected_launches(name, step):
    """Launches of step ``step`` per group: one per maximal run of consecutive parameters that have a
    gradient and share their step count (SGD: share "this is my first step"), a run of zero elements
    not counting."""
    sgd = OPTIM_CONFIGS[name]["cls"] == "SGD"
    before = expected_steps(name, step - 1)
    out = []
    for gi, group in enumerate(group_shapes(name)):
        runs, prev, elems = 0, None, 0
        for i, shape in enumerate(group):
            key = None
            if has_grad(gi, i, step):
                key = (before[gi][i] == 0) if sgd else before[gi][i]
            if key != prev:
                runs += prev is not None and elems > 0
                elems = 0
            if key is not None:
                elems += padded(int(np.prod(shape)))
            prev = key
        runs += prev is not None and elems > 0
        out.append(int(runs))
    return out


def snapshot(opt, params):
    """Detached CPU copies of the parameters and of ``state_dict()["state"]``."""
    state = {}
    for pid, ent in opt.state_dict()["state"].items():
        state[pid] = {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v)
                      for k, v in ent.items()}
    return dict(params=[[p.detach().cpu().clone() for p in group] for group in params], state=state)


def run_schedule(name, dtype=torch.float32, device="cpu", fused=False, after_step=None):
    """The step schedule of the optimiser case on ``torch.optim`` (``fused=False``: the gradient of
    group 0 is multiplied by the last step's grad_scale) or on the Fused* class (the scale goes into
    ``param_groups[0]["grad_scale"]``). Returns ({step: snapshot} for step 1 and the last step, opt,
    params)."""
    params0, grads = optim_tensors(name)
    params = [[torch.nn.Parameter(p.to(device=device, dtype=dtype, copy=True)) for p in group]
              for group in params0]
    opt = make_optimizer(name, params, fused)
    last = n_steps(name)
    snaps = {}
    for step in range(1, last + 1):
        scale = GRAD_SCALE_LAST if step == last else 1.0
        opt.zero_grad(set_to_none=True)
        for gi, group in enumerate(params):
            for i, p in enumerate(group):
                if not has_grad(gi, i, step):
                    p.grad = None
                    continue
                g = grads[step - 1][gi][i].to(device=device, dtype=dtype, copy=True)
                if not fused and gi == 0:
                    g *= scale
                p.grad = g
        if fused:
            opt.param_groups[0]["grad_scale"] = scale
        opt.step()
        if after_step is not None:
            after_step(step, opt)
        if step in (1, last):
            snaps[step] = snapshot(opt, params)
    return snaps, opt, params


@functools.lru_cache(maxsize=None)
def reference_snapshots(name, dtype):
    """``torch.optim`` on the CPU in ``dtype`` (computed once per configuration, never modified)."""
    return run_schedule(name, dtype=dtype)[0]


def rel_err(x, ref64):
    """max |x - ref| over the largest reference magnitude (inf when the reference is all zero and x is not)."""
    if ref64.numel() == 0:
        return 0.0
    d = float((x.double() - ref64.double()).abs().max())
    m = float(ref64.double().abs().max())
    if m == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / m


def optim_allowed(yardstick):
    """4 x the error of fp32 torch.optim (multiply-add contraction, the division by sqrt(bc2) done as
    a division by a rounded scalar: a few ulps per step), never below one fp32 ulp of the largest
    magnitude."""
    return max(4.0 * yardstick, ULP32)


def compared_tensors(snap):
    """[(label, tensor)] of a snapshot: every parameter and every state tensor."""
    out = []
    for gi, group in enumerate(snap["params"]):
        for i, p in enumerate(group):
            out.append((f"param[{gi}][{i}]", p))
    for pid in sorted(snap["state"]):
        for k, v in sorted(snap["state"][pid].items()):
            if torch.is_tensor(v) and v.dim() > 0:
                out.append((f"state[{pid}].{k}", v))
    return out


def sgd_reference(p, g, buf, lr, momentum, wd, nesterov, first, grad_scale):
    """torch.optim.SGD's single-tensor update (dampening 0) in the dtype of its inputs."""
    d = g * grad_scale + wd * p
    if momentum != 0.0:
        buf = d.clone() if first else momentum * buf + d
        d = d + momentum * buf if nesterov else buf
    return p - lr * d, buf


# ops.sgd_step directly: the issue's size, and one more vector past the 4096 x 256 cap (the float4 body
# covers OPTIM_CAP *vectors* per trip, so only the second size takes a second trip of that loop)
SGD_DIRECT_SIZES = (SGD_VEC * OPTIM_CAP + 3, SGD_VEC * (OPTIM_CAP + 1) + 3)
SGD_DIRECT_VARIANTS = {
    "first_nesterov": dict(momentum=0.9, nesterov=True, first=True),
    "later_nesterov": dict(momentum=0.9, nesterov=True, first=False),
    "first_classical": dict(momentum=0.9, nesterov=False, first=True),
    "later_classical": dict(momentum=0.9, nesterov=False, first=False),
    "no_momentum": dict(momentum=0.0, nesterov=False, first=False),
}
EMA_SIZE = OPTIM_CAP + 259
EMA_DECAYS = (0.999, 0.0, 1.0)


@functools.lru_cache(maxsize=3)
def direct_tensors(n):
    gen = torch.Generator().manual_seed(n)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 10.0 ** (-3.0 * torch.rand(n, generator=gen))
    g[::1009] = 0.0
    b = torch.randn(n, generator=gen) * 0.1
    return p, g, b


# =====================================================================================================
# Losses
# =====================================================================================================
EPS32 = np.float32(1e-6)
_ONE = np.float32(1.0)
SPECIAL_VALUES = np.array([
    0.0,
    np.nextafter(np.float32(0.0), _ONE),             # the smallest denormal
    np.float32(1e-38),
    np.nextafter(EPS32, np.float32(0.0)),
    np.nextafter(EPS32, _ONE),
    np.float32(1e-4),
    np.float32(0.5),
    _ONE - np.float32(1e-4),
    np.nextafter(_ONE - EPS32, np.float32(0.0)),
    np.nextafter(_ONE - EPS32, _ONE),
    _ONE - np.float32(2.0 ** -24),
    1.0,
], dtype=np.float32)
SPECIAL_SPATIAL = (4, 5, 7)
SPECIAL_B = 2
N_SPECIAL = 2 * len(SPECIAL_VALUES)     # each value with target 0, then each with target 1

LARGE_SPATIAL = (88, 90, 89)
LARGE_B = 2
LARGE_V = 88 * 90 * 89
C32_SPATIAL = (5, 6, 7)


def class_weights(C):
    return [0.5 + 0.25 * (c % 4) for c in range(C)]


# name -> (function of oracle.torch_ref.losses / modules.segmentation.losses, kwargs)
BINARY_ENTRIES = {
    "bce": ("binary_cross_entropy", dict(weight=0.7, scale=2.0)),
    "bce_smoothed": ("binary_cross_entropy", dict(label_smoothing=0.1)),
    "focal_g2": ("binary_focal_loss", dict(gamma=2.0, alpha=0.7)),
    "focal_g1": ("binary_focal_loss", dict(gamma=1.0)),
    "focal_g05": ("binary_focal_loss", dict(gamma=0.5, alpha=0.7)),
    "focal_g0": ("binary_focal_loss", dict(gamma=0.0, alpha=1.3)),
    "dice": ("binary_generalized_dice_loss", dict(smooth=1.0)),
    "dice_smooth0": ("binary_generalized_dice_loss", dict(smooth=0.0)),   # t + p < eps is clamped
    "tversky": ("binary_focal_tversky_loss", dict(alpha=0.2, beta=0.8, gamma=2.0)),
}


def mc_entries(C):
    w = class_weights(C)
    return {
        "cat_ce": ("cat_cross_entropy", dict(weight=w, label_smoothing=0.2)),
        "mc_focal_g3": ("mc_focal_loss", dict(alpha=w, gamma=3.0)),
        "mc_focal_g04": ("mc_focal_loss", dict(alpha=w, gamma=0.4, label_smoothing=0.1)),
        "mc_dice": ("mc_generalized_dice_loss", dict(weight=w, smooth=0.1, scale=2.0)),
        "mc_dice_smooth0": ("mc_generalized_dice_loss", dict(weight=w, smooth=0.0)),
        "mc_tversky": ("mc_focal_tversky_loss", dict(alpha=w, beta=0.5, gamma=1.2)),
    }


# the fused dice + focal pair through CompoundLoss: (dice kwargs, focal kwargs)
PAIR_ENTRIES = {
    "pair_g2": (dict(smooth=1e-5, eps=1e-6), dict(gamma=2.0, eps=1e-6)),
    "pair_g05": (dict(smooth=1.0), dict(gamma=0.5)),
}
# where the CPU test pins the reference's finiteness (fp64 and fp32, value and gradient)
FINITE_BINARY = ("bce", "focal_g2", "focal_g05", "dice")
FINITE_MC = ("cat_ce", "mc_focal_g3", "mc_focal_g04", "mc_dice")


def _item_weights(B, gen):
    return torch.rand((B,), generator=gen) + 0.5


def _random_binary(B, spatial, gen):
    p = torch.sigmoid(torch.randn((B, 1, *spatial), generator=gen) * 2)
    t = (torch.rand(p.shape, generator=gen) > 0.6).float()
    return p, t


def _random_mc(B, C, spatial, gen):
    p = torch.softmax(torch.randn((B, C, *spatial), generator=gen) * 2, 1)
    cls = torch.randint(0, C, (B, *spatial), generator=gen)
    nd = len(spatial) + 1
    t = torch.nn.functional.one_hot(cls, C).permute(0, nd, *range(1, nd)).float().contiguous()
    return p, t


@functools.lru_cache(maxsize=None)
def special_case(C):
    """dict(p, t, r, r2, special): a small random volume with the special values written over the first
    voxels of every item. ``special`` marks those voxels (all channels). C = 1: the binary family;
    C = 2: the value in channel 0 and its complement in channel 1; C = 5: the complement spread over
    the four other channels. Target 1 is class 0, target 0 is class 1."""
    gen = torch.Generator().manual_seed(100 + C)
    B, k = SPECIAL_B, len(SPECIAL_VALUES)
    vals = torch.from_numpy(np.concatenate([SPECIAL_VALUES, SPECIAL_VALUES]))
    tbit = torch.cat([torch.zeros(k), torch.ones(k)])
    if C == 1:
        p, t = _random_binary(B, SPECIAL_SPATIAL, gen)
    else:
        p, t = _random_mc(B, C, SPECIAL_SPATIAL, gen)
    pf, tf = p.view(B, C, -1), t.view(B, C, -1)
    special = torch.zeros(pf.shape, dtype=torch.bool)
    special[:, :, :N_SPECIAL] = True
    if C == 1:
        pf[:, 0, :N_SPECIAL] = vals
        tf[:, 0, :N_SPECIAL] = tbit
    else:
        pf[:, 0, :N_SPECIAL] = vals
        pf[:, 1:, :N_SPECIAL] = ((1.0 - vals) / np.float32(C - 1))[None, None, :]
        tf[:, :, :N_SPECIAL] = 0.0
        tf[:, 0, :N_SPECIAL] = tbit
        tf[:, 1, :N_SPECIAL] = 1.0 - tbit
    return dict(p=p, t=t, r=_item_weights(B, gen), r2=_item_weights(B, gen),
                special=special.view(p.shape))


@functools.lru_cache(maxsize=None)
def large_case(C):
    gen = torch.Generator().manual_seed(200 + C)
    p, t = (_random_binary(LARGE_B, LARGE_SPATIAL, gen) if C == 1
            else _random_mc(LARGE_B, C, LARGE_SPATIAL, gen))
    return dict(p=p, t=t, r=torch.tensor([0.75, 1.5]), r2=torch.tensor([1.25, 0.5]))


@functools.lru_cache(maxsize=None)
def c32_case():
    gen = torch.Generator().manual_seed(232)
    p, t = _random_mc(2, SEGLOSS_MAX_C, C32_SPATIAL, gen)
    return dict(p=p, t=t, r=_item_weights(2, gen))


def ref_loss(fn, kw, case, dtype):
    """(value [B], d sum(value * r) / d p) of ``oracle.torch_ref.losses.<fn>`` on the CPU in ``dtype``."""
    p = case["p"].to(dtype).clone().requires_grad_(True)
    v = getattr(RL, fn)(p, case["t"].to(dtype), **kw).reshape(p.shape[0])
    (v * case["r"].to(dtype)).sum().backward()
    return v.detach(), p.grad


def ref_pair(dice_kw, focal_kw, case, dtype):
    """The dice + focal pair: ((dice [B], focal [B]), d (sum dice r + sum focal r2) / d p)."""
    p = case["p"].to(dtype).clone().requires_grad_(True)
    t = case["t"].to(dtype)
    dice = RL.binary_generalized_dice_loss(p, t, **dice_kw).reshape(-1)
    focal = RL.binary_focal_loss(p, t, **focal_kw).reshape(-1)
    ((dice * case["r"].to(dtype)).sum() + (focal * case["r2"].to(dtype)).sum()).backward()
    return (dice.detach(), focal.detach()), p.grad


def elementwise_bound(ref32, ref64):
    """|kernel - ref64| may reach 4 |ref32 - ref64| (elements the formula itself makes ill-conditioned
    in fp32, e.g. log(1 + eps)) + 2^-20 |ref64| (a handful of ulps for the others)."""
    return 4.0 * (ref32.double() - ref64).abs() + REL_FLOOR * ref64.abs()


def whole_allowed(ref32, ref64):
    """Whole-tensor rule: 4 x the fp32 CPU restatement's error against fp64 (max error over the largest
    magnitude), with a floor of 2^-20."""
    return max(4.0 * rel_err(ref32, ref64), REL_FLOOR)
