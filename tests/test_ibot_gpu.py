"""iBOT on the GPU (csrc/ibot.hip): the mask-token splice, the token sums and the centre sum derived
from them, the fused per-view losses (both reductions, both teacher modes, forward and the
one-writer backward) against the fp64 restatement (tests/ibot_ref.py, pinned to the real reference by
tests/test_ibot.py) and against the composed path, and one training step of two networks through
``iBOTPL.training_step`` and ``FusedAdamW`` against tests/golden/ibot_step.npz.

Inputs follow test_dino_gpu.make_inputs: uniform in [-1, 1], the seed walked until the largest
teacher probability at t2 = 0.04 is below 0.9 -- for the views over at most 16 seeds
(``make_view_inputs``). Every kernel result is computed twice and compared
bit for bit. Tolerances: splice exact, the token's gradient < 5e-5 of its largest entry; token sums
< 1e-5 of the largest entry, the centre sum rtol 1e-4 (test_dino_gpu.py's bound on ``center_sum``);
losses rtol 1e-5, gradients and reduced outputs < 5e-5 of the largest entry (DINO's loss bounds);
the step bounds of test_dino_gpu.py::test_training_step_matches_reference."""
import functools

import numpy as np
import pytest
import torch

import dino_ref as R
import ibot_ref as IR
from cases import grad_rel_err
from ibot_cases import NETS, StepGold, step_config
from oracle.weights import fill_state_dict
from test_dino_gpu import make_inputs, rel

pytestmark = pytest.mark.gpu

T0, T1 = (0.1, 0.04), (0.1, 0.1)


# ---- splice -----------------------------------------------------------------------------------------
def _splice_idx(N, M, kind):
    if kind == "all":
        return np.arange(N)
    if kind == "offset":                 # shifted by 3 (registers + class token), up to row N - 1
        return np.unique(np.concatenate([np.arange(M - 1) * 2 + 3, [N - 1]]))
    return np.unique(np.linspace(0, N - 1, M).astype(np.int64))


@pytest.mark.parametrize("B,N,E,M,kind", [(1, 1, 1, 1, "spread"), (3, 7, 5, 3, "spread"),
                                          (2, 67, 64, 67, "all"), (3, 19, 250, 6, "offset")])
def test_mask_token_splice(cuda, B, N, E, M, kind):
    from adell_mri_amd import functional as HF

    idx = _splice_idx(N, M, kind)
    assert len(idx) == M and (kind != "offset" or (idx[0] == 3 and idx[-1] == N - 1))
    g = torch.Generator().manual_seed(B * N * E + M)
    x = torch.rand((B, N, E), generator=g) * 2 - 1
    token = torch.rand((E,), generator=g)
    r = torch.rand((B, N, E), generator=g) * 2 - 1
    xr, tr = x.double().requires_grad_(True), token.double().requires_grad_(True)
    yr = IR.splice(xr, idx, tr)
    (yr * r.double()).sum().backward()
    outs = []
    for _ in range(2):
        xd, td = x.to(cuda).requires_grad_(True), token.to(cuda).requires_grad_(True)
        yd = HF.mask_tokens(xd, idx, td)
        assert yd.data_ptr() != xd.data_ptr()                      # out of place
        (yd * r.to(cuda)).sum().backward()
        outs.append((yd.detach(), xd.grad, td.grad))
    yd, dx, dtoken = outs[0]
    assert torch.equal(yd.cpu(), yr.detach().float()) and torch.equal(xd.detach().cpu(), x)
    assert torch.equal(dx.cpu(), xr.grad.float())
    err = rel(dtoken, tr.grad)
    print((B, N, E, M), f"dtoken {err:.2e}")
    assert err < 5e-5
    for u, v in zip(*outs):
        assert torch.equal(u, v)


# ---- token sums ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Tt,K,first", [(1, 1, 5, 0), (3, 7, 37, 1), (2, 64, 300, 0),
                                          (2, 9, 4099, 1), (1, 216, 1025, 0)])
def test_token_sums_and_the_centre_sum(cuda, B, Tt, K, first):
    from adell_mri_amd import ops

    _, y1, _ = make_inputs((B, Tt, K))
    _, y2, _ = make_inputs((B, Tt, K), seed=B * Tt * K + 1000)
    T = Tt - first
    want_mean = IR.token_sums(y1.double(), first, 1.0 / T)
    want_raw = IR.token_sums(y1.double(), first)
    want_center, rows = IR.mask_center_sum(y1.double(), y2.double(), first)
    assert rows == 2 * B * T
    outs = []
    for _ in range(2):
        sums = torch.empty((2 * B, K), device=cuda, dtype=torch.float64)
        mean, raw = ops.ibot_token_sums(y1.to(cuda), first, 1.0 / T, raw_out=sums[:B])
        other, _ = ops.ibot_token_sums(y2.to(cuda), first, want_raw=True, raw_out=sums[B:])
        assert raw.data_ptr() == sums.data_ptr()
        outs.append((mean, raw.clone(), other, ops.ibot_center_sum(sums)))
    mean, raw, other, center = outs[0]
    errs = dict(mean=rel(mean, want_mean), raw=rel(raw, want_raw))
    print((B, Tt, K, first), ops.ibot_token_sums_plan(B, T, K), {k: f"{v:.2e}" for k, v in errs.items()},
          "centre", f"{float(((center.cpu().double() - want_center).abs() / want_center.abs()).max()):.2e}")
    assert tuple(mean.shape) == (B, K) and tuple(center.shape) == (1, K)
    assert errs["mean"] < 1e-5 and errs["raw"] < 1e-5
    np.testing.assert_allclose(center.cpu().numpy(), want_center.numpy(), rtol=1e-4)
    for u, v in zip(*outs):
        assert torch.equal(u, v)


# ---- fused per-view losses ---------------------------------------------------------------------------
def _rows(T, kind):
    if kind == "one":
        return np.array([T // 2])
    if kind == "all":
        return np.arange(T)
    if isinstance(kind, int):            # that many rows, spread, the last one among them
        return np.unique(np.linspace(0, T - 1, kind).astype(np.int64))
    return np.unique(np.array([0, T // 3, T - 1]))      # "few"


def make_view_inputs(shape, tries=16):
    """test_dino_gpu.make_inputs with a bounded walk. That rule keeps the largest teacher probability
    below 0.9 because the TEACHER's gradient is a difference of nearly equal numbers beyond it; with
    a few hundred rows of a few dozen columns (8 x 80 rows of 33) every seed has a sharper row and
    the walk would not end. The view gives the teacher no gradient, so after ``tries`` seeds the
    first one is taken; the bounds on the loss and on ds stay what they are."""
    first = int(np.prod(shape))
    for seed in range(first, first + tries):
        g = torch.Generator().manual_seed(seed)
        a = torch.rand(shape, generator=g) * 2 - 1
        b = torch.rand(shape, generator=g) * 2 - 1
        centers = 0.2 * (torch.rand((shape[-1],), generator=g) * 2 - 1)
        if float(torch.softmax((b.double() - centers.double()) / 0.04, -1).max()) < 0.9:
            return a, b, centers
    return make_view_inputs(shape, tries=1) if tries > 1 else (a, b, centers)


# (B, Tt, K, rows, class token, reduce, teacher mode, temperatures)
VIEWS = [
    (1, 1, 5, "one", False, "mean", "center", T0),
    (3, 7, 37, "few", True, "cls", "center", T0),
    (3, 7, 37, "all", False, "mean", "sk", T1),
    (1, 20, 300, "few", True, "mean", "sk", T0),
    (3, 20, 1025, "all", True, "cls", "center", T1),
    (3, 20, 300, "one", False, "mean", "center", T0),
    (1, 7, 1025, "few", False, "mean", "sk", T1),
    (3, 20, 37, "few", True, "cls", "sk", T0),
    (1, 3, 65537, "all", True, "cls", "center", T0),      # (B, M, K) = (1, 2, 65537): rows in chunks
    (1, 2, 65537, "all", False, "mean", "sk", T0),
    (8, 80, 33, 70, False, "mean", "center", T0),         # 560 rows, one chunk each, unaligned rows
    (8, 80, 33, 70, False, "mean", "sk", T1),
]


@functools.lru_cache(maxsize=None)
def view_reference(case):
    """fp64 restatement on the fp32 inputs, computed once: loss, s_red, ds of the loss alone, ds of
    loss + sum(s_red * w)."""
    B, Tt, K, kind, cls, reduce_fn, method, temps = case
    s, y, centers = make_view_inputs((B, Tt, K))
    w = make_inputs((B, K), seed=B * K + 7)[0]
    m = _rows(Tt - int(cls), kind)
    out = []
    for with_red in (False, True):
        x = s.double().requires_grad_(True)
        s_red, loss = IR.view(x, y.double(), m, centers.double(), temps[0], temps[1], cls, reduce_fn,
                              method)
        (loss + (s_red * w.double()).sum() if with_red else loss).backward()
        out.append(x.grad)
    return loss.item(), s_red.detach(), out[0], out[1]


def run_view(cuda, case, composed=False):
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.self_supervised.losses import DinoLoss

    B, Tt, K, kind, cls, reduce_fn, method, temps = case
    s, y, centers = make_view_inputs((B, Tt, K))
    w = make_inputs((B, K), seed=B * K + 7)[0].to(cuda)
    c = int(cls)
    m = _rows(Tt - c, kind)
    crit = DinoLoss(temps, K, teacher_score_method=method).to(cuda)
    crit.centers.copy_(centers)
    res = []
    for with_red in (False, True):
        x = s.to(cuda).requires_grad_(True)
        t = y.to(cuda).requires_grad_(True)
        if composed:      # gathered rows through the dense loss, a torch mean
            idx = torch.as_tensor(m + c, device=cuda)
            loss = crit(x[:, idx], t.detach()[:, idx])
            s_red = x[:, 0] if reduce_fn == "cls" else x[:, c:].mean(1)
        elif method == "center":
            s_red, loss = HF.ibot_view(x, t, m, crit.centers, temps[0], temps[1], cls, reduce_fn)
        else:
            table = HF.patch_rows(m, Tt, c, cuda)
            scores = crit.sinkhorn_knopp_teacher(t.detach().index_select(1, table.dev))
            s_red, loss = HF.ibot_view(x, t, table, scores, temps[0], temps[1], cls, reduce_fn,
                                       teacher_is_scores=True)
        (loss + (s_red * w).sum() if with_red else loss).backward()
        assert t.grad is None                                   # the teacher receives no gradient
        res.append(x.grad)
    return loss.detach(), s_red.detach(), res[0], res[1]


def check_view(got, want, tag):
    wl, wred, wds0, wds1 = want
    loss, s_red, ds0, ds1 = got
    errs = dict(loss=abs(loss.item() - float(wl)) / abs(float(wl)), s_red=rel(s_red, wred),
                ds_loss=rel(ds0, wds0), ds=rel(ds1, wds1))
    print(tag, {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["loss"] < 1e-5, (tag, errs)
    for k in ("s_red", "ds_loss", "ds"):
        assert errs[k] < 5e-5, (tag, errs)
    assert ds1.shape == wds1.shape and s_red.shape == wred.shape


@pytest.mark.parametrize("case", VIEWS, ids=lambda c: "-".join(str(v) for v in c[:7]) + f"-t2={c[7][1]}")
def test_view_losses_match_fp64(cuda, case):
    B, Tt, K, kind, cls, reduce_fn, method, temps = case
    got = run_view(cuda, case)
    check_view(got, view_reference(case), str(case))
    again = run_view(cuda, case)                                # bit for bit
    for u, v in zip(got, again):
        assert torch.equal(u, v)
    c = int(cls)
    m = _rows(Tt - c, kind)
    unmasked = np.setdiff1d(np.arange(Tt - c), m) + c
    if reduce_fn == "cls" and len(unmasked):                    # exact zeros: written, not left over
        for ds in got[2:]:
            assert float(ds[:, torch.as_tensor(unmasked, device=cuda)].abs().max()) == 0.0
    if len(unmasked):                                           # the loss alone: zero off the mask
        off = np.concatenate([unmasked, np.arange(c)])
        assert float(got[2][:, torch.as_tensor(off, device=cuda)].abs().max()) == 0.0
    # the composed path -- rows gathered, the dense loss, a torch mean -- gives the same values
    wl, wred, wds0, wds1 = run_view(cuda, case, composed=True)
    check_view(got, (wl.item(), wred, wds0, wds1), "composed " + str(case))


def test_view_refuses_rows_beyond_the_patch_tokens(cuda):
    from adell_mri_amd import functional as HF

    s = torch.zeros((2, 7, 8), device=cuda)
    with pytest.raises(IndexError):
        HF.ibot_view(s, s, [2, 6], torch.zeros(8, device=cuda), 0.1, 0.1, True, "cls")
    with pytest.raises(IndexError):
        HF.mask_tokens(s, [7], torch.zeros(8, device=cuda))


# ---- one training step -------------------------------------------------------------------------------
LOSS_KEYS = ("ema.", "loss_mask.", "loss_global.")


def build_pl(name, cuda):
    """iBOTPL of one fixture network: weights from fill_state_dict, the fixture's centres, then a
    fresh teacher made from those weights (as the constructor makes it from the initial ones)."""
    from adell_mri_amd.modules.self_supervised.pl import iBOTPL
    from adell_mri_amd.utils import ExponentialMovingAverage

    g = StepGold(name)
    net = iBOTPL(aug_image_key_1="a", aug_image_key_2="b", ema=ExponentialMovingAverage(0.99),
                 temperature=float(g.top["temperature"]), centers_m=float(g.top["center_m"]),
                 **step_config(name))
    own = {k: v for k, v in net.state_dict().items() if not k.startswith(LOSS_KEYS)}
    assert list(own) == [str(k) for k in g["state_keys"]]
    net.load_state_dict(fill_state_dict(own, gain=float(g["gain"])), strict=False)
    net.last_layer_.parametrizations.weight.original0.requires_grad = False
    net.loss_mask.centers.copy_(torch.from_numpy(g["mask:centers0"]))
    net.loss_global.centers.copy_(torch.from_numpy(g["global:centers0"]))
    net = net.to(cuda).train()
    net.ema = ExponentialMovingAverage(float(g.top["ema_decay"]))
    net.ema.update(net, exclude_keys=["centers"])
    batch = {"a": torch.from_numpy(g["x1"]).to(cuda), "b": torch.from_numpy(g["x2"]).to(cuda)}
    return net, g, batch


def own_parameters(net):
    return [(k, p) for k, p in net.named_parameters() if not k.startswith("ema.")]


def fresh_masker(net):
    net.patch_masker_.rng = np.random.default_rng(net.seed)


def check_centres(net, g):
    for which, crit in (("mask", net.loss_mask), ("global", net.loss_global)):
        assert crit.updated is True                     # applied inside the first loss call
        np.testing.assert_allclose(crit.async_batch_center.cpu().numpy(), g[f"{which}:center_sum"],
                                   rtol=1e-4, err_msg=which)
        np.testing.assert_allclose(crit.centers.cpu().numpy(), g[f"{which}:centers1"], rtol=1e-4,
                                   err_msg=which)
    B, T = int(g.top["B"]), int(g["patch_tokens"])
    assert net.loss_mask.len_teacher_output == 2 * B * T and net.loss_global.len_teacher_output == 2 * B


@pytest.mark.parametrize("name", NETS)
def test_training_step_matches_reference(cuda, name):
    """The student on both views with two consecutive masker draws, the teacher without masking, the
    centre updates before the losses, both losses, every parameter gradient (the mask token's among
    them), one AdamW step and the EMA update (self_supervised/pl.py:1370-1419). As in the DINO step
    test the fixture's EMA is reached by one more ``ema.update`` after the optimiser step."""
    from adell_mri_amd.trainer import StepRunner

    net, g, batch = build_pl(name, cuda)
    B = int(g.top["B"])
    with torch.no_grad():       # the student's outputs with the step's two draws, then the draws again
        for view, key in enumerate(("a", "b")):
            s_red, s_tok, mc = net.forward_training(batch[key], mask=True)
            np.testing.assert_array_equal(mc, g[f"coords{view}"])
            assert rel(s_tok, g["student_tokens"][view * B:(view + 1) * B]) < 1e-4
            assert rel(s_red, g["student_red"][view * B:(view + 1) * B]) < 1e-4
            t_red, t_tok = net.ema.shadow.forward_training(batch[key])
            assert rel(t_tok, g["teacher_tokens"][view * B:(view + 1) * B]) < 1e-4
            assert rel(t_red, g["teacher_red"][view * B:(view + 1) * B]) < 1e-4
    fresh_masker(net)
    runner = StepRunner(net)
    runner.optimizer.zero_grad()
    loss = net.training_step(batch, 0)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-4)
    np.testing.assert_allclose(net.last_losses[0].item(), g["loss_mask"], rtol=1e-4)
    np.testing.assert_allclose(net.last_losses[1].item(), g["loss_global"], rtol=1e-4)
    _, further = net.patch_masker_(torch.zeros((1, 4, 2)), n_patches=net.n_patches)
    np.testing.assert_array_equal(np.unique(np.concatenate(further) + net.extra_tokens), g["coords2"])
    loss.backward()
    seen = 0
    for k, p in own_parameters(net):
        if "grad:" + k in g.files:
            assert grad_rel_err(g, k, p.grad.cpu().numpy()) < 5e-3, k
            seen += 1
        else:       # the frozen magnitude; the embedding's unused way back to patches
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
    assert seen == sum(k.startswith("grad:") for k in g.files)
    check_centres(net, g)
    runner.optimizer.step()
    net.ema.update(net, exclude_keys=["centers"])
    for k, p in own_parameters(net):
        np.testing.assert_allclose(p.detach().cpu().numpy(), g["step1:" + k], rtol=2e-4, atol=2e-6,
                                   err_msg=k)
    shadow = dict(net.ema.shadow.named_parameters())
    for k, _ in own_parameters(net):
        np.testing.assert_allclose(shadow[k].detach().cpu().numpy(), g["ema1:" + k], rtol=1e-5,
                                   atol=1e-7, err_msg=k)


def test_validation_step_updates_the_centres_but_not_the_ema(cuda):
    net, g, batch = build_pl("net3d", cuda)
    before = {k: p.detach().clone() for k, p in net.ema.shadow.named_parameters()}
    ema_steps = net.ema.step
    with torch.no_grad():
        loss = net.validation_step(batch, 0)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-4)
    assert net.ema.step == ema_steps
    for k, p in net.ema.shadow.named_parameters():
        assert torch.equal(p, before[k]), k
    check_centres(net, g)
    # the composed methods give the step's values on their own
    fresh_masker(net)
    with torch.no_grad():
        s_red, s_tok, mc = net.forward_training(batch["a"], mask=True)
        t_red, t_tok = net.ema.shadow.forward_training(batch["a"])
        composed = net.calculate_loss_mask(s_tok, t_tok, mc)
        crit, c = net.loss_mask, net.class_token
        want = R.dino_loss(s_tok.double().cpu()[:, mc], t_tok.double().cpu()[:, mc],
                           crit.centers.double().cpu(), crit.t1, crit.t2)
        np.testing.assert_allclose(composed.item(), want.item(), rtol=1e-5)
        assert net.calculate_loss_global(s_red, t_red).ndim == 0
        with pytest.raises(IndexError):
            net.calculate_loss_mask(s_tok, t_tok, np.array([0, s_tok.shape[1]]))
    assert net.ema.step == ema_steps
