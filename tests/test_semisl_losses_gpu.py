"""Semi-supervised losses beyond LocalContrastiveLoss on the device (-m gpu): the fused kernels of
csrc/semisl.hip against the fixtures of the real reference and against the fp64 restatements of
tests/semisl_losses_ref.py at shapes that span several blocks and every launch path; the queue gather
bit for bit; the wrapper's anchor step; host synchronisation."""
import gc

import numpy as np
import pytest
import torch

import semisl_losses_cases as C
import semisl_losses_ref as R
from adell_mri_amd import functional as HF
from adell_mri_amd import ops
from adell_mri_amd.modules.activations import activation_factory
from adell_mri_amd.modules.semi_supervised_segmentation import (LocalContrastiveLossWithAnchors,
                                                                NearestNeighbourLoss,
                                                                PseudoLabelCrossEntropy,
                                                                UNetContrastiveSemiSL)
from adell_mri_amd.utils.utils import ExponentialMovingAverage
from cases import SEMISL_CASES
from oracle.weights import tensor_for
from test_semisl_losses import (_anchor_module_run, check_anchor_against_fixture,
                                check_pl_against_fixture, pl_module_run, run_nn_script)

pytestmark = pytest.mark.gpu
GOLD = C.GOLD


@pytest.fixture(scope="module")
def bounds():
    return C.bounds()


@pytest.fixture(scope="module", autouse=True)
def _return_cached_memory():
    """The multi-megabyte tensors of this module go back to the driver when it is done, garbage that
    still holds some included: tests that measure peak memory later in the session see no cached
    blocks of these sizes."""
    yield
    if torch.cuda.is_available():
        gc.collect()
        torch.cuda.empty_cache()


def _value_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    print(what, "value err", float(err.max()), "of", float(np.abs(ref).max()))
    assert (err <= C.VALUE_ATOL + C.VALUE_RTOL * np.abs(ref)).all(), (what, err.max())


def _grad_close(got, ref, what):
    got, ref = got.detach().cpu().numpy().astype(np.float64), ref.numpy()
    err, top = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(what, "grad err", err, "of", top)
    assert err <= C.GRAD_REL * top, (what, err, top)


# ---- anchor loss ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(C.ANCHOR_CASES))
def test_anchor_loss_matches_fixture(cuda, tag, bounds):
    assert HF.semisl_route("anchor", C=C.ANCHOR_CASES[tag]["shape"][1]) == "fused"
    loss, grads = _anchor_module_run(tag, cuda)
    assert tuple(loss.shape) == (C.ANCHOR_CASES[tag]["shape"][0],)
    check_anchor_against_fixture(tag, loss, grads, bounds)


def _anchor_inputs(shape, seed, zero_voxel=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    a1 = torch.randn(shape, generator=g) + 0.5 * x
    a2 = torch.randn(shape, generator=g) - 0.25 * x
    r = torch.rand(shape[0], generator=g) + 0.5
    if zero_voxel:      # a zero vector in each: the clamp of the cosine and its gradient
        x.flatten(2)[0, :, 1] = 0.0
        a1.flatten(2)[0, :, 2] = 0.0
        a2.flatten(2)[-1, :, 3] = 0.0
    return x, a1, a2, r


# under one block and odd; several blocks at the smallest C; C not a power of two; 2-D; more voxels
# than the 1024 blocks of an item cover in one round (16 voxels per block at C = 64)
@pytest.mark.parametrize("shape,temperature", [((3, 8, 3, 5, 7), 0.1), ((2, 4, 17, 16, 16), 0.1),
                                               ((2, 20, 9, 11, 13), 0.2), ((2, 8, 6, 10), 0.1),
                                               ((1, 64, 26, 26, 26), 0.1)])
@pytest.mark.parametrize("zero_voxel", [False, True])
def test_anchor_loss_matches_fp64_restatement(cuda, shape, temperature, zero_voxel):
    # (the gradient at a zero vector is of the order of 1 / 1e-8 and sets the scale of the comparison:
    # the other voxels are held to their own scale by the run without one)
    x, a1, a2, r = _anchor_inputs(shape, shape[1], zero_voxel=zero_voxel)
    ref, dx, da1, da2 = R.anchor_loss_and_grads(x, a1, a2, r, temperature)
    xh, a1h, a2h = (t.to(cuda).requires_grad_(True) for t in (x, a1, a2))
    val = HF.loco_anchor_loss(xh, a1h, a2h, temperature)
    (val * r.to(cuda)).sum().backward()
    _value_close(val.detach().cpu().numpy(), ref.numpy(), "anchor")
    _grad_close(xh.grad, dx, "dx")
    _grad_close(a1h.grad, da1, "da1")
    _grad_close(a2h.grad, da2, "da2")
    assert xh.grad.shape == xh.shape
    # bit-reproducible, forward and backward
    xb, a1b, a2b = (t.to(cuda).requires_grad_(True) for t in (x, a1, a2))
    again = HF.loco_anchor_loss(xb, a1b, a2b, temperature)
    (again * r.to(cuda)).sum().backward()
    assert torch.equal(val, again)
    assert torch.equal(xh.grad, xb.grad) and torch.equal(a1h.grad, a1b.grad)
    # detached anchors: only dx
    xc = x.to(cuda).requires_grad_(True)
    a1c, a2c = a1.to(cuda), a2.to(cuda)
    HF.loco_anchor_loss(xc, a1c, a2c, temperature).mul(r.to(cuda)).sum().backward()
    assert a1c.grad is None and a2c.grad is None
    assert torch.equal(xc.grad, xh.grad)


def test_anchor_loss_composed_route_on_device(cuda):
    x, a1, a2, r = _anchor_inputs((2, 6, 4, 5), 3)      # C % 4 != 0
    assert HF.semisl_route("anchor", C=6) == "composed"
    ref, dx, _, _ = R.anchor_loss_and_grads(x, a1, a2, r, 0.1)
    xh = x.to(cuda).requires_grad_(True)
    val = HF.loco_anchor_loss(xh, a1.to(cuda), a2.to(cuda), 0.1)
    (val * r.to(cuda)).sum().backward()
    _value_close(val.detach().cpu().numpy(), ref.numpy(), "anchor composed")
    _grad_close(xh.grad, dx, "dx composed")


# ---- nearest-neighbour loss -------------------------------------------------------------------------------
def test_nearest_neighbour_script_on_device(cuda, bounds):
    run_nn_script(cuda, bounds)


def _nn_inputs(shape, K, Q, seed, sorted_classes=True, absent=None):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    y = (torch.rand((shape[0], K) + tuple(shape[2:]), generator=g) > 0.5).float()
    past = torch.randn(Q, shape[1], generator=g)
    cls = torch.randint(0, K, (Q,), generator=g)
    if absent is not None:
        cls[cls == absent] = (absent + 1) % K
    if sorted_classes:
        cls = cls.sort().values
    return x, y, past, cls.to(torch.int32)


# Q = 3 (smaller than a tile of 32 and than a step of 4), K = 2, C = 8; Q = 37 (a tile and a ragged
# step), K = 5, C = 20, classes in queue order and shuffled, a class never queued; 315 voxels per item:
# odd, three forward and five backward blocks over the two items; C = 64, the widest
@pytest.mark.parametrize("shape,K,Q,sorted_classes,absent", [
    ((2, 8, 3, 5, 7), 2, 3, True, None),
    ((2, 20, 5, 7, 9), 5, 37, True, 3),
    ((2, 20, 5, 7, 9), 5, 37, False, None),
    ((1, 64, 9, 11), 3, 64, True, None),
])
def test_nn_queue_loss_matches_fp64_restatement(cuda, shape, K, Q, sorted_classes, absent):
    x, y, past, cls = _nn_inputs(shape, K, Q, Q + K, sorted_classes, absent)
    assert HF.semisl_route("nn", C=shape[1], K=K) == "fused"
    ref, dx = R.nn_loss_and_grad(x, y, past, cls, 0.1)
    xh = x.to(cuda).requires_grad_(True)
    args = (y.to(cuda), past.to(cuda), cls.to(cuda), 0.1)
    val = HF.nn_queue_loss(xh, *args)
    assert val.dim() == 0
    val.backward()
    _value_close(val.detach().cpu().numpy(), ref.numpy(), "nn")
    _grad_close(xh.grad, dx, "nn dx")
    xb = x.to(cuda).requires_grad_(True)
    again = HF.nn_queue_loss(xb, *args)
    again.backward()
    assert torch.equal(val, again) and torch.equal(xh.grad, xb.grad)


def test_nn_queue_loss_float_labels_and_temperature(cuda):
    """y is arbitrary float data: both exponentials are computed."""
    x, y, past, cls = _nn_inputs((2, 8, 4, 5, 3), 3, 10, 11)
    y = y * 0.7 + 0.1 * torch.rand(y.shape, generator=torch.Generator().manual_seed(5))
    ref, dx = R.nn_loss_and_grad(x, y, past, cls, 0.5)
    xh = x.to(cuda).requires_grad_(True)
    val = HF.nn_queue_loss(xh, y.to(cuda), past.to(cuda), cls.to(cuda), 0.5)
    val.backward()
    _value_close(val.detach().cpu().numpy(), ref.numpy(), "nn float labels")
    _grad_close(xh.grad, dx, "nn float labels dx")


def test_nn_queue_loss_nan_voxel(cuda):
    x, y, past, cls = _nn_inputs((2, 8, 3, 5, 7), 3, 9, 4)
    x.flatten(2)[1, :, 17] = float("nan")
    xh = x.to(cuda).requires_grad_(True)
    yh, ph, ch = y.to(cuda), past.to(cuda), cls.to(cuda)
    val = HF.nn_queue_loss(xh, yh, ph, ch, 0.1)
    val.backward()
    labels = torch.nn.functional.one_hot(ch.long(), 3)
    want = HF.nn_queue_loss_composite(x.to(cuda), yh, ph, labels, 0.1)
    assert torch.isfinite(val)
    _value_close(val.detach().cpu().numpy(), want.cpu().numpy(), "nn with a NaN voxel")
    grad = xh.grad.flatten(2)
    assert (grad[1, :, 17] == 0).all()
    keep = torch.ones(grad.shape[2], dtype=torch.bool, device=cuda)
    keep[17] = False
    assert torch.isfinite(grad[0]).all() and torch.isfinite(grad[1][:, keep]).all()
    assert float(grad.abs().max()) > 0


def test_nearest_neighbour_empty_queue_launches_nothing(cuda, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a kernel wrapper was called on an empty queue")
    for name in ("nn_queue_normalize", "nn_queue_loss_fwd", "nn_queue_count"):
        monkeypatch.setattr(ops, name, boom)
    mod = NearestNeighbourLoss(**C.NN_ARGS)
    X, y = (torch.from_numpy(v).to(cuda) for v in C.nn_forward_inputs())
    out = mod(X.requires_grad_(True), y)
    assert out.dim() == 0 and out.device.type == "cuda" and float(out) == 0.0


@pytest.mark.parametrize("channels_last", [False, True])
def test_nn_queue_put_gathers_the_reference_rows(cuda, channels_last):
    """Two counting chunks per item (8000 voxels), three classes of which one overflows, against the
    reference's own indexing on the device with a generator in the same state."""
    g = torch.Generator().manual_seed(9)
    X = torch.randn(2, 8, 20, 20, 20, generator=g).to(cuda)
    y = torch.zeros(2, 4, 20, 20, 20)
    y[:, 0] = (torch.rand(2, 20, 20, 20, generator=g) > 0.5).float()
    flat = y.flatten(2)                 # a view
    flat[0, 1, [5, 4097, 7999]] = 1.0
    flat[1, 1, [0, 4095, 4096]] = 2.5
    flat[:, 2] = -1.0
    flat[1, 3, 7999] = 1.0
    y = y.to(cuda)
    if channels_last:
        X = X.contiguous(memory_format=torch.channels_last_3d)
    mod = NearestNeighbourLoss(maxsize=4, n_classes=4, max_elements_per_batch=50, n_samples_per_class=1,
                               seed=3)
    mod.put(X, y)
    rng = np.random.default_rng(3)
    Xf, yf = X.flatten(2), y.flatten(2)
    b, c, v = torch.where(yf > 0)
    for cl in range(4):
        idx = c == cl
        want = Xf[b[idx], :, v[idx]]
        if want.shape[0] > 50:
            want = want[rng.choice(want.shape[0], 50)]
        if want.shape[0] == 0:
            assert mod.q[cl].qsize() == 0
            continue
        got = mod.q[cl].queue[0]
        assert got.is_contiguous() and torch.equal(got, want), cl
    assert [q.qsize() for q in mod.q] == [1, 1, 0, 1]


# ---- pseudo-label cross entropy ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.PL_CASES))
def test_pseudo_label_ce_matches_fixture(cuda, name, bounds):
    loss, grad = pl_module_run(name, cuda)
    assert loss.dim() == 0
    check_pl_against_fixture(name, loss, grad, bounds)


# the issue's shape at K = 2, 3, 5; 63 blocks; more voxels than the 4096 blocks cover in one round
@pytest.mark.parametrize("shape", [(2, 2, 5, 7, 3), (2, 3, 5, 7, 3), (2, 5, 5, 7, 3), (2, 3, 20, 20, 20),
                                   (1, 2, 102, 102, 102)])
def test_pseudo_label_ce_matches_fp64_restatement(cuda, shape):
    g = torch.Generator().manual_seed(shape[1] + shape[2])
    pred = 3 * torch.randn(shape, generator=g)
    proba = torch.rand(shape, generator=g)
    weight = torch.rand(shape[1], generator=g) + 0.5
    for kw in (dict(), dict(weight=weight, label_smoothing=0.05, reduction="sum")):
        ref, d = R.pseudo_label_ce_and_grad(pred, proba, 0.6, **kw)
        ph = pred.to(cuda).requires_grad_(True)
        kwh = dict(kw, weight=weight.to(cuda)) if "weight" in kw else kw
        val = HF.pseudo_label_ce(ph, proba.to(cuda), 0.6, **kwh)
        val.backward()
        _value_close(val.detach().cpu().numpy(), ref.numpy(), f"pl {kw.get('reduction', 'mean')}")
        _grad_close(ph.grad, d, "pl d pred")
        pb = pred.to(cuda).requires_grad_(True)
        again = HF.pseudo_label_ce(pb, proba.to(cuda), 0.6, **kwh)
        again.backward()
        assert torch.equal(val, again) and torch.equal(ph.grad, pb.grad)


def test_pseudo_label_ce_reduction_none_is_composed(cuda):
    pred, proba = (torch.from_numpy(v).to(cuda) for v in C.pl_inputs())
    assert HF.semisl_route("pseudo_label", K=pred.shape[1], reduction="none") == "composed"
    mod = PseudoLabelCrossEntropy(C.PL_THRESHOLD, reduction="none")
    got = mod(pred, proba)
    want = torch.nn.functional.cross_entropy(pred, (proba > C.PL_THRESHOLD).float(), reduction="none")
    assert got.shape == (2, 5, 7, 3) and torch.equal(got, want)


# ---- the wrapper ------------------------------------------------------------------------------------------
def test_step_semi_sl_with_anchors(cuda):
    name = "unet2d_semisl"
    kw = dict(SEMISL_CASES[name])
    kw["activation_fn"] = activation_factory[kw["activation_fn"]]
    ema = ExponentialMovingAverage(decay=0.9, final_decay=1.0, n_steps=10)
    net = UNetContrastiveSemiSL(loss_fn_semi_sl=LocalContrastiveLossWithAnchors(), ema=ema, **kw)
    sd = {k: torch.from_numpy(tensor_for(k, v.shape)) if v.numel() > 0 else v
          for k, v in net.state_dict().items() if "shadow" not in k}
    net.load_state_dict(sd, strict=False)
    net = net.to(cuda).eval()
    seen = []

    def recording(fn):
        def wrapped(**kwargs):
            out = fn(**kwargs)
            seen.append(out)
            return out
        return wrapped

    net.forward_features = recording(net.forward_features)
    net.ema.shadow.forward_features = recording(net.ema.shadow.forward_features)
    g = torch.Generator().manual_seed(4)
    x, x_1, x_2 = (torch.rand(2, 1, 16, 16, generator=g).to(cuda) for _ in range(3))
    out = net.step_semi_sl(x, x_1, x_2, None, None)
    assert len(seen) == 3
    anchor_1, anchor_2, features = seen
    assert not anchor_1.requires_grad and not anchor_2.requires_grad and features.requires_grad
    want = net.ssl_weight * R.anchor_loss(*(t.detach().cpu().double() for t in (features, anchor_1,
                                                                                 anchor_2)), 0.1).mean()
    _value_close(out.detach().cpu().numpy(), want.numpy(), "step_semi_sl")
    out.backward()
    grads = [p.grad for k, p in net.named_parameters() if "shadow" not in k and p.grad is not None]
    assert len(grads) > 4 and all(torch.isfinite(gr).all() for gr in grads)
    assert any(float(gr.abs().max()) > 0 for gr in grads)
    assert all(p.grad is None for p in net.ema.shadow.parameters())


# ---- synchronisation --------------------------------------------------------------------------------------
class _no_sync:
    def __enter__(self):
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *exc):
        torch.cuda.set_sync_debug_mode("default")
        return False


def test_fused_losses_read_nothing_on_the_host(cuda):
    x, a1, a2, r = (t.to(cuda) for t in _anchor_inputs((2, 8, 5, 6, 7), 1))
    x.requires_grad_(True)
    a1.requires_grad_(True)
    pred = torch.randn(2, 3, 5, 6, 7, device=cuda, requires_grad=True)
    proba = torch.rand(2, 3, 5, 6, 7, device=cuda)
    weight = torch.ones(3, device=cuda)
    xn, y, past, cls = (t.to(cuda) for t in _nn_inputs((2, 8, 5, 6, 7), 3, 12, 2))
    xn.requires_grad_(True)
    mod = NearestNeighbourLoss(**C.NN_ARGS)
    for i in range(2):                          # put is allowed its one host read
        X, yy = (torch.from_numpy(v).to(cuda) for v in C.nn_put_inputs(i))
        mod.put(X, yy)
    with _no_sync():
        (HF.loco_anchor_loss(x, a1, a2, 0.1) * r).sum().backward()
        HF.pseudo_label_ce(pred, proba, 0.5, weight, 0.1, "mean").backward()
        HF.nn_queue_loss(xn, y, past, cls, 0.1).backward()
    torch.cuda.synchronize()
    assert x.grad is not None and a1.grad is not None and pred.grad is not None and xn.grad is not None
    # the module's forward reads nothing either once the queue has been drained and concatenated
    past_samples, classes = mod._past_samples()
    past_class = torch.as_tensor(classes.astype(np.int32), device=cuda)
    X, yy = (torch.from_numpy(v).to(cuda) for v in C.nn_forward_inputs())
    X.requires_grad_(True)
    with _no_sync():
        HF.nn_queue_loss(X, yy, past_samples, past_class, mod.temperature).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(X.grad).all()
