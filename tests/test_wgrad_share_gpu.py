"""The share hint of the z-ring weight gradient on the device: the runtime gives the hinted launch one
block per CU and the plain one two; the hinted call returns the plain call's bits at the shapes of
test_wgrad_zring_shape_gpu.py (badly scaled operands, 3e-6 of fp64) and on a split-row source; a
hinted launch on a second stream beside a forward conv leaves both results what they are alone; a
training step is bit-identical with FLAGS["no_wgrad_share"] on and off."""
import ctypes

import pytest
import torch

from adell_mri_amd import _lib, ops

pytestmark = pytest.mark.gpu

TOL = 3e-6                   # tests/test_wgrad_zring_shape_gpu.py
NONE, AUTO, ALWAYS = 0, 1, 2

# n, c0, c1, cout, (D, H, W), pad -- from test_wgrad_zring_shape_gpu.CASES
CASES = [
    (1, 32, 0, 32, (6, 16, 24), 1),
    (1, 32, 0, 64, (9, 17, 33), 1),
    (1, 16, 16, 32, (9, 17, 33), 1),
    (2, 32, 0, 32, (24, 16, 16), 1),
]


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


def test_occupancy_is_one_block_per_cu_with_the_hint_and_two_without(cuda):
    """hipOccupancyMaxActiveBlocksPerMultiprocessor for the kernel with the LDS each launch requests
    (no kernel runs)."""
    L = _lib.lib()
    big = ops.make_conv_desc(2, (128, 128, 128), 32, 32, 32, 3, 1, 1)  # AUTO is accepted
    small = ops.make_conv_desc(1, (6, 16, 24), 32, 0, 32, 3, 1, 1)     # six blocks: AUTO is refused
    assert L.adell_wgrad_zring_occupancy(ctypes.byref(big), NONE) == 2
    assert L.adell_wgrad_zring_occupancy(ctypes.byref(big), AUTO) == 1
    assert L.adell_wgrad_zring_occupancy(ctypes.byref(big), ALWAYS) == 1
    assert L.adell_wgrad_zring_occupancy(ctypes.byref(small), NONE) == 2
    assert L.adell_wgrad_zring_occupancy(ctypes.byref(small), AUTO) == 2
    assert L.adell_wgrad_zring_occupancy(ctypes.byref(small), ALWAYS) == 1


@pytest.mark.parametrize("n,c0,c1,cout,size,pad", CASES)
def test_hinted_call_returns_the_plain_bits(cuda, n, c0, c1, cout, size, pad):
    g = torch.Generator().manual_seed(7 * c0 + cout + size[1] + pad)
    D, H, W = size
    Do, Ho, Wo = (s + 2 * pad - 2 for s in size)
    cin = c0 + c1
    x = torch.randn(n, cin, D, H, W, generator=g) * 37.0
    dy = torch.randn(n, cout, Do, Ho, Wo, generator=g) * 3e-4
    p = ops.conv3d_bwd_weight_share_plan(n, size, c0, c1, cout, 3, 1, pad, ALWAYS)
    assert p is not None and p.zring[7] == 0 and p.blocks_per_cu == 1, "the hint must be taken here"

    dw_ref = torch.nn.grad.conv3d_weight(x.double(), (cout, cin, 3, 3, 3), dy.double(), padding=pad)
    db_ref = dy.double().sum(dim=(0, 2, 3, 4))
    x0 = ops.ndhwc(x[:, :c0].contiguous().to(cuda))
    x1 = ops.ndhwc(x[:, c0:].contiguous().to(cuda)) if c1 else None
    dyd = ops.ndhwc(dy.to(cuda))

    def run(share):
        return ops.conv3d_bwd_weight(x0, dyd, 3, 1, pad, x1=x1, want_db=True, f16x3=True, share=share)

    dw, db = run(False)
    for share in (ALWAYS, True):
        dws, dbs = run(share)
        assert torch.equal(dws, dw) and torch.equal(dbs, db), share
    e_w, e_b = _rel(dws.cpu().double(), dw_ref), _rel(dbs.cpu().double(), db_ref)
    print(f"zring32 shared, fp64 parity {n}x({c0}+{c1})->{cout} {size}: dW {e_w:.3e} db {e_b:.3e}")
    assert e_w < TOL
    assert e_b < TOL


def test_hinted_call_on_a_split_row_source(cuda):
    """(1 x (32 + 32) -> 64 at 48 x 48 x 44, of tests/test_split_rows_gpu.py: both sources as rows)"""
    N, C0, C1, Cout, size = 1, 32, 32, 64, (48, 48, 44)
    assert ops.conv3d_bwd_weight_rows_ok(N, size, C0, C1, Cout, 3, 1, 1)
    assert ops.conv3d_bwd_weight_share_plan(N, size, C0, C1, Cout, 3, 1, 1, ALWAYS).blocks_per_cu == 1
    g = torch.Generator().manual_seed(5)
    x0 = ops.ndhwc((torch.randn(N, C0, *size, generator=g) * 1.5).to(cuda))
    x1 = ops.ndhwc(torch.randn(N, C1, *size, generator=g).to(cuda))
    dy = ops.ndhwc((torch.randn(N, Cout, *size, generator=g) * 0.01).to(cuda))
    r0, s0 = ops.rows_from_f32(x0, 9)
    r1, s1 = ops.rows_from_f32(x1, 10)
    before = ops.ROWS_FALLBACKS[0]
    kw = dict(x1=r1, want_db=True, f16x3=True, rows0=s0, rows1=s1)
    dw, db = ops.conv3d_bwd_weight(r0, dy, 3, 1, 1, **kw)
    for share in (ALWAYS, True):
        dws, dbs = ops.conv3d_bwd_weight(r0, dy, 3, 1, 1, share=share, **kw)
        assert torch.equal(dws, dw) and torch.equal(dbs, db), share
    assert ops.ROWS_FALLBACKS[0] == before


def test_hinted_launch_beside_a_forward_conv(cuda):
    """1 x 32 -> 32 at 16^3: the weight gradient, hinted, on a second stream while the current stream
    runs f16x3 forward convs; both equal their serial values."""
    g = torch.Generator().manual_seed(3)
    size = (16, 16, 16)
    x = ops.ndhwc((torch.randn(1, 32, *size, generator=g) * 1.5).to(cuda))
    dy = ops.ndhwc((torch.randn(1, 32, *size, generator=g) * 0.01).to(cuda))
    w = (torch.randn(32, 32, 3, 3, 3, generator=g) * 0.05).to(cuda)
    b = torch.randn(32, generator=g).to(cuda)
    wp = ops.pack_weight_f16x3(w, 0)
    assert ops.conv3d_bwd_weight_share_plan(1, size, 32, 0, 32, 3, 1, 1, ALWAYS).blocks_per_cu == 1

    y_ref, _ = ops.conv3d_fwd(x, wp, b, 32, 3, 1, 1)
    dw_ref, db_ref = ops.conv3d_bwd_weight(x, dy, 3, 1, 1, want_db=True, f16x3=True)
    torch.cuda.synchronize()

    main, side = torch.cuda.current_stream(), torch.cuda.Stream(device=cuda)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        grads = [ops.conv3d_bwd_weight(x, dy, 3, 1, 1, want_db=True, f16x3=True, share=ALWAYS)
                 for _ in range(4)]
    ys = [ops.conv3d_fwd(x, wp, b, 32, 3, 1, 1)[0] for _ in range(8)]
    main.wait_stream(side)
    torch.cuda.synchronize()
    for y in ys:
        assert torch.equal(y, y_ref)
    for dw, db in grads:
        assert torch.equal(dw, dw_ref) and torch.equal(db, db_ref)


def _train_step(cuda, kw, shape, flag, monkeypatch):
    from adell_mri_amd import functional as HF
    from adell_mri_amd.modules.activations import activation_factory
    from adell_mri_amd.modules.segmentation.losses import (CompoundLoss, binary_focal_loss,
                                                           binary_generalized_dice_loss)
    from adell_mri_amd.modules.segmentation.pl import UNetPL
    from adell_mri_amd.trainer import StepRunner
    from oracle.weights import tensor_for

    monkeypatch.setitem(HF.FLAGS, "no_wgrad_share", flag)
    kw = dict(kw)
    kw["activation_fn"] = activation_factory[kw["activation_fn"]]
    kw["dropout_param"] = 0.0
    loss_fn = CompoundLoss([(binary_generalized_dice_loss, {"smooth": 1e-5, "eps": 1e-6}),
                            (binary_focal_loss, {"gamma": 1.0, "eps": 1e-6})])
    net = UNetPL(image_key="image", label_key="mask", learning_rate=5e-4, weight_decay=5e-3,
                 loss_fn=loss_fn, **kw)
    net.load_state_dict({k: torch.from_numpy(tensor_for(k, v.shape))
                         for k, v in net.state_dict().items()})
    net = net.to(cuda).train()
    g = torch.Generator().manual_seed(1)
    batch = {"image": torch.rand((shape[0], kw["in_channels"], *shape[1:]), generator=g).to(cuda),
             "mask": (torch.rand((shape[0], 1, *shape[1:]), generator=g) > 0.9).float().to(cuda)}
    loss = StepRunner(net).train_step(batch)
    torch.cuda.synchronize()
    return float(loss.detach()), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


# the small U-Net of tests/test_train_gpu.py (8 / 16 channels: every hint is refused, the new entry
# points run), and the smallest one whose full-resolution z-ring launches take the hint by themselves
# (more blocks than CUs, 128 planes per block: 32 channels at 2 x 128^3)
@pytest.mark.parametrize("name,shape", [("unet3d_cfg2_small", (1, 32, 32, 32)),
                                        ("wide", (2, 128, 128, 128))])
def test_training_step_is_bit_identical_with_and_without_the_hint(cuda, monkeypatch, name, shape):
    from adell_mri_amd import functional as HF
    from cases import UNET_CASES

    kw = dict(UNET_CASES["unet3d_cfg2_small"])
    if name == "wide":
        kw.update(depth=[32, 32, 32])
        for c0, c1 in ((32, 0), (32, 32)):
            assert ops.conv3d_bwd_weight_share_plan(2, shape[1:], c0, c1, 32, 3, 1, 1,
                                                    AUTO).blocks_per_cu == 1
    calls, real = [], ops.conv3d_bwd_weight

    def spy(*a, **k):
        calls.append(bool(k.get("share")))
        return real(*a, **k)

    monkeypatch.setattr(ops, "conv3d_bwd_weight", spy)
    loss0, grads0 = _train_step(cuda, kw, shape, True, monkeypatch)
    calls0, calls[:] = list(calls), []
    loss1, grads1 = _train_step(cuda, kw, shape, False, monkeypatch)
    calls1 = list(calls)
    assert not any(calls0), "no_wgrad_share: no call may carry a hint"
    if HF.FLAGS["wgrad_stream"]:
        assert any(calls1), "the side-stream weight gradients must carry the hint"
    assert loss0 == loss1
    assert sorted(grads0) == sorted(grads1)
    for k in grads0:
        assert torch.equal(grads0[k], grads1[k]), k
