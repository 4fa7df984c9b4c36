"""The 32 x 32 channel-tile form of the z-marching backward-weight kernel (conv_wgrad_zring.hip)
against torch's fp64 weight and bias gradient on the CPU, on operands that are NOT well scaled
(x * 37, dy * 3e-4: the power-of-two block scaling has to carry them), at the smallest shapes at
which each of its paths can still go wrong (the plan needs Wo, Ho >= 8 and Do >= 4). The bound,
max |d| / max |ref| < 3e-6, is the one test_zring16_against_fp64 holds for the 16 x 16 tile form;
every case also runs twice and must be bit-equal (same slabs, same fold order)."""
import ctypes

import pytest
import torch

from adell_mri_amd import _lib, ops

pytestmark = pytest.mark.gpu

TOL = 3e-6

# n, c0, c1, cout, (D, H, W), pad
CASES = [
    (1, 32, 0, 32, (6, 16, 24), 1),      # several columns, every k-step, z priming against the tensor edge
    (1, 32, 0, 64, (9, 17, 33), 1),      # bricks with one valid row and one valid column
    (1, 32, 0, 32, (14, 18, 22), 0),     # padding 0
    (1, 16, 16, 32, (9, 17, 33), 1),     # a tile that straddles the concat boundary
    (1, 48, 16, 80, (10, 16, 24), 1),    # a ragged last tile on the output side
    (2, 32, 0, 32, (24, 16, 16), 1),     # batch items and z segments
    (1, 32, 0, 32, (6, 192, 192), 1),    # 576 columns on 512 blocks: a block walks two units and re-primes its ring
]


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-300))


@pytest.mark.parametrize("n,c0,c1,cout,size,pad", CASES)
def test_zring32_against_fp64(cuda, n, c0, c1, cout, size, pad):
    g = torch.Generator().manual_seed(7 * c0 + cout + size[1] + pad)
    D, H, W = size
    Do, Ho, Wo = (s + 2 * pad - 2 for s in size)
    cin = c0 + c1
    x = torch.randn(n, cin, D, H, W, generator=g) * 37.0
    dy = torch.randn(n, cout, Do, Ho, Wo, generator=g) * 3e-4

    plan = (ctypes.c_int * 8)()      # WgradZrPlan: ntx, nty, nseg, seglen, nci, nco, R, t16
    assert _lib.lib().adell_wgrad_zring_plan(n, D, H, W, c0, c1, cout, 3, 3, 3, 1, 1, 1, Do, Ho, Wo,
                                             plan) == 1
    assert plan[7] == 0, "this file is about the 32 x 32 tile form"
    if size == (6, 192, 192):
        assert n * plan[0] * plan[1] * plan[2] > plan[6], "a block has to walk more than one unit"

    dw_ref = torch.nn.grad.conv3d_weight(x.double(), (cout, cin, 3, 3, 3), dy.double(), padding=pad)
    db_ref = dy.double().sum(dim=(0, 2, 3, 4))

    x0 = ops.ndhwc(x[:, :c0].contiguous().to(cuda))
    x1 = ops.ndhwc(x[:, c0:].contiguous().to(cuda)) if c1 else None
    dyd = ops.ndhwc(dy.to(cuda))

    def run():
        return ops.conv3d_bwd_weight(x0, dyd, 3, 1, pad, x1=x1, want_db=True, f16x3=True)

    dw, db = run()
    dw2, db2 = run()
    e_w, e_b = _rel(dw.cpu().double(), dw_ref), _rel(db.cpu().double(), db_ref)
    print(f"zring32 fp64 parity {n}x({c0}+{c1})->{cout} {size} pad {pad}: dW {e_w:.3e} db {e_b:.3e}")
    assert e_w < TOL
    assert e_b < TOL
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
