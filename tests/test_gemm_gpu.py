"""fp32-MFMA row-major GEMM (csrc/gemm.hip) behind torch.nn.Linear: the fused bias / residual
epilogue and the gradients against float64 (every route in every operand layout:
tests/test_gemm_plans.py)."""
import numpy as np
import pytest
import torch

import test_gemm_plans as table
from adell_mri_amd import functional as HF


def rel(a, r):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return float(np.abs(a - r).max() / (np.abs(r).max() + 1e-30))


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(c.M, c.N, c.K) for c in table.CASES if c.family == "f32" and "former" in c.opt])
@pytest.mark.parametrize("layout", ["nt", "nn", "tn"])
def test_gemm_layouts_match_float64(cuda, M, N, K, layout):
    """One layout of the shape's row in the case table of tests/test_gemm_plans.py: the route the row
    pins, then the product against float64 at the family's bar."""
    table.check_f32_case(table.case_of("f32", M, N, K), cuda, [layout])


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K", [(5, 7, 9), (432, 768, 768), (16, 2048, 1024), (2048, 96, 384)])
def test_linear_bias_residual_and_grads(cuda, M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn((M, K), generator=g, dtype=torch.float64).requires_grad_(True)
    w = (torch.randn((N, K), generator=g, dtype=torch.float64) / np.sqrt(K)).requires_grad_(True)
    b = torch.randn((N,), generator=g, dtype=torch.float64).requires_grad_(True)
    r = torch.randn((M, N), generator=g, dtype=torch.float64).requires_grad_(True)
    y = torch.nn.functional.linear(x, w, b) + r
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    xd, wd, bd, rd = [t.detach().float().to(cuda).requires_grad_(True) for t in (x, w, b, r)]
    yd = HF.linear(xd, wd, bd, residual=rd)
    yd.backward(dy.float().to(cuda))
    assert rel(yd, y.detach().numpy()) < 5e-6
    assert rel(xd.grad, x.grad.numpy()) < 5e-6
    assert rel(wd.grad, w.grad.numpy()) < 5e-6
    assert rel(bd.grad, b.grad.numpy()) < 5e-6
    assert rel(rd.grad, r.grad.numpy()) < 1e-7


@pytest.mark.gpu
def test_linear_on_token_tensor_keeps_leading_shape(cuda):
    x = torch.randn((2, 24, 32), device=cuda, requires_grad=True)
    w = torch.randn((48, 32), device=cuda, requires_grad=True)
    y = HF.linear(x, w)
    assert y.shape == (2, 24, 48)
    ref = x.detach().double().cpu() @ w.detach().double().cpu().t()
    assert rel(y, ref.numpy()) < 5e-6
    y.sum().backward()
    assert x.grad.shape == x.shape and w.grad.shape == w.shape
