"""SWIN-UNets whose windows or heads are beyond the small-window attention kernel
(tests/swin_window_cases.py) against fixtures generated from the real reference
(tools/make_golden_swin_windows.py): 216-token windows on the MFMA sequence kernels, 16-token windows
with 64- and 128-wide heads, 125-token windows with 24-wide heads on the vector-ALU kernels. The
shift mask travels as region labels, the relative-position tables get their gradient from
ops.attention_bias_grad."""
import numpy as np
import pytest
import torch

from adell_mri_amd import functional as HF
from adell_mri_amd.modules.layers.linear_blocks import MultiHeadSelfAttention
from adell_mri_amd.modules.layers.vit import mask_from_labels, shift_region_labels
from oracle.torch_ref.unet import compound_loss
from swin_window_cases import SWIN_WINDOW_CASES, build_net, load_fixture

pytestmark = pytest.mark.gpu


def _logits_err(net, g, cuda):
    with torch.no_grad():
        logits, _ = net(torch.from_numpy(g["x"]).to(cuda), return_logits=True)
    ref = g["logits"]
    assert logits.shape == ref.shape
    return np.abs(logits.cpu().numpy() - ref).max() / np.abs(ref).max()


@pytest.mark.parametrize("name", list(SWIN_WINDOW_CASES))
def test_logits_loss_and_gradients_match_reference(cuda, name):
    g = load_fixture(name)
    net = build_net(name).to(cuda).eval()
    err = _logits_err(net, g, cuda)
    print(name, "logits", f"{err:.2e}")
    assert err < 1e-4, err
    prob, _ = net(torch.from_numpy(g["x"]).to(cuda))
    loss = compound_loss(prob, torch.from_numpy(g["y"]).to(cuda))
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=1e-4)
    loss.backward()
    tables = 0
    for k, p in net.named_parameters():
        if ("grad:" + k) not in g:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            continue
        # the criterion of tests/test_swin.py: the reference's fp64 gradient is the target, the bar
        # 3e-3 or twice the reference's own fp32-vs-fp64 difference
        ref32, ref64 = g["grad:" + k], g["grad64:" + k]
        scale = np.abs(ref64).max()
        if k.endswith(".bias") and ("grad64:" + k[:-5] + ".weight") in g:
            scale = max(scale, 1e-1 * np.abs(g["grad64:" + k[:-5] + ".weight"]).max())
        noise = np.abs(ref32 - ref64).max() / (scale + 1e-12)
        err = np.abs(p.grad.cpu().numpy() - ref64).max() / (scale + 1e-12)
        assert err < max(3e-3, 2 * noise), (k, err, noise)
        if k.endswith("relative_position_bias_table"):
            tables += 1
            assert float(p.grad.abs().max()) > 0 and np.abs(ref64).max() > 0, k
    assert tables == 4


def test_labels_route_equals_dense_mask_route(cuda):
    """One windowed layer (216 tokens, 8 windows x 2 images) called with region labels and with the
    dense mask built from them (rel[None] + mask[:, None] as a per-sequence bias, its gradient back
    through the library's add): the routes differ only in the rounding of entries the softmax sends
    to zero and in the order of the sums over the items."""
    torch.manual_seed(3)
    mha = MultiHeadSelfAttention(64, 64, 64, 64, n_heads=2, window_size=[6, 6, 6]).to(cuda)
    with torch.no_grad():
        mha.relative_position_bias_table.mul_(25.0)       # entries of order 0.5, not 0.02
    labels = shift_region_labels([12] * 3, [6] * 3, 2)
    assert labels.shape == (8, 216)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 8, 216, 64, generator=g).to(cuda)
    dy = torch.randn(2, 8, 216, 64, generator=g).to(cuda)
    res = []
    for kw in (dict(mask_labels=labels.to(cuda)), dict(mask=mask_from_labels(labels).to(cuda))):
        mha.zero_grad()
        xi = x.clone().requires_grad_(True)
        y = mha(xi, **kw)
        y.backward(dy)
        torch.cuda.synchronize()
        res.append(dict(out=y.detach().clone(), dx=xi.grad.clone(),
                        **{k: p.grad.clone() for k, p in mha.named_parameters()}))
    assert float(res[0]["relative_position_bias_table"].abs().max()) > 0
    for k in res[0]:
        a, b = res[0][k].double(), res[1][k].double()
        err = float((a - b).abs().max() / b.abs().max())
        print(k, f"{err:.2e}")
        assert err < 1e-6, (k, err)


def test_sliced_path_switch_gives_the_same_logits(cuda, monkeypatch):
    """ADELL_NO_SEQ_ATTENTION=1 (read into functional.FLAGS at import): sliced q / k / v through
    functional.attention instead of the in-place sequence form."""
    name = "swinunet3d_t216_a32"
    g = load_fixture(name)
    monkeypatch.setitem(HF.FLAGS, "no_seq_attention", True)
    assert not HF.seq_attention_ok(216, 32, 32)
    net = build_net(name).to(cuda).eval()
    err = _logits_err(net, g, cuda)
    print("sliced path logits", f"{err:.2e}")
    assert err < 1e-4, err


def test_training_mode_with_dropout_runs_and_learns(cuda):
    from adell_mri_amd.optim import FusedSGD

    name = "swinunet3d_t216_a32"
    g = load_fixture(name)
    net = build_net(name, dropout_rate=0.1).to(cuda).train()
    opt = FusedSGD(net.parameters(), lr=1e-2, momentum=0.9)
    x, y = torch.from_numpy(g["x"]).to(cuda), torch.from_numpy(g["y"]).to(cuda)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        prob, _ = net(x)
        loss = compound_loss(prob, y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print("losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
