"""The sequence attention kernels (csrc/tokens.hip) as SWIN windows use them beyond the small-window
kernel: a relative-position bias per head (bias slice h for sequence b * H + h), the shift mask as
region labels (-100 between tokens whose labels differ), and the gradient of the bias summed over
the items, which no kernel materialises per sequence (ops.attention_bias_grad).

Against torch fp64 on the CPU of softmax(q k^T scale + rel[h] + mask_from_labels) v; inputs as in
tests/test_attention_plans.py (fp32-representable, seeded by case id) and its bars: largest error
over largest reference value, 1e-5 for out / lse, 5e-5 for the gradients, dbias included (a sum of
at most 8 fp32 terms adds under 1e-6). Where torch's own fp32 CPU evaluation of the same inputs
exceeds a quarter of a bar, the bar is 4 x that value and the value is printed (the rule of the
"large scores" cases there)."""
import collections
import zlib

import pytest
import torch

from adell_mri_amd import _lib, ops
from adell_mri_amd import functional as HF
from adell_mri_amd.modules.layers.vit import shift_region_labels

pytestmark = pytest.mark.gpu

# items B = images x windows; labels has nlab rows (windows per image), item b reads row b % nlab.
# opt: "real" labels of shift_region_labels; "drop" dropout 0.1; "unaligned" every operand one
# element into its storage; "per_seq" also nbias = B * H through the autograd wrapper
Case = collections.namedtuple("Case", "B H T A Dv nlab path opt")
CASES = [
    Case(6, 2, 216, 32, 32, 3, "mfma_resident", {"per_seq"}),
    Case(8, 1, 216, 32, 32, 8, "mfma_resident", {"real"}),
    Case(4, 1, 216, 128, 128, 2, "mfma_streamed", set()),
    Case(8, 2, 16, 64, 64, 4, "mfma_resident", set()),
    Case(2, 2, 343, 32, 32, 2, "mfma_resident", set()),       # 7^3: T % 4 != 0
    Case(2, 1, 512, 32, 32, 2, "mfma_resident", set()),       # the largest 8^3 window
    Case(4, 2, 125, 24, 24, 2, "valu", {"per_seq"}),
    Case(4, 2, 50, 64, 64, 2, "valu", {"unaligned"}),
    Case(4, 2, 77, 64, 64, 2, "mfma_resident", {"drop"}),     # T % 4 != 0: Philox block boundaries
    Case(4, 2, 70, 24, 40, 2, "valu", {"drop"}),
]
P_DROP, SEED, OFFSET = 0.1, 1234567891011, 7
BARS = dict(out=1e-5, lse=1e-5, dq=5e-5, dk=5e-5, dv=5e-5, dbias=5e-5)


def _case_id(c):
    tags = "".join("_" + t for t in sorted(c.opt - {"per_seq"}))
    return f"b{c.B}_h{c.H}_t{c.T}_a{c.A}_d{c.Dv}_l{c.nlab}{tags}"


def _inputs(c):
    g = torch.Generator().manual_seed(zlib.crc32(_case_id(c).encode()))
    BH = c.B * c.H
    q = torch.randn(BH, c.T, c.A, generator=g)
    k = torch.randn(BH, c.T, c.A, generator=g)
    v = torch.randn(BH, c.T, c.Dv, generator=g)
    do = torch.randn(BH, c.T, c.Dv, generator=g)
    rel = torch.randn(c.H, c.T, c.T, generator=g)
    if "real" in c.opt:
        labels = shift_region_labels([12] * 3, [6] * 3, 2)
        assert labels.shape == (c.nlab, c.T)
    else:
        labels = torch.randint(0, 4, (c.nlab, c.T), generator=g, dtype=torch.int32)
    return q, k, v, do, rel, labels


def _label_mask(c, labels, dtype):
    """[B * H, T, T]: -100 where the labels of item bh // H differ (row (bh // H) % nlab)."""
    lab = labels[(torch.arange(c.B * c.H) // c.H) % c.nlab]
    return torch.where(lab[:, :, None] != lab[:, None, :], -100.0, 0.0).to(dtype)


def _reference(c, q, k, v, do, bias, labels, keep=None, dtype=torch.float64):
    """bias [nbias, T, T]: sequence bh reads slice bh % nbias; its gradient comes back summed."""
    qr, kr, vr, br = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v, bias))
    s = qr @ kr.transpose(-1, -2) * (c.A ** -0.5) + br[torch.arange(c.B * c.H) % br.shape[0]]
    if labels is not None:
        s = s + _label_mask(c, labels, dtype)
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep.to(dtype)
    out = p @ vr
    out.backward(do.to(dtype))
    return dict(out=out.detach(), lse=torch.logsumexp(s.detach(), -1), dq=qr.grad, dk=kr.grad,
                dv=vr.grad, dbias=br.grad)


def _rel(a, b):
    b = b.double()
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))


def _dev(t, cuda, offset=False):
    if not offset:
        return t.to(cuda)
    buf = torch.zeros(t.numel() + 1, device=cuda, dtype=t.dtype)
    view = buf[1:].view(t.shape)
    view.copy_(t.to(cuda))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _keep_mask(cuda, c, qd, kd, scale):
    """The keep mask of (SEED, OFFSET) scaled by 1 / (1 - p): a function of (seed, offset, bh, query,
    key, T) alone, so it is read off the vector-ALU forward with identity V -- without bias and
    labels, whose -100 entries would underflow and read as dropped."""
    BH = c.B * c.H
    assert c.T <= 256
    with _lib.tuning(attn_nomfma=1):
        assert ops.attention_plan(c.T, c.A, c.T).path == "valu"
        eye = torch.eye(c.T, device=cuda).expand(BH, c.T, c.T).contiguous()
        pt, _ = ops.attention_fwd(qd, kd, eye, None, scale, P_DROP, SEED, OFFSET)
        p0, _ = ops.attention_fwd(qd, kd, eye, None, scale)
    kept = pt != 0
    assert bool((p0 != 0).all())
    assert torch.allclose(pt[kept], p0[kept] / (1 - P_DROP), rtol=1e-5, atol=1e-8)
    frac = kept.float().mean().item()
    assert abs(frac - (1 - P_DROP)) < 0.01, frac
    return kept.cpu().double() / (1 - P_DROP)


def _check(tag, got, ref, ref32, names):
    e32 = {n: _rel(ref32[n], ref[n]) for n in names}
    bars = {n: BARS[n] if e32[n] <= BARS[n] / 4 else 4 * e32[n] for n in names}
    wide = {n: f"{e32[n]:.2e}" for n in names if bars[n] != BARS[n]}
    if wide:
        print(f"{tag}: torch fp32 CPU above a quarter of the bar: {wide}")
    errs = {n: _rel(got[n], ref[n]) for n in names}
    print(tag, {n: f"{e:.2e}" for n, e in errs.items()})
    assert all(bool(torch.isfinite(got[n]).all()) for n in names), "non-finite result"
    bad = {n: (e, bars[n]) for n, e in errs.items() if not e < bars[n]}
    assert not bad, f"{tag}: relative error above the bound: {bad}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_case_matches_torch_fp64(cuda, case):
    c = case
    off = "unaligned" in c.opt
    assert ops.attention_plan(c.T, c.A, c.Dv, "dq", aligned=not off).path == c.path
    q, k, v, do, rel, labels = _inputs(c)
    qd, kd, vd, dod, reld, labd = (_dev(t, cuda, off) for t in (q, k, v, do, rel, labels))
    scale = c.A ** -0.5
    drop = (P_DROP, SEED, OFFSET) if "drop" in c.opt else ()
    keep = _keep_mask(cuda, c, qd, kd, scale) if drop else None
    ref = _reference(c, q, k, v, do, rel, labels, keep)
    ref32 = _reference(c, q, k, v, do, rel, labels, keep, torch.float32)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())

    out, lse = ops.attention_fwd(qd, kd, vd, reld, scale, *drop, labels=labd, heads=c.H)
    dq, dk, dv = ops.attention_bwd(qd, kd, vd, reld, out, dod, lse, scale, *drop, labels=labd,
                                   heads=c.H)
    dbias = ops.attention_bias_grad(qd, kd, vd, reld, out, dod, lse, scale, c.H, *drop, labels=labd,
                                    heads=c.H)
    torch.cuda.synchronize()
    assert dbias.shape == (c.H, c.T, c.T)
    got = {n: t.cpu() for n, t in dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv, dbias=dbias).items()}
    _check(_case_id(c), got, ref, ref32, list(BARS))


@pytest.mark.parametrize("case", [c for c in CASES if "per_seq" in c.opt], ids=_case_id)
def test_per_sequence_bias_through_functional_attention(cuda, case):
    """nbias = B * H: the gradient of a per-sequence bias is dS itself, returned by the backward of
    functional.attention."""
    c = case
    q, k, v, do, _, labels = _inputs(c)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(c.B * c.H, c.T, c.T, generator=g)
    ref = _reference(c, q, k, v, do, bias, labels)
    ref32 = _reference(c, q, k, v, do, bias, labels, None, torch.float32)
    leaves = [t.to(cuda).requires_grad_(True) for t in (q, k, v, bias)]
    out = HF.attention(*leaves, labels=labels.to(cuda), heads=c.H)
    out.backward(do.to(cuda))
    torch.cuda.synchronize()
    got = dict(out=out.detach().cpu(), dq=leaves[0].grad.cpu(), dk=leaves[1].grad.cpu(),
               dv=leaves[2].grad.cpu(), dbias=leaves[3].grad.cpu())
    assert got["dbias"].shape == bias.shape
    _check("functional " + _case_id(c), got, ref, ref32, ["out", "dq", "dk", "dv", "dbias"])


def _ln(x, gamma, beta):
    return torch.nn.functional.layer_norm(x, x.shape[-1:], gamma, beta, 1e-5)


def test_seq_attention_returns_the_bias_gradient(cuda):
    """functional.seq_attention (q-norm, k-norm and attention on the packed projection) with a
    per-head bias that requires grad and labels: output and every gradient against fp64."""
    B, H, T, a, hd, nlab = 4, 2, 80, 32, 64, 2
    g = torch.Generator().manual_seed(11)
    per = 2 * a + hd
    qkv = torch.randn(B * T, H * per, generator=g)
    do = torch.randn(B * T, H * hd, generator=g)
    rel = torch.randn(H, T, T, generator=g)
    qg, qb, kg, kb = (torch.randn(a, generator=g) * 0.3 + s for s in (1.0, 0.0, 1.0, 0.0))
    labels = torch.randint(0, 3, (nlab, T), generator=g, dtype=torch.int32)
    c = Case(B, H, T, a, hd, nlab, "mfma_resident", set())

    def reference(dtype):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in (qkv, rel, qg, qb, kg, kb)]
        x = leaves[0].view(B, T, H, per).permute(0, 2, 1, 3)
        qn = _ln(x[..., :a], leaves[2], leaves[3]).reshape(B * H, T, a)
        kn = _ln(x[..., a:2 * a], leaves[4], leaves[5]).reshape(B * H, T, a)
        s = qn @ kn.transpose(-1, -2) * (a ** -0.5) + leaves[1][torch.arange(B * H) % H]
        s = s + _label_mask(c, labels, dtype)
        o = torch.softmax(s, -1) @ x[..., 2 * a:].reshape(B * H, T, hd)
        o = o.view(B, H, T, hd).permute(0, 2, 1, 3).reshape(B * T, H * hd)
        o.backward(do.to(dtype))
        return dict(zip(("out", "dqkv", "dbias", "dqg", "dqb", "dkg", "dkb"),
                        [o.detach()] + [t.grad for t in leaves]))

    ref, ref32 = reference(torch.float64), reference(torch.float32)
    leaves = [t.to(cuda).requires_grad_(True) for t in (qkv, rel, qg, qb, kg, kb)]
    assert HF.seq_attention_ok(T, a, hd)
    o = HF.seq_attention(leaves[0], leaves[2], leaves[3], leaves[4], leaves[5], B, H, T, a, hd,
                         bias=leaves[1], labels=labels.to(cuda))
    o.backward(do.to(cuda))
    torch.cuda.synchronize()
    got = dict(zip(("out", "dqkv", "dbias", "dqg", "dqb", "dkg", "dkb"),
                   [o.detach().cpu()] + [t.grad.cpu() for t in leaves]))
    # dkb is left out: a constant added to every key moves all scores of a query alike, so its
    # gradient is zero in exact arithmetic and rounding noise in the reference
    names = [n for n in got if n != "dkb"]
    assert bool(torch.isfinite(got["dkb"]).all())
    e32 = {n: _rel(ref32[n], ref[n]) for n in names}
    errs = {n: _rel(got[n], ref[n]) for n in names}
    print("seq_attention", {n: f"{e:.2e}" for n, e in errs.items()}, "torch fp32 CPU",
          {n: f"{e:.2e}" for n, e in e32.items()})
    for n in names:
        bar = 1e-5 if n == "out" else 5e-5
        bar = bar if e32[n] <= bar / 4 else 4 * e32[n]
        assert errs[n] < bar, (n, errs[n], bar)


@pytest.mark.parametrize("shape", [(2, 2, 216, 32, 32, "mfma_resident"),
                                   (2, 1, 216, 128, 128, "mfma_streamed"),
                                   (2, 2, 125, 24, 24, "valu")], ids=lambda s: s[-1])
def test_equal_labels_change_nothing(cuda, shape):
    B, H, T, A, Dv, path = shape
    assert ops.attention_plan(T, A, Dv).path == path
    c = Case(B, H, T, A, Dv, 1, path, set())
    q, k, v, do, rel, _ = (t.to(cuda) for t in _inputs(c))
    same = torch.full((1, T), 7, dtype=torch.int32, device=cuda)
    scale = A ** -0.5
    res = []
    for lab in (None, same):
        out, lse = ops.attention_fwd(q, k, v, rel, scale, labels=lab, heads=H)
        grads = ops.attention_bwd(q, k, v, rel, out, do, lse, scale, labels=lab, heads=H)
        db = ops.attention_bias_grad(q, k, v, rel, out, do, lse, scale, H, labels=lab, heads=H)
        res.append((out, lse, *grads, db))
    for name, x, y in zip(("out", "lse", "dq", "dk", "dv", "dbias"), *res):
        assert torch.equal(x, y), name


def _bias_grad_peak(cuda, B, H=2, T=216, A=32):
    g = torch.Generator().manual_seed(B)
    q, k, v, do = (torch.randn(B * H, T, A, generator=g).to(cuda) for _ in range(4))
    rel = torch.randn(H, T, T, generator=g).to(cuda)
    lab = torch.randint(0, 4, (4, T), generator=g, dtype=torch.int32).to(cuda)
    scale = A ** -0.5
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out, lse = ops.attention_fwd(q, k, v, rel, scale, labels=lab, heads=H)
    torch.cuda.synchronize()
    fwd_peak = torch.cuda.max_memory_allocated() - base
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    db = ops.attention_bias_grad(q, k, v, rel, out, do, lse, scale, H, labels=lab, heads=H)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    again = ops.attention_bias_grad(q, k, v, rel, out, do, lse, scale, H, labels=lab, heads=H)
    return fwd_peak, out.numel() * 4 + lse.numel() * 4, peak, db, again


def test_bias_grad_is_deterministic_and_its_memory_does_not_grow_with_the_items(cuda):
    """No tensor of items * H * T^2 elements exists: the bias gradient allocates its [H, T, T]
    result and a workspace sized by (H, T) alone, the forward with labels its out and lse."""
    H, T = 2, 216
    peaks = {}
    for B in (8, 64):
        fwd_peak, fwd_need, peak, db, again = _bias_grad_peak(cuda, B)
        assert torch.equal(db, again), "attention_bias_grad differs from run to run"
        assert fwd_need <= fwd_peak <= fwd_need + 2 * 512, (B, fwd_peak, fwd_need)   # allocator rounding
        peaks[B] = peak
    ws = _lib.lib().adell_attention_bias_grad_workspace_floats(H, T)
    assert peaks[8] == peaks[64], peaks
    assert peaks[64] <= H * T * T * 4 + ws * 4 + 2 * 512, (peaks, ws)
    assert peaks[64] < 64 * H * T * T * 4 // 2          # dS of all sequences would be 24 MB
