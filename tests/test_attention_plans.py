"""Every launch plan of full-sequence attention (csrc/tokens.hip adell_att_plan: 9 MFMA head shapes, each
resident or streamed, forward / dQ / dK-dV, and the three vector-ALU kernels), from one case table:

- on the build host (no GPU), each case still gets the plan it is in the table for in all three passes
  (ops.attention_plan: the function the launchers take their decisions from), every branch has exactly
  one case, and the table has a case at every resident limit and at the T one above it, the limits read
  off the plan query. A retune that moves a shape onto another kernel, or a case deleted from the
  table, fails here naming the branch;
- on the GPU, each case runs through ops.attention_fwd / ops.attention_bwd (the "functional" ones also
  through functional.attention) against torch fp64 on the CPU: softmax(Q K^T scale + bias) V, lse =
  logsumexp of the scores, gradients from autograd.

Bars (the ones tests/test_tokens_gpu.py holds): largest error over the largest reference value, 1e-5
for out and lse, 5e-5 for dQ, dK and dV. torch's own fp32 CPU evaluation of the formula is below 1.2e-6
of fp64 on these inputs (2.5e-6 on the large-score ones), so the bars are not the reference's noise.

Dropout cases: the keep mask is a function of (seed, offset, bh, query, key, T) alone, so it is read
off the vector-ALU forward with identity V (column blocks of at most 256) and the MFMA kernels must
reproduce it -- at T % 4 != 0 across Philox block boundaries."""
import collections
import zlib

import pytest
import torch

from adell_mri_amd import _lib, ops

SHAPES = [(A, Dv) for A in (32, 64, 128) for Dv in (32, 64, 128)]
PASSES = ("fwd", "dq", "dkv")
LDS_MAX = 160 * 1024

# plan: what ops.attention_plan gives for (fwd, dq, dkv); a dict entry adds fields to check (rows).
# opt: "functional" also runs through functional.attention; "inf" -inf bias entries; "large" q and k
# scaled by 3; "drop" dropout p = 0.1 against the mask read off the vector-ALU forward; "unaligned"
# every operand one element into its storage (and the plan asked with aligned=False).
Case = collections.namedtuple("Case", "branch BH T A Dv nbias plan opt")

RES, STR, VALU = ("mfma_resident",) * 3, ("mfma_streamed",) * 3, ("valu",) * 3
MIXED = ("mfma_resident", "mfma_resident", "mfma_streamed")


def _rows(fwd, dq, dkv):
    return tuple(dict(path="valu", rows=r) for r in (fwd, dq, dkv))


CASES = [
    # ---- the nine MFMA head shapes, resident ------------------------------------------------------
    Case("resident (32,32): dK/dV limit", 2, 544, 32, 32, 0, RES, set()),
    Case("resident (32,64)", 2, 33, 32, 64, 1, RES, set()),
    Case("resident (64,32)", 2, 17, 64, 32, 2, RES, set()),
    Case("resident (64,64): limit", 2, 288, 64, 64, 0, RES, {"functional"}),
    Case("resident (32,128)", 2, 77, 32, 128, 0, RES, set()),
    Case("resident (128,32)", 4, 50, 128, 32, 2, RES, set()),
    Case("resident (64,128): limit", 2, 192, 64, 128, 0, RES, set()),
    Case("resident (128,64)", 2, 100, 128, 64, 2, RES, set()),
    Case("resident (128,128): limit", 2, 128, 128, 128, 0, RES, set()),
    # the resident limits the cases above are not on
    Case("resident (32,64): limit", 2, 384, 32, 64, 0, RES, set()),
    Case("resident (64,32): limit", 2, 384, 64, 32, 0, RES, set()),
    Case("resident (32,128): limit", 2, 224, 32, 128, 0, RES, set()),
    Case("resident (128,32): limit", 2, 224, 128, 32, 0, RES, set()),
    Case("resident (128,64): limit", 2, 192, 128, 64, 0, RES, set()),
    # ---- streamed: the first T past the limit (last key tile of one row; idle waves at 129 and 385) -
    Case("streamed (32,32)", 2, 577, 32, 32, 0, STR, set()),
    Case("streamed (32,64)", 2, 385, 32, 64, 1, STR, set()),
    Case("streamed (64,32)", 2, 385, 64, 32, 2, STR, set()),
    Case("streamed (64,64)", 2, 289, 64, 64, 0, STR, {"functional"}),
    Case("streamed (32,128)", 2, 225, 32, 128, 0, STR, set()),
    Case("streamed (128,32)", 2, 225, 128, 32, 0, STR, set()),
    Case("streamed (64,128)", 2, 193, 64, 128, 0, STR, set()),
    Case("streamed (128,64)", 2, 193, 128, 64, 0, STR, set()),
    Case("streamed (128,128)", 4, 129, 128, 128, 2, STR, set()),
    # ---- mixed regime: the dK/dV row is 2 floats longer ------------------------------------------
    Case("mixed (32,32): first T with dK/dV streamed", 2, 545, 32, 32, 0, MIXED, set()),
    Case("mixed (32,32): forward / dQ limit", 2, 576, 32, 32, 0, MIXED, set()),
    # ---- MFMA edges in T --------------------------------------------------------------------------
    Case("T 16: smallest MFMA T", 2, 16, 64, 64, 0, RES, set()),
    Case("T 15: vector-ALU neighbour of T 16", 2, 15, 64, 64, 0, VALU, set()),
    Case("T 32: one full tile", 2, 32, 64, 64, 0, RES, set()),
    Case("T 33: one row over a tile", 2, 33, 64, 64, 0, RES, set()),
    # ---- vector-ALU kernels: column bands of the lane + 64 d loops --------------------------------
    Case("vector-ALU band 1, T one over the key tile", 2, 65, 72, 72, 1, VALU, {"functional"}),
    Case("vector-ALU bands 3 and 2", 2, 70, 200, 136, 0, VALU, set()),
    Case("vector-ALU bands 2 and 3, T one over the row block", 2, 17, 136, 200, 2, VALU, set()),
    Case("vector-ALU band 0: odd dims, exact tile", 4, 64, 7, 9, 2, VALU, set()),
    # ---- backward LDS budget: 16 rows per block while they fit, 8 otherwise -----------------------
    Case("budget A + Dv = 502: 16 rows everywhere", 1, 5, 256, 246, 0, _rows(16, 16, 16), set()),
    Case("budget A + Dv = 507: dK/dV on 8 rows", 1, 5, 251, 256, 0, _rows(16, 16, 8), set()),
    Case("budget (256,256): both backward kernels on 8 rows", 1, 5, 256, 256, 0, _rows(16, 8, 8),
         set()),
    Case("budget: several 8-row blocks", 2, 21, 256, 256, 1, _rows(16, 8, 8), set()),
    # ---- -inf bias (a boolean attn_mask): first key tile of some queries fully masked --------------
    Case("-inf bias, resident", 2, 130, 64, 64, 2, RES, {"inf", "functional"}),
    Case("-inf bias, streamed", 2, 130, 128, 128, 1, STR, {"inf"}),
    Case("-inf bias, vector-ALU", 2, 130, 24, 40, 2, VALU, {"inf", "functional"}),
    # ---- large scores (q and k scaled by 3) --------------------------------------------------------
    # torch fp32 CPU against fp64 on these inputs (max |score| 36.7), measured on the build host: out
    # 1.9e-6, lse 2.1e-7, dQ 1.7e-6, dK 2.1e-6, dV 8.3e-7; 4 x that is below the standing bars, which hold
    Case("large scores, MFMA", 2, 97, 64, 64, 0, RES, {"large"}),
    # (max |score| 36.0) out 9.8e-7, lse 2.3e-7, dQ 2.5e-6, dK 2.0e-6, dV 1.1e-6: the standing bars hold
    Case("large scores, vector-ALU", 2, 97, 24, 24, 0, VALU, {"large"}),
    # ---- dropout ----------------------------------------------------------------------------------
    Case("dropout, resident, odd T", 2, 77, 64, 64, 0, RES, {"drop"}),
    Case("dropout, streamed", 2, 129, 128, 128, 0, STR, {"drop"}),
    Case("dropout, mixed", 2, 545, 32, 32, 0, MIXED, {"drop"}),
    Case("dropout, vector-ALU", 2, 70, 72, 40, 1, VALU, {"drop"}),
    # ---- operands that are not 16-byte aligned take the vector-ALU kernels ------------------------
    Case("unaligned routing", 2, 50, 64, 64, 0, VALU, {"unaligned"}),
]

# every branch has exactly one case: deleting a case fails test_table_covers_every_branch by name
BRANCHES = [
    "resident (32,32): dK/dV limit", "resident (32,64)", "resident (64,32)", "resident (64,64): limit",
    "resident (32,128)", "resident (128,32)", "resident (64,128): limit", "resident (128,64)",
    "resident (128,128): limit",
    "resident (32,64): limit", "resident (64,32): limit", "resident (32,128): limit",
    "resident (128,32): limit", "resident (128,64): limit",
    "streamed (32,32)", "streamed (32,64)", "streamed (64,32)", "streamed (64,64)", "streamed (32,128)",
    "streamed (128,32)", "streamed (64,128)", "streamed (128,64)", "streamed (128,128)",
    "mixed (32,32): first T with dK/dV streamed", "mixed (32,32): forward / dQ limit",
    "T 16: smallest MFMA T", "T 15: vector-ALU neighbour of T 16", "T 32: one full tile",
    "T 33: one row over a tile",
    "vector-ALU band 0: odd dims, exact tile", "vector-ALU band 1, T one over the key tile",
    "vector-ALU bands 3 and 2", "vector-ALU bands 2 and 3, T one over the row block",
    "budget A + Dv = 502: 16 rows everywhere", "budget A + Dv = 507: dK/dV on 8 rows",
    "budget (256,256): both backward kernels on 8 rows", "budget: several 8-row blocks",
    "-inf bias, resident", "-inf bias, streamed", "-inf bias, vector-ALU",
    "large scores, MFMA", "large scores, vector-ALU",
    "dropout, resident, odd T", "dropout, streamed", "dropout, mixed", "dropout, vector-ALU",
    "unaligned routing",
]


def _case_id(c):
    tags = "".join("_" + t for t in sorted(c.opt - {"functional"}))
    return f"bh{c.BH}_t{c.T}_a{c.A}_d{c.Dv}_b{c.nbias}{tags}"


def _plans(c):
    return tuple(ops.attention_plan(c.T, c.A, c.Dv, w, aligned="unaligned" not in c.opt) for w in PASSES)


def _mismatch(c, plans):
    bad = []
    for which, plan, want in zip(PASSES, plans, c.plan):
        want = dict(path=want) if isinstance(want, str) else want
        for key, v in want.items():
            if getattr(plan, key) != v:
                bad.append(f"{which}: {key} {getattr(plan, key)} != {v}")
        if plan.path != "refused" and plan.blocks != -(-c.T // plan.rows):
            bad.append(f"{which}: {plan.blocks} blocks of {plan.rows} rows for {c.T} tokens")
        if plan.lds > LDS_MAX:
            bad.append(f"{which}: {plan.lds} B of LDS")
    return bad


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_plan_of_case(case):
    plans = _plans(case)
    bad = _mismatch(case, plans)
    assert not bad, (f"branch '{case.branch}' lost its case {_case_id(case)}: {bad}; the planner now "
                     f"gives {plans}. Update the case table so the branch keeps a case.")


def test_table_covers_every_branch():
    have = [c.branch for c in CASES]
    assert len(set(have)) == len(have), "a branch has two cases: give each its own tag"
    missing = [b for b in BRANCHES if b not in have]
    assert not missing, f"no case for: {missing}"
    assert not set(have) - set(BRANCHES), f"not in BRANCHES: {sorted(set(have) - set(BRANCHES))}"
    assert len(CASES) <= 60
    ids = [_case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids), "two cases share an id (and with it their inputs)"


def _resident_limit(A, Dv, which):
    """Largest T the plan query keeps resident (the resident T are an interval from 16)."""
    path = [ops.attention_plan(T, A, Dv, which).path for T in range(16, 1025)]
    n = path.count("mfma_resident")
    assert n and path == ["mfma_resident"] * n + ["mfma_streamed"] * (len(path) - n), (A, Dv, which)
    return 15 + n


def test_table_has_a_case_on_each_side_of_each_resident_limit():
    """The limits come from the plan query, not from this file: a retune of the resident budget or of a
    row size moves them, and the table then has to move with them."""
    missing = []
    for A, Dv in SHAPES:
        for i, which in enumerate(PASSES):
            L = _resident_limit(A, Dv, which)
            for T, want in ((L, "mfma_resident"), (L + 1, "mfma_streamed")):
                hit = [c for c in CASES if (c.T, c.A, c.Dv) == (T, A, Dv) and not c.opt - {"functional"}
                       and ops.attention_plan(T, A, Dv, which).path == want
                       and (c.plan[i] if isinstance(c.plan[i], str) else c.plan[i]["path"]) == want]
                if not hit:
                    missing.append(f"({A},{Dv}) {which}: no {want} case at T = {T}")
    assert not missing, f"the resident limits moved away from the table's cases: {missing}"


def test_table_selects_every_kernel_it_promises():
    """Counted on the plans themselves: all 9 head shapes x resident / streamed x 3 passes, the mixed
    regime, both row blocks of both vector-ALU backward kernels, all four column bands for A and Dv,
    streamed launches with idle waves, dropout with T % 4 != 0 on the MFMA kernels."""
    seen, bands_a, bands_d, rows = set(), set(), set(), set()
    for c in CASES:
        plans = _plans(c)
        for which, p in zip(PASSES, plans):
            seen.add((c.A, c.Dv, p.path, which))
            if p.path == "valu":
                rows.add((which, p.rows))
        if plans[0].path == "valu":
            bands_a.add((c.A - 1) // 64)
            bands_d.add((c.Dv - 1) // 64)
    want = {(A, Dv, path, which) for A, Dv in SHAPES for path in ("mfma_resident", "mfma_streamed")
            for which in PASSES}
    assert want <= seen, f"no case for: {sorted(want - seen)}"
    assert any([p.path for p in _plans(c)] == list(MIXED) for c in CASES)
    assert rows == {("fwd", 16), ("dq", 16), ("dq", 8), ("dkv", 16), ("dkv", 8)}
    assert bands_a == bands_d == {0, 1, 2, 3}
    # a streamed launch whose last block has idle waves: fewer than 4 tiles of 32 rows in it
    assert any(_plans(c)[0].path == "mfma_streamed" and 0 < c.T % 128 <= 96 for c in CASES)
    drop = [c for c in CASES if "drop" in c.opt]
    assert {tuple(p.path for p in _plans(c)) for c in drop} == {RES, STR, MIXED, VALU}
    assert all(c.T % 4 for c in drop if _plans(c)[0].path != "valu")
    # a bias shared by all sequences, one per sequence, and one per two of four: on every kind of path
    for kind in ("mfma_resident", "mfma_streamed", "valu"):
        got = {(c.BH, c.nbias) for c in CASES if _plans(c)[0].path == kind and _plans(c)[2].path == kind}
        assert {(2, 1), (2, 2), (4, 2)} <= got, (kind, got)


def test_plan_honours_alignment_and_the_switch():
    P = ops.attention_plan
    for which in PASSES:
        assert P(50, 64, 64, which).path == "mfma_resident"
        assert P(50, 64, 64, which, aligned=False).path == "valu"
        assert P(577, 32, 32, which, aligned=False).path == "valu"
        with _lib.tuning(attn_nomfma=1):
            assert P(50, 64, 64, which).path == "valu"
            assert P(577, 32, 32, which).path == "valu"
        assert P(50, 64, 64, which).path == "mfma_resident"
    assert ops.attention_strided_ok(50, 64, 64) and not ops.attention_strided_ok(15, 64, 64)
    assert not ops.attention_strided_ok(50, 64, 48)
    with _lib.tuning(attn_nomfma=1):
        assert not ops.attention_strided_ok(50, 64, 64)


def test_forward_and_backward_accept_the_same_head_dims():
    """Whatever the forward plans, both backward kernels plan too (no forward that succeeds and a
    backward that raises, no dQ launch followed by a refused dK/dV), within the LDS of a CU; head
    dims above 256 are refused in all three passes."""
    P = ops.attention_plan
    for A in (1, 7, 64, 128, 129, 200, 246, 247, 250, 251, 252, 255, 256):
        for Dv in (1, 9, 64, 128, 200, 246, 251, 252, 256):
            for T in (5, 16, 70):
                plans = [P(T, A, Dv, w) for w in PASSES]
                assert all(p.path != "refused" and 0 < p.lds <= LDS_MAX for p in plans), (T, A, Dv, plans)
                if plans[0].path == "valu":
                    assert plans[0].rows == 16
                    assert plans[1].rows == (16 if A + Dv <= 507 else 8), (A, Dv, plans)
                    assert plans[2].rows == (16 if A + Dv <= 502 else 8), (A, Dv, plans)
    for A, Dv in ((257, 8), (8, 257), (300, 300)):
        assert [P(5, A, Dv, w).path for w in PASSES] == ["refused"] * 3


# ---- GPU: every case against torch fp64 on the CPU ----------------------------------------------

P_DROP, SEED, OFFSET = 0.1, 1234567891011, 7


def _inputs(c):
    """fp32-representable operands as fp64 tensors (the reference sees exactly what the kernels do)."""
    g = torch.Generator().manual_seed(zlib.crc32(_case_id(c).encode()))
    q = torch.randn(c.BH, c.T, c.A, generator=g)
    k = torch.randn(c.BH, c.T, c.A, generator=g)
    v = torch.randn(c.BH, c.T, c.Dv, generator=g)
    do = torch.randn(c.BH, c.T, c.Dv, generator=g)
    bias = torch.randn(c.nbias, c.T, c.T, generator=g) if c.nbias else None
    if "large" in c.opt:
        q, k = q * 3.0, k * 3.0
    if "inf" in c.opt:
        # keys [0, 64) masked for queries q % 3 == 0, keys [32, 64) for q % 3 == 1: the first key tile
        # (32 keys MFMA, 64 keys vector-ALU) of those queries is all -inf, no row is fully masked
        qi = torch.arange(c.T)
        bias[:, qi % 3 == 0, :64] = float("-inf")
        bias[:, qi % 3 == 1, 32:64] = float("-inf")
        assert bool(torch.isfinite(bias).any(-1).all())
    return [None if t is None else t.double() for t in (q, k, v, do, bias)]


def _reference(c, q, k, v, do, bias, mask=None, dtype=torch.float64):
    qr, kr, vr = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    s = qr @ kr.transpose(-1, -2) * (c.A ** -0.5)
    if bias is not None:
        s = s + bias.to(dtype)[torch.arange(c.BH) % c.nbias]
    p = torch.softmax(s, -1)
    if mask is not None:
        p = p * mask.to(dtype)
    out = p @ vr
    out.backward(do.to(dtype))
    return dict(out=out.detach(), lse=torch.logsumexp(s.detach(), -1), dq=qr.grad, dk=kr.grad,
                dv=vr.grad)


def _rel(a, b):
    b = b.double()
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))


def _dev(t, cuda, offset=False):
    """`t` as an fp32 device tensor; `offset`: contiguous, but one element (4 bytes) into a 16-byte
    aligned storage, as a view that starts inside a larger buffer is."""
    if t is None:
        return None
    t = t.float()
    if not offset:
        return t.to(cuda)
    buf = torch.zeros(t.numel() + 1, device=cuda, dtype=torch.float32)
    view = buf[1:].view(t.shape)
    view.copy_(t.to(cuda))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _keep_mask(cuda, c, qd, kd, bd, scale):
    """The keep mask of (SEED, OFFSET) scaled by 1 / (1 - p), read off the vector-ALU forward with
    identity V in column blocks of at most 256; the kept probabilities are the undropped ones."""
    kept = torch.empty(c.BH, c.T, c.T, dtype=torch.bool)
    with _lib.tuning(attn_nomfma=1):
        for c0 in range(0, c.T, 256):
            w = min(256, c.T - c0)
            assert ops.attention_plan(c.T, c.A, w).path == "valu"
            eye = torch.eye(c.T, device=cuda)[:, c0:c0 + w].expand(c.BH, c.T, w).contiguous()
            pt, _ = ops.attention_fwd(qd, kd, eye, bd, scale, P_DROP, SEED, OFFSET)
            p0, _ = ops.attention_fwd(qd, kd, eye, bd, scale)
            blk = pt != 0
            assert torch.allclose(pt[blk], p0[blk] / (1 - P_DROP), rtol=1e-5, atol=1e-8)
            kept[:, :, c0:c0 + w] = blk.cpu()
    frac = kept.float().mean().item()
    assert abs(frac - (1 - P_DROP)) < 0.01, frac
    return kept.double() / (1 - P_DROP)


BARS = dict(out=1e-5, lse=1e-5, dq=5e-5, dk=5e-5, dv=5e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_case_matches_torch_fp64(cuda, case):
    c = case
    plans = _plans(c)
    assert not _mismatch(c, plans), plans
    q, k, v, do, bias = _inputs(c)
    off = "unaligned" in c.opt
    qd, kd, vd, dod = (_dev(t, cuda, off) for t in (q, k, v, do))
    bd = _dev(bias, cuda)
    scale = c.A ** -0.5
    drop = (P_DROP, SEED, OFFSET) if "drop" in c.opt else ()
    mask = _keep_mask(cuda, c, qd, kd, bd, scale) if drop else None
    ref = _reference(c, q, k, v, do, bias, mask)
    assert all(bool(torch.isfinite(t).all()) for t in ref.values())

    out, lse = ops.attention_fwd(qd, kd, vd, bd, scale, *drop)
    dq, dk, dv = ops.attention_bwd(qd, kd, vd, bd, out, dod, lse, scale, *drop)
    torch.cuda.synchronize()
    got = dict(out=out, lse=lse, dq=dq, dk=dk, dv=dv)
    if "functional" in c.opt:
        from adell_mri_amd import functional as HF

        leaves = [t.clone().requires_grad_(True) for t in (qd, kd, vd)]
        fo = HF.attention(*leaves, bd)
        fo.backward(dod)
        torch.cuda.synchronize()
        for name, t in zip(("out", "dq", "dk", "dv"), (fo.detach(), *[t.grad for t in leaves])):
            assert torch.equal(t, got[name]), name
    got = {n: t.cpu() for n, t in got.items()}
    assert all(bool(torch.isfinite(t).all()) for t in got.values()), "non-finite result"

    bars = dict(BARS)
    if "large" in c.opt:
        # the bar is 4 x the error of torch's own fp32 CPU evaluation where that exceeds the standing one
        ref32 = _reference(c, q, k, v, do, bias, mask, torch.float32)
        e32 = {n: _rel(ref32[n], ref[n]) for n in BARS}
        bars = {n: max(BARS[n], 4 * e32[n]) for n in BARS}
        print(f"{_case_id(c)}: torch fp32 CPU", {n: f"{e:.2e}" for n, e in e32.items()})
    errs = {n: _rel(got[n], ref[n]) for n in BARS}
    print(_case_id(c), "/".join(p.path for p in plans), {n: f"{e:.2e}" for n, e in errs.items()})
    bad = {n: (e, bars[n]) for n, e in errs.items() if not e < bars[n]}
    assert not bad, f"'{c.branch}' {_case_id(c)}: relative error above the bound: {bad}"


@pytest.mark.gpu
def test_one_unaligned_operand_runs_the_vector_alu_kernels(cuda):
    """Any single operand one element into its storage sends the call to the vector-ALU kernels (the
    MFMA ones stage with 16-byte loads): bit-identical to the same call under attn_nomfma."""
    c = next(c for c in CASES if "unaligned" in c.opt)
    assert all(p.path == "valu" for p in _plans(c))       # settled on the host before anything runs
    q, k, v, do, _ = _inputs(c)
    scale = c.A ** -0.5
    al = [_dev(t, cuda) for t in (q, k, v, do)]
    with _lib.tuning(attn_nomfma=1):
        out0, lse0 = ops.attention_fwd(*al[:3], None, scale)
        grads0 = ops.attention_bwd(*al[:3], None, out0, al[3], lse0, scale)
    for i, name in enumerate(("q", "k", "v", "dout")):
        t = list(al)
        t[i] = _dev((q, k, v, do)[i], cuda, offset=True)
        if i < 3:
            out, lse = ops.attention_fwd(*t[:3], None, scale)
            assert torch.equal(out, out0) and torch.equal(lse, lse0), name
        grads = ops.attention_bwd(*t[:3], None, out0, t[3], lse0, scale)
        for g, g0 in zip(grads, grads0):
            assert torch.equal(g, g0), name


@pytest.mark.gpu
def test_head_dims_above_256_are_refused_by_forward_and_backward(cuda):
    z = torch.zeros(1, 5, 257, device=cuda)
    s = torch.zeros(1, 5, 8, device=cuda)
    lse = torch.zeros(1, 5, device=cuda)
    for q, v in ((z, s), (s, z)):
        with pytest.raises(_lib.AdellHipError):
            ops.attention_fwd(q, q, v, None, 1.0)
        with pytest.raises(_lib.AdellHipError):
            ops.attention_bwd(q, q, v, None, v, v, lse, 1.0)
