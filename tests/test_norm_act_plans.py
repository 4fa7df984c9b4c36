"""Every route of a norm -> dropout -> activation site (csrc/norm_act.hip adell_na_plan: scalar, float4,
fast and narrow kernels forward and backward, the low-rank and from-dt backward, three finalize kernels,
the two-level statistics fold, keep bits), from one case table:

- on the build host (no GPU), each case still gets the plan it is in the table for (ops.norm_act_plan:
  the function the launchers take their decisions from), every branch has exactly one case, and the
  table has a case on each side of every threshold, the thresholds read off the plan query. A retune
  that moves a shape onto another kernel, or a case deleted from the table, fails here naming the branch;
- on the GPU, each case runs through ops.channel_partials / stats_finalize / norm_act_fwd / norm_act_bwd
  (and, by option, norm_act_bwd_lowrank, norm_act_bwd_sums + norm_act_bwd_apply_sums, prelu_wgrad)
  against torch fp64 autograd on the CPU of the formula in the header of norm_act.hip:
  out = act(dropout((x - mean) * rstd * gamma + beta)).

Bars (the ones tests/test_ops_gpu.py and the layer sweep hold): largest error over the largest reference
value, 2e-5 for out, 5e-5 for dx, 2e-4 for dgamma, dbeta and dact_w, 1e-4 for mean and rstd. Beside each
case stands how far torch's own fp32 CPU evaluation of the formula is from fp64 on the same inputs
(measured once on the build host: out, dx, and the largest of the parameter gradients); where 4 x that
number exceeds the standing bar, the case's bar is 4 x the number.

Dropout: the keep mask is a function of (seed, offset, global element index) alone -- Philox-4x32 as
csrc/common.h describes it, restated in numpy below and checked once against the scalar kernel; every
other route must reproduce it bit for bit, the stored keep bits included."""
import collections
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch

from adell_mri_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-5
P_DROP, SEED, OFFSET = 0.15, 0x1234567891011, 7

# stats: "inst" / "batch" / None. aw: PReLU weights, 0 (none), 1 or "C". opt: "mask" keep bits wanted;
# "x_off" / "dout_off" that operand one element (4 bytes) into a 16-byte aligned storage; "lowrank" also
# norm_act_bwd_lowrank with 2 factors; "sums" also norm_act_bwd_sums + norm_act_bwd_apply_sums.
# plan: fields of ops.norm_act_plan the case pins. noise: torch fp32 CPU against fp64 (out, dx, params).
Case = collections.namedtuple("Case", "branch N C size stats affine act aw drop opt plan noise")


def _p(fwd, bwd, fin, **kw):
    return dict(fwd=fwd, bwd=bwd, finalize=fin, **kw)


CASES = [
    # ---- the generic kernels past one grid (the grid cap is 4096 blocks of 256 threads) ------------
    Case("scalar: grid-stride above the grid cap", 1, 6, (57, 57, 57), "inst", False, "swish", 0, 0.15,
         set(), _p("scalar", "scalar", "per_item", fwd_grid=(4096, 1), apply_grid=(4096, 1), rows=181),
         (2.1e-07, 2.4e-07, 0.0)),
    Case("float4: grid-stride above the grid cap", 2, 24, (45, 45, 45), "batch", True, "gelu", 0, 0.15,
         set(), _p("float4", "float4", "all_items", fwd_grid=(4096, 1), apply_grid=(4096, 1), rows=89),
         (1.8e-07, 2.0e-07, 1.3e-07)),
    # ---- the fast kernels: 1024 partial rows per item at most, then 2048-float4 chunks and idle blocks
    Case("fast: partial rows at the cap, idle blocks", 1, 64, (41, 41, 41), "inst", False, "tanh", 0,
         0.0, set(), _p("fast", "fast", "per_item", fwd_grid=(1077, 1), rows=1024),
         (1.9e-07, 1.9e-07, 0.0)),
    Case("fast: 519 slabs, two-level statistics", 1, 4, (81, 81, 81), "inst", False, "elu", 0, 0.0,
         set(), _p("fast", "fast", "per_item", rows=519), (9.9e-08, 1.5e-07, 0.0)),
    Case("fast: C 1024, three items, batch statistics", 3, 1024, (3, 3, 5), "batch", True, "prelu", "C",
         0.15, {"sums"}, _p("fast", "fast", "all_items", fwd_grid=(12, 3), rows=12),
         (1.9e-07, 1.7e-07, 2.1e-07)),
    Case("float4: C 2048 is past the fast kernels", 1, 2048, (3, 3, 5), "inst", False, "sigmoid", 0,
         0.15, set(), _p("float4", "float4", "per_item", fwd_grid=(90, 1), rows=1),
         (1.2e-07, 2.0e-07, 0.0)),
    # ---- one and two channels: narrow while a float4 holds whole voxels of one item ----------------
    Case("narrow: C 2, even volume", 2, 2, (12, 10, 9), "inst", True, "prelu", "C", 0.15, set(),
         _p("narrow", "narrow", "all_items", rows=1), (8.0e-08, 1.1e-07, 4.0e-07)),
    Case("scalar: C 2, odd volume", 2, 2, (9, 7, 5), "inst", True, "prelu", "C", 0.15, set(),
         _p("scalar", "scalar", "all_items", rows=1), (1.2e-07, 1.5e-07, 2.0e-07)),
    Case("narrow: C 1, batch statistics", 3, 1, (12, 10, 9), "batch", True, "sigmoid", 0, 0.0,
         {"sums"}, _p("narrow", "narrow", "all_items", rows=1), (9.4e-08, 1.9e-07, 6.3e-07)),
    Case("scalar: C 1, volume no multiple of 4", 1, 1, (9, 7, 5), "inst", False, "tanh", 0, 0.15,
         set(), _p("scalar", "scalar", "per_item", rows=1), (1.1e-07, 1.4e-07, 0.0)),
    # ---- keep bits: the last group of an item with fewer than four float4, and full groups ---------
    Case("mask tail: C 4, V 65", 2, 4, (5, 13, 1), "inst", False, "identity", 0, 0.15, {"mask"},
         _p("fast", "fast", "per_item", mask_bytes=2 * 2 * 32), (1.2e-07, 1.1e-07, 0.0)),
    Case("mask tail: C 8, V 33", 2, 8, (3, 11, 1), "inst", False, "swish", 0, 0.15, {"mask"},
         _p("fast", "fast", "per_item", mask_bytes=2 * 2 * 32), (1.7e-07, 1.3e-07, 0.0)),
    Case("mask: full groups and a part group", 3, 32, (5, 5, 5), "inst", True, "leaky_relu", 0, 0.15,
         {"mask"}, _p("fast", "fast", "all_items", mask_bytes=3 * 16 * 32), (1.3e-07, 1.8e-07, 1.7e-07)),
    # ---- operands that are not 16-byte aligned ------------------------------------------------------
    Case("unaligned: x and dout one element in", 2, 32, (7, 6, 5), "inst", False, "relu", 0, 0.15,
         {"x_off", "dout_off"}, _p("scalar", "scalar", "per_item"), (1.2e-07, 1.4e-07, 0.0)),
    Case("unaligned dout: forward fast, backward scalar", 2, 16, (7, 6, 5), "inst", False, "gelu", 0,
         0.15, {"dout_off"}, _p("fast", "scalar", "per_item"), (1.3e-07, 1.2e-07, 0.0)),
    Case("unaligned x: C 24 off the float4 kernels", 1, 24, (7, 6, 5), "batch", False, "elu", 0, 0.15,
         {"x_off"}, _p("scalar", "scalar", "all_items"), (1.1e-07, 1.8e-07, 0.0)),
    # ---- low-rank upstream gradient -----------------------------------------------------------------
    Case("lowrank: two factors on the fast kernels", 2, 16, (9, 8, 7), "inst", False, "swish", 0, 0.15,
         {"lowrank"}, _p("fast", "fast", "per_item"), (1.7e-07, 1.6e-07, 0.0)),
    # ---- which finalize runs ------------------------------------------------------------------------
    Case("finalize none: no statistics, no affine gradients", 2, 8, (7, 6, 5), None, False, "gelu", 0,
         0.15, set(), _p("fast", "fast", "none", rows=0, workspace=0), (1.1e-07, 1.6e-07, 0.0)),
    Case("finalize all-items: affine gradients without statistics", 2, 12, (7, 6, 5), None, True,
         "prelu", 1, 0.0, set(), _p("float4", "float4", "all_items", rows=1), (5.3e-08, 3.3e-08, 1.9e-07)),
    Case("finalize all-items: instance statistics with affine gradients", 3, 3, (7, 6, 5), "inst", True,
         "leaky_relu", 0, 0.0, set(), _p("scalar", "scalar", "all_items", rows=1),
         (1.4e-07, 1.3e-07, 9.0e-08)),
    # ---- the per-item finalize keeps two rows in flight from 33 rows --------------------------------
    Case("per-item finalize: 32 rows", 1, 3, (32, 32, 32), "inst", False, "swish", 0, 0.0, set(),
         _p("scalar", "scalar", "per_item", rows=32), (1.5e-07, 2.4e-07, 0.0)),
    # (65538 voxel rows: prelu_wgrad in chunks of 68 rows, 964 partial rows for its 16-lane final fold)
    Case("per-item finalize: 33 rows", 2, 3, (9, 11, 331), "inst", False, "prelu", "C", 0.0, set(),
         _p("scalar", "scalar", "per_item", rows=33), (1.3e-07, 1.7e-07, 4.4e-07)),
]

# every branch has exactly one case: deleting a case fails test_table_covers_every_branch by name
BRANCHES = [
    "scalar: grid-stride above the grid cap", "float4: grid-stride above the grid cap",
    "fast: partial rows at the cap, idle blocks", "fast: 519 slabs, two-level statistics",
    "fast: C 1024, three items, batch statistics", "float4: C 2048 is past the fast kernels",
    "narrow: C 2, even volume", "scalar: C 2, odd volume", "narrow: C 1, batch statistics",
    "scalar: C 1, volume no multiple of 4",
    "mask tail: C 4, V 65", "mask tail: C 8, V 33", "mask: full groups and a part group",
    "unaligned: x and dout one element in", "unaligned dout: forward fast, backward scalar",
    "unaligned x: C 24 off the float4 kernels",
    "lowrank: two factors on the fast kernels",
    "finalize none: no statistics, no affine gradients",
    "finalize all-items: affine gradients without statistics",
    "finalize all-items: instance statistics with affine gradients",
    "per-item finalize: 32 rows", "per-item finalize: 33 rows",
]

# partial rows per item of the synthetic statistics chains, channels of those chains
STATS_NTILES = (1, 7, 8, 9, 56, 57, 64, 65, 512, 513, 769)
STATS_C = (1, 31, 32, 33)
# the chains norm_act_bwd_from_dt folds (C = 32 only: it needs the fast kernels): also 32 and 33 rows
FROM_DT_NTILES = STATS_NTILES + (32, 33)
# rows per item after the first level of the fold, for the chains that have one
STATS_Z = {512: 0, 513: 3, 769: 4}

BARS = dict(out=2e-5, dx=5e-5, dgamma=2e-4, dbeta=2e-4, dact_w=2e-4, mean=1e-4, rstd=1e-4)


def _case_id(c):
    tags = "".join("_" + t for t in sorted(c.opt))
    return (f"n{c.N}_c{c.C}_{'x'.join(map(str, c.size))}_{c.stats}_{'aff' if c.affine else 'noaff'}_"
            f"{c.act}{c.aw or ''}_p{c.drop}{tags}")


def _V(c):
    return c.size[0] * c.size[1] * c.size[2]


def _plan(c, **kw):
    una = tuple(n for n in ("x", "dout") if n + "_off" in c.opt)
    args = dict(stats_per_item=0 if c.stats == "batch" else 1, drop_p=c.drop, unaligned=una,
                want_mask="mask" in c.opt, norm=c.stats is not None, affine_grads=c.affine)
    args.update(kw)
    return ops.norm_act_plan(c.N, _V(c), c.C, **args)


def _mismatch(c, plan):
    return [f"{k}: {getattr(plan, k)} != {v}" for k, v in c.plan.items() if getattr(plan, k) != v]


# ---- build host: the table against the plan query ------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_plan_of_case(case):
    plan = _plan(case)
    bad = _mismatch(case, plan)
    assert not bad, (f"branch '{case.branch}' lost its case {_case_id(case)}: {bad}; the planner now "
                     f"gives {plan}. Update the case table so the branch keeps a case.")
    # what the query reports is what the sizing entry points report
    d = _lib.NormActDesc(case.N, _V(case), case.C, 1, 0, 0, 0.0, case.drop, 0, 0)
    ws = _lib.lib().adell_norm_act_bwd_workspace(ctypes.byref(d))
    assert plan.workspace == (ws if plan.finalize != "none" else 0)
    if plan.mask_bytes:
        assert plan.mask_bytes == _lib.lib().adell_norm_act_mask_bytes(ctypes.byref(d))
    assert plan.workspace >= 4 * (case.N * plan.rows * case.C * 2 + 2 * case.N * case.C) * (plan.rows > 0)
    if "lowrank" in case.opt:
        assert _plan(case, lowrank=2).bwd == "fast"


def test_table_covers_every_branch():
    have = [c.branch for c in CASES]
    assert len(set(have)) == len(have), "a branch has two cases: give each its own tag"
    missing = [b for b in BRANCHES if b not in have]
    assert not missing, f"no case for: {missing}"
    assert not set(have) - set(BRANCHES), f"not in BRANCHES: {sorted(set(have) - set(BRANCHES))}"
    assert len(CASES) <= 40
    ids = [_case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids), "two cases share an id (and with it their inputs)"
    assert all(c.N * _V(c) * c.C <= 4_500_000 for c in CASES), "a case above 4.5 M elements"


def test_table_selects_every_route_it_promises():
    """Counted on the plans themselves: all four kernels forward and backward, all three finalize
    kinds, dropout on every route, per-channel PReLU on the narrow route and at the widest fast C,
    all nine activations, N of 1 and 3, every statistics mode."""
    plans = [(c, _plan(c)) for c in CASES]
    routes = {"scalar", "float4", "fast", "narrow"}
    assert {p.fwd for _, p in plans} == routes and {p.bwd for _, p in plans} == routes
    assert {p.finalize for _, p in plans} == {"none", "per_item", "all_items"}
    assert {p.fwd for c, p in plans if c.drop} == routes and {p.bwd for c, p in plans if c.drop} == routes
    assert any(p.fwd != p.bwd and c.drop for c, p in plans), "no dropout case whose passes differ in route"
    assert any(p.fwd == "narrow" and c.aw == "C" for c, p in plans)
    cmax = _widest_fast_c()
    assert any(p.fwd == "fast" and c.C == cmax and c.aw == "C" for c, p in plans)
    acts = {(c.act, c.aw) for c in CASES}
    assert {a for a, _ in acts} == {"identity", "swish", "relu", "leaky_relu", "prelu", "gelu", "sigmoid",
                                    "tanh", "elu"}
    assert {("prelu", 1), ("prelu", "C")} <= acts
    # prelu_wgrad: a case whose row chunks are past the smallest chunk, with more partial rows than the
    # 16 lanes of its final fold (the chunking is read off the workspace it asks for: 4 C bytes a chunk)
    chunks = []
    for c in CASES:
        if c.act == "prelu":
            d = _lib.NormActDesc(c.N, _V(c), c.C, 1, ops.ACT_IDS["prelu"], c.C, 0.0, 0.0, 0, 0)
            nb = _lib.lib().adell_prelu_wgrad_workspace(ctypes.byref(d)) // (4 * c.C)
            chunks.append((-(-c.N * _V(c) // nb), nb))
    assert min(ch for ch, _ in chunks) < max(ch for ch, _ in chunks) and any(
        ch > min(chunks)[0] and nb > 16 for ch, nb in chunks), chunks
    assert {1, 3} <= {c.N for c in CASES}
    assert {c.stats for c in CASES} == {"inst", "batch", None}
    assert {(c.stats, c.affine) for c in CASES} >= {("inst", True), ("inst", False), ("batch", True),
                                                     ("batch", False), (None, True), (None, False)}


def _widest_fast_c():
    """Largest power-of-two C the plan query gives the fast kernels."""
    fast = [C for C in (2 ** k for k in range(2, 16)) if ops.norm_act_plan(1, 64, C).fwd == "fast"]
    assert fast == [2 ** k for k in range(2, 2 + len(fast))], fast
    return fast[-1]


def _generic_cap():
    """Grid cap of the generic kernels, and the threads of a block, read off the query."""
    cap = ops.norm_act_plan(1, 1 << 34, 3).fwd_grid[0]
    assert ops.norm_act_plan(1, 1 << 35, 3).fwd_grid[0] == cap
    # N items of one voxel and one channel are N elements on the scalar kernel
    threads = next(n for n in range(1, 1 << 12) if ops.norm_act_plan(n + 1, 1, 1).fwd_grid[0] == 2)
    assert ops.norm_act_plan(cap * threads, 1, 1).fwd_grid == (cap, 1)
    assert ops.norm_act_plan(cap * threads - threads, 1, 1).fwd_grid == (cap - 1, 1)
    return cap, cap * threads


def _fast_rows_cap():
    """Cap of the fast partials kernel's rows per item and the float4 of a row below it."""
    cap = ops.norm_act_plan(1, 1 << 34, 4).rows
    assert ops.norm_act_plan(1, 1 << 35, 4).rows == cap
    per = next(V for V in range(1, 1 << 14) if ops.norm_act_plan(1, V + 1, 4).rows == 2)
    return cap, cap * per


def test_table_has_a_case_on_each_side_of_every_threshold():
    """The thresholds come from the plan query, not from this file: a retune of a cap or of a loop
    moves them, and the table then has to move with them."""
    plans = [(c, _plan(c)) for c in CASES]
    missing = []
    # generic grid cap: a case whose units (float4 or elements) exceed one grid by less than 2 x, on
    # both generic kernels, forward and backward; cases below it
    cap, units = _generic_cap()
    for route, per in (("scalar", 1), ("float4", 4)):
        n = [(c.N * _V(c) * c.C // per, p) for c, p in plans if p.fwd == route and p.bwd == route]
        if not any(units < u <= 2 * units and p.fwd_grid[0] == cap == p.apply_grid[0] for u, p in n):
            missing.append(f"{route}: no case just above the grid cap of {cap} blocks ({units} units)")
        if not any(u <= units and p.fwd_grid[0] < cap for u, p in n):
            missing.append(f"{route}: no case below the grid cap")
    # fast partials: rows at the cap with more float4 than cap x 1024 (2048-float4 chunks, idle blocks)
    rcap, n4cap = _fast_rows_cap()
    fast = [(_V(c) * c.C // 4, p) for c, p in plans if p.bwd == "fast" and p.rows]
    if not any(n4cap < n4 <= 2 * n4cap and p.rows == rcap for n4, p in fast):
        missing.append(f"fast: no case just above {rcap} partial rows ({n4cap} float4 per item)")
    if not any(rcap // 2 < p.rows < rcap for _, p in fast):
        missing.append(f"fast: no case with more than half of, but fewer than, {rcap} partial rows")
    # the finalize kernels' row loops, the two-level fold
    sp = ops.norm_act_stats_plan(1, 1, 1)
    for r in (sp.unroll2_from - 1, sp.unroll2_from):
        if not any(p.finalize == "per_item" and p.rows == r for _, p in plans):
            missing.append(f"per-item finalize: no case with {r} rows")
        if r not in FROM_DT_NTILES:
            missing.append(f"from_dt chains: no chain of {r} rows")
    for r in (sp.unroll8_from - 1, sp.unroll8_from):
        if r not in STATS_NTILES:
            missing.append(f"statistics chains: no chain of {r} rows")
    levels = [ops.norm_act_stats_plan(1, t, 1).levels for t in range(1, 4097)]
    fold = levels.count(1)
    assert levels == [1] * fold + [2] * (4096 - fold)
    for r in (fold, fold + 1):
        if r not in STATS_NTILES or r not in FROM_DT_NTILES:
            missing.append(f"statistics chains: no chain of {r} rows (the fold starts above {fold})")
    # rows one block of the first level folds: Z goes from 2 to 3 one row past two full blocks
    per = (next(t for t in range(fold + 1, 1 << 14) if ops.norm_act_stats_plan(1, t, 1).Z == 3) - 1) // 2
    for t, z in STATS_Z.items():
        if ops.norm_act_stats_plan(1, t, 1).Z != z:
            missing.append(f"two-level fold: a chain of {t} rows folds to {ops.norm_act_stats_plan(1, t, 1).Z} "
                           f"rows, not {z} ({per} rows per block)")
    if not any(t > fold and t % per == 1 and t // per >= 3 for t in STATS_NTILES):
        missing.append(f"statistics chains: no chain of three full blocks of {per} rows and one row more")
    if not any(ops.norm_act_stats_plan(1, ops_ntiles(_V(c)), 1).levels == 2 for c, _ in plans):
        missing.append(f"no case whose channel_partials give more than {fold} rows")
    # widest fast C, narrow against scalar, N
    cmax = _widest_fast_c()
    if not any(c.C == cmax and p.fwd == "fast" and p.bwd == "fast" for c, p in plans):
        missing.append(f"no fast case at C = {cmax}")
    if not any(c.C == 2 * cmax and p.fwd == "float4" and p.bwd == "float4" for c, p in plans):
        missing.append(f"no float4 case at C = {2 * cmax}")
    for C in (1, 2):
        for want, ok in (("narrow", lambda v: v % 4 == 0), ("scalar", lambda v: v % 4 != 0)):
            if not any(c.C == C and ok(_V(c) * C) and p.fwd == want == p.bwd for c, p in plans):
                missing.append(f"no {want} case at C = {C}")
    assert any(c.C == 2 and _V(c) % 2 == 0 for c in CASES) and any(c.C == 2 and _V(c) % 2 for c in CASES)
    assert not missing, f"the thresholds moved away from the table's cases: {missing}"


def ops_ntiles(V):
    return _lib.lib().adell_channel_partials_ntiles(int(V))


def test_plan_refuses_what_the_launchers_refuse():
    P = ops.norm_act_plan
    # keep bits and split rows exist on the fast route alone
    assert P(2, 65, 4, drop_p=0.15, want_mask=True).fwd == "fast"
    assert P(2, 65, 4, drop_p=0.15, want_mask=True).mask_bytes == 2 * 2 * 32
    assert P(2, 65, 4, drop_p=0.0, want_mask=True).mask_bytes == 0          # no dropout: nothing stored
    for kw in (dict(C=6), dict(C=2), dict(C=2048), dict(C=4, unaligned=("x",)),
               dict(C=4, unaligned=("out",))):
        C = kw.pop("C")
        assert P(2, 64, C, drop_p=0.15, want_mask=True, **kw).fwd == "refused", (C, kw)
        assert P(2, 64, C, split=True, **kw).fwd == "refused", (C, kw)
    assert P(2, 64, 8, split=True).fwd == "refused" and P(2, 64, 16, split=True).fwd == "fast"
    assert P(2, 64, 2, drop_p=0.15).fwd == "narrow"
    # the low-rank backward needs the fast kernels proper
    assert P(2, 64, 16, lowrank=2).bwd == "fast"
    for kw in (dict(C=2), dict(C=24), dict(C=2048), dict(C=16, unaligned=("x",)),
               dict(C=16, unaligned=("dx",))):
        C = kw.pop("C")
        assert P(2, 64, C, lowrank=2, **kw).bwd == "refused", (C, kw)
    # one unaligned tensor moves only the pass that reads or writes it
    assert (P(2, 64, 16, unaligned=("out",)).fwd, P(2, 64, 16, unaligned=("out",)).bwd) == ("scalar", "fast")
    assert (P(2, 64, 16, unaligned=("dx",)).fwd, P(2, 64, 16, unaligned=("dx",)).bwd) == ("fast", "scalar")
    # per-item finalize up to the grid's 65535 rows
    assert P(65535, 4, 4).finalize == "per_item" and P(65536, 4, 4).finalize == "all_items"
    # the 65535-block cap of the fast forward and dx grids (268 M elements per item: no GPU case)
    assert P(1, 1 << 26, 4).fwd_grid == (65535, 1) and P(1, 1 << 26, 4).apply_grid == (65535, 1)
    assert P(1, (1 << 26) - 1024, 4).fwd_grid == (65535, 1) and P(1, (1 << 26) - 2048, 4).fwd_grid == (65534, 1)


def _aligned_pointer():
    buf = (ctypes.c_float * 64)()             # never dereferenced: the calls fail before a launch
    a = (ctypes.addressof(buf) + 15) & ~15
    return buf, ctypes.c_void_p(a)


def test_workspace_of_the_plan_is_what_the_entry_points_require():
    """One byte less than the query reports is refused as too small; with the reported size the call
    gets as far as the null-pointer check (both before any HIP call: no GPU needed)."""
    h = _lib.lib()
    keep, p = _aligned_pointer()

    def refused_as(rc, word):
        assert rc == _lib.E_BADARG, rc
        assert word in h.adell_last_error(), h.adell_last_error()

    for N, V, C, spi, affine in ((1, 57 ** 3, 6, 1, False), (2, 41 ** 3, 64, 0, True), (3, 45, 1024, 1, False),
                                 (2, 315, 2, 1, True)):
        plan = ops.norm_act_plan(N, V, C, stats_per_item=spi, affine_grads=affine)
        d = _lib.NormActDesc(N, V, C, spi, 0, 0, 0.0, 0.0, 0, 0)
        ws = plan.workspace
        assert ws > 0
        g = p if affine else None
        refused_as(h.adell_norm_act_bwd(ctypes.byref(d), p, p, p, p, None, None, None, p, g, g, p, ws - 1,
                                        None), b"workspace too small")
        refused_as(h.adell_norm_act_bwd(ctypes.byref(d), None, p, p, p, None, None, None, p, g, g, p, ws,
                                        None), b"null pointer")
        if ops.norm_act_plan(N, V, C, lowrank=2).bwd == "fast":
            refused_as(h.adell_norm_act_bwd_lowrank(ctypes.byref(d), p, p, p, 2, p, p, p, p, ws - 1, None),
                       b"workspace too small")
        if spi == 0:
            refused_as(h.adell_norm_act_bwd_sums(ctypes.byref(d), p, p, p, p, None, None, None, p, g, g, p,
                                                 ws - 1, None), b"workspace too small")
            refused_as(h.adell_norm_act_bwd_sums(ctypes.byref(d), p, p, p, p, None, None, None, None, g, g,
                                                 p, ws, None), b"null record")
    # without statistics and affine gradients there is no reduction pass and no workspace
    d = _lib.NormActDesc(2, 64, 8, 1, 0, 0, 0.0, 0.0, 0, 0)
    assert ops.norm_act_plan(2, 64, 8, norm=False).workspace == 0
    refused_as(h.adell_norm_act_bwd(ctypes.byref(d), None, p, None, None, None, None, None, p, None, None,
                                    None, 0, None), b"null pointer")
    # statistics chains
    for N, nt, C in ((2, 512, 33), (2, 513, 33), (3, 769, 4)):
        sp = ops.norm_act_stats_plan(N, nt, C)
        assert sp.workspace == h.adell_stats_finalize_workspace(N, nt, C)
        assert sp.workspace == (4 * N * sp.Z * C * 2 if sp.levels == 2 else 0)
        if sp.levels == 2:
            refused_as(h.adell_stats_finalize(p, N, nt, C, 64, 1e-5, 1, p, p, p, sp.workspace - 1, None),
                       b"workspace too small")
            refused_as(h.adell_bn_stats_sums(p, N, nt, C, 64, p, p, sp.workspace - 1, None),
                       b"workspace too small")
        refused_as(h.adell_stats_finalize(None, N, nt, C, 64, 1e-5, 1, p, p, p, sp.workspace, None),
                   b"null pointer")
        refused_as(h.adell_bn_stats_sums(None, N, nt, C, 64, p, p, sp.workspace, None), b"null pointer")
        if C == 4:
            d = _lib.NormActDesc(N, 48, C, 1, 0, 0, 0.0, 0.0, 0, 0)
            need = sp.workspace + 4 * 2 * N * C
            refused_as(h.adell_norm_act_bwd_from_dt(ctypes.byref(d), p, p, p, p, p, nt, C + 4, 2, p, p,
                                                    need - 1, None), b"workspace too small")
            refused_as(h.adell_norm_act_bwd_from_dt(ctypes.byref(d), None, p, p, p, p, nt, C + 4, 2, p, p,
                                                    need, None), b"null pointer")
    del keep


# ---- the dropout mask, restated ------------------------------------------------------------------

def _philox_rounds():
    src = open(os.path.join(ROOT, "adell_mri_amd", "csrc", "common.h")).read()
    return int(re.search(r"#define\s+ADELL_PHILOX_ROUNDS\s+(\d+)", src).group(1))


def _philox4(c0, c1, c2, c3, k0, k1, rounds):
    """Philox-4x32 as csrc/common.h states it (32-bit words held in uint64 arrays)."""
    lo32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & lo32 for c in np.broadcast_arrays(c0, c1, c2, c3))
    for _ in range(rounds):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & lo32, p1 >> np.uint64(32), p1 & lo32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def _keep(total, p=P_DROP, seed=SEED, offset=OFFSET):
    """Keep flags of elements 0 .. total - 1 of a tensor in memory order: counter = (float4 index low,
    float4 index high, offset, 0), key = the seed's halves, word e & 3, u = (word >> 8) 2^-24, kept
    when u >= p (the graph step counter is 0 in eager runs)."""
    i = np.arange((total + 3) // 4, dtype=np.uint64)
    w = _philox4(i, i >> np.uint64(32), offset, 0, seed & 0xFFFFFFFF, seed >> 32, _philox_rounds())
    words = np.stack(w, 1).reshape(-1)[:total]
    u = (words >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u >= np.float32(p)


def _mask_words(keep, N, VC):
    """The keep bits as the forward stores them: element el of item n is bit (el >> 2) & 63 of word
    (n * groups + (el >> 8)) * 4 + (el & 3); bits past the end of an item are 0."""
    groups = (VC + 255) // 256
    padded = np.zeros((N, groups * 256), dtype=np.uint64)
    padded[:, :VC] = keep.reshape(N, VC)
    bits = padded.reshape(N, groups, 64, 4) << np.arange(64, dtype=np.uint64)[None, None, :, None]
    return np.bitwise_or.reduce(bits, axis=2).reshape(-1)


def test_keep_restatement_is_a_fair_generator():
    """Host check of the restatement itself: the kept fraction, and independence of the four words."""
    k = _keep(1 << 18)
    assert abs(k.mean() - (1 - P_DROP)) < 4e-3, k.mean()
    assert abs(k.reshape(-1, 4).mean(0) - (1 - P_DROP)).max() < 6e-3
    assert not np.array_equal(k, _keep(1 << 18, offset=OFFSET + 1))
    assert not np.array_equal(k, _keep(1 << 18, seed=SEED + 1))
    w = _mask_words(_keep(2 * 260), 2, 260).reshape(2, 2, 4)
    assert int(w[0, 1].max()) < 2 and int(w[1, 1].max()) < 2       # 260 elements: one float4 in group 1


# ---- the formula, in torch on the CPU ------------------------------------------------------------

_KINKED = {"relu": 0.0, "leaky_relu": 0.0, "prelu": 0.0}
ACT_P = {"leaky_relu": 0.1, "elu": 1.0}


def _act(name, u, p):
    if name == "identity":
        return u
    if name == "swish":
        return u * torch.sigmoid(u)
    if name == "relu":
        return torch.relu(u)
    if name in ("leaky_relu", "prelu"):
        return torch.where(u > 0, u, p * u)
    if name == "gelu":
        return 0.5 * u * (1.0 + torch.erf(u * 0.7071067811865476))
    if name == "sigmoid":
        return torch.sigmoid(u)
    if name == "tanh":
        return torch.tanh(u)
    if name == "elu":
        return torch.where(u > 0, u, p * (torch.exp(torch.clamp(u, max=0.0)) - 1.0))
    raise KeyError(name)


_INPUTS = {}


def _inputs(c):
    """fp32-representable operands as fp64 tensors in memory order [N, V, C] (the reference sees exactly
    what the kernels do), computed once per case and left unchanged."""
    key = _case_id(c)
    if key in _INPUTS:
        return _INPUTS[key]
    g = torch.Generator().manual_seed(zlib.crc32(key.encode()))
    N, V, C = c.N, _V(c), c.C
    t = dict(x=torch.randn(N, V, C, generator=g) * 1.5 + 0.5 * torch.randn(1, 1, C, generator=g) + 0.25)
    if "lowrank" in c.opt:
        t["g"] = torch.randn(N, V, 2, generator=g)
        t["w"] = torch.randn(2, C, generator=g)
    else:
        t["dout"] = torch.randn(N, V, C, generator=g)
    if c.affine:
        t["gamma"] = 1.0 + 0.3 * torch.randn(C, generator=g)
        t["beta"] = 0.3 * torch.randn(C, generator=g)
    if c.aw:
        t["act_w"] = 0.25 + 0.1 * torch.randn(C if c.aw == "C" else 1, generator=g)
    t = {k: v.double() for k, v in t.items()}
    if c.drop:
        t["keep"] = torch.from_numpy(_keep(N * V * C, c.drop).reshape(N, V, C))
    _INPUTS[key] = t
    return t


def _reference(c, t, dtype=torch.float64):
    x = t["x"].to(dtype).clone().requires_grad_(True)
    leaves = {k: t[k].to(dtype).clone().requires_grad_(True) for k in ("gamma", "beta", "act_w") if k in t}
    h = x
    res = {}
    if c.stats is not None:
        dims = (1,) if c.stats == "inst" else (0, 1)
        mean = x.mean(dims, keepdim=True)
        var = ((x - mean) ** 2).mean(dims, keepdim=True)
        rstd = 1.0 / torch.sqrt(var + EPS)
        h = (x - mean) * rstd
        res["mean"] = mean.detach().reshape(-1, c.C) if c.stats == "inst" else mean.detach().reshape(c.C)
        res["rstd"] = rstd.detach().reshape(res["mean"].shape)
    if c.affine:
        h = h * leaves["gamma"] + leaves["beta"]
    if c.drop:
        scale = 1.0 / (1.0 - float(np.float32(c.drop)))
        h = h * (t["keep"].to(dtype) * scale)
    if c.act in _KINKED:
        # the derivative jumps at 0: the inputs keep clear of it (else the case is ill-posed in fp32)
        live = h.detach()[t["keep"]] if c.drop else h.detach()
        assert float(live.abs().min()) > 1e-6, "an input on the activation's kink"
    p = leaves["act_w"] if c.aw else ACT_P.get(c.act, 0.0)
    out = _act(c.act, h, p)
    dout = (t["g"].to(dtype) @ t["w"].to(dtype)) if "lowrank" in c.opt else t["dout"].to(dtype)
    out.backward(dout)
    res.update(out=out.detach(), dx=x.grad)
    if c.affine:
        res.update(dgamma=leaves["gamma"].grad, dbeta=leaves["beta"].grad)
    if c.aw:
        res["dact_w"] = leaves["act_w"].grad
    return res


def _rel(a, b):
    b = b.double()
    return float((a.double().reshape(b.shape) - b).abs().max() / (b.abs().max() + 1e-300))


def reference_noise(c):
    """torch fp32 CPU against fp64 on the case's inputs: (out, dx, largest parameter gradient). The
    numbers in the table's `noise` column; run on the build host when a case is added or changed."""
    t = _inputs(c)
    r64, r32 = _reference(c, t), _reference(c, t, torch.float32)
    par = [_rel(r32[k], r64[k]) for k in ("dgamma", "dbeta", "dact_w") if k in r64]
    return _rel(r32["out"], r64["out"]), _rel(r32["dx"], r64["dx"]), max(par, default=0.0)


def _bars(c):
    n_out, n_dx, n_par = c.noise
    bars = dict(BARS)
    bars["out"] = max(BARS["out"], 4 * n_out)
    bars["dx"] = max(BARS["dx"], 4 * n_dx)
    for k in ("dgamma", "dbeta", "dact_w"):
        bars[k] = max(BARS[k], 4 * n_par)
    return bars


@pytest.mark.parametrize("case", [c for c in CASES if c.N * _V(c) * c.C <= 200_000], ids=_case_id)
def test_recorded_reference_noise_is_not_understated(case):
    """The small cases measured again: no more than 4 x the recorded number (the largest error of a few
    thousand fp32 results, and the order of torch's fp32 sums depends on the host's thread count), and a
    gradient the case does not have is recorded as 0."""
    got = reference_noise(case)
    for name, g, want in zip(("out", "dx", "params"), got, case.noise):
        assert g <= 4 * want and (g > 0) == (want > 0), (name, g, want)
    assert _bars(case) == BARS, "4 x the reference noise of a small case is below every standing bar"


# ---- GPU: every case against torch fp64 on the CPU ----------------------------------------------

def _dev(t, c, cuda, offset=False):
    """[N, V, C] values as an fp32 device tensor of logical shape [N, C, D, H, W] in NDHWC memory;
    `offset`: one element (4 bytes) into a 16-byte aligned storage."""
    n, _, ch = t.shape
    buf = torch.zeros(t.numel() + 4, device=cuda, dtype=torch.float32)
    o = 1 if offset else 0
    flat = buf[o:o + t.numel()]
    flat.copy_(t.reshape(-1).float().to(cuda))
    view = flat.view(n, *c.size, ch).permute(0, 4, 1, 2, 3)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * o
    return view


def _nvc(t):
    """Device result [N, C, D, H, W] (NDHWC memory) as a CPU tensor [N, V, C]."""
    return t.permute(0, 2, 3, 4, 1).reshape(t.shape[0], -1, t.shape[1]).cpu()


def _poison(nbytes, cuda):
    """Leave a freed block of all-ones bits for the next allocation of this size to land on (the
    caching allocator hands back the block just freed): a word the kernel does not write shows."""
    junk = torch.full((max(nbytes // 8, 1),), -1, device=cuda, dtype=torch.int64)
    torch.cuda.synchronize()
    del junk


@pytest.mark.gpu
def test_keep_restatement_matches_the_scalar_kernel(cuda):
    """The restated mask against the scalar kernel (C = 3 on one and on four batch items, past a block
    and with a total that is no multiple of 4): identity activation, no norm, so out is x / (1 - p)
    where kept and 0 where dropped."""
    for N, size in ((1, (7, 11, 13)), (4, (5, 7, 9))):
        c = Case("", N, 3, size, None, False, "identity", 0, P_DROP, set(), {}, ())
        assert _plan(c).fwd == "scalar"
        x = torch.rand(N, _V(c), 3) + 0.5
        out = _nvc(ops.norm_act_fwd(_dev(x, c, cuda), None, None, "identity", drop_p=P_DROP, seed=SEED,
                                    rng_offset=OFFSET))
        keep = torch.from_numpy(_keep(x.numel()).reshape(x.shape))
        assert torch.equal(out != 0, keep)
        assert torch.allclose(out[keep], x[keep] / (1 - P_DROP), rtol=1e-6)
        other = _nvc(ops.norm_act_fwd(_dev(x, c, cuda), None, None, "identity", drop_p=P_DROP, seed=SEED,
                                      rng_offset=OFFSET + 1))
        assert torch.equal(other != 0, torch.from_numpy(_keep(x.numel(), offset=OFFSET + 1).reshape(x.shape)))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_case_matches_torch_fp64(cuda, case):
    c = case
    plan = _plan(c)
    assert not _mismatch(c, plan), plan
    t = _inputs(c)
    ref = _reference(c, t)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    N, V, C = c.N, _V(c), c.C
    spi = 0 if c.stats == "batch" else 1
    xd = _dev(t["x"], c, cuda, "x_off" in c.opt)
    dev = {k: t[k].float().to(cuda) for k in ("gamma", "beta", "act_w") if k in t}
    gamma, beta, act_w = dev.get("gamma"), dev.get("beta"), dev.get("act_w")
    kw = dict(act_p=ACT_P.get(c.act, 0.0), drop_p=c.drop, seed=SEED, rng_offset=OFFSET)
    got = {}
    mean = rstd = None
    if c.stats is not None:
        part = ops.channel_partials(xd)
        assert part.shape[1] == ops_ntiles(V)
        mean, rstd = ops.stats_finalize(part, V, EPS, per_item=c.stats == "inst")
        got.update(mean=mean, rstd=rstd)

    want_mask = "mask" in c.opt
    if want_mask:
        _poison(plan.mask_bytes, cuda)
    fwd = ops.norm_act_fwd(xd, mean, rstd, c.act, gamma, beta, act_w, stats_per_item=spi,
                           want_mask=want_mask, **kw)
    out, mask = fwd if want_mask else (fwd, None)
    got["out"] = _nvc(out)
    if "lowrank" in c.opt:
        gd = _dev(t["g"], c, cuda)
        wd = t["w"].float().to(cuda)
        got["dx"] = _nvc(ops.norm_act_bwd_lowrank(xd, gd, wd, mean, rstd, c.act, **kw))
        doutd = _dev(t["g"].float().double() @ t["w"], c, cuda)       # the full dout, rounded to fp32
        full = ops.norm_act_bwd(xd, doutd, mean, rstd, c.act, stats_per_item=spi, **kw)[0]
        got["dx_full_dout"] = _nvc(full)
    else:
        doutd = _dev(t["dout"], c, cuda, "dout_off" in c.opt)
        dx, dg, db = ops.norm_act_bwd(xd, doutd, mean, rstd, c.act, gamma, beta, act_w, stats_per_item=spi,
                                      want_affine_grads=c.affine, **kw)
        got["dx"] = _nvc(dx)
        if c.affine:
            got.update(dgamma=dg, dbeta=db)
    if c.aw:
        got["dact_w"] = ops.prelu_wgrad(xd, doutd, mean, rstd, act_w, gamma, beta, spi, c.drop, SEED, OFFSET)
    if "sums" in c.opt:
        rec, dg2, db2 = ops.norm_act_bwd_sums(xd, doutd, mean, rstd, c.act, gamma, beta, act_w,
                                              want_affine_grads=c.affine, **kw)
        dx2 = ops.norm_act_bwd_apply_sums(xd, doutd, mean, rstd, rec, c.act, gamma, beta, act_w, **kw)
        got.update(dx_sums=_nvc(dx2), dgamma_sums=dg2, dbeta_sums=db2)
        assert float(rec[2 * C]) == N * V
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, v in got.items()}
    assert all(bool(torch.isfinite(v).all()) for v in got.values()), "non-finite result"

    if c.drop:
        # the route reproduces the restated mask bit for bit (a dropped element is act(0) = 0 for every
        # activation the dropout cases use but sigmoid, whose 0.5 is no value of a kept element here)
        # (relu, and gelu where erf rounds to -1, give kept elements the dropped value too; a flipped flag
        # there still shows in dx)
        zero, keep = (0.5 if c.act == "sigmoid" else 0.0), t["keep"]
        assert bool((got["out"][~keep] == zero).all()), f"'{c.branch}': the forward kept a dropped element"
        if c.act not in ("relu", "gelu"):
            assert bool((got["out"][keep] != zero).all()), f"'{c.branch}': the forward dropped a kept element"
        if c.stats is None:
            assert bool((got["dx"][~keep] == 0).all()), f"'{c.branch}': the backward kept a dropped element"
    if want_mask:
        words = mask.cpu().numpy().view(np.uint64)
        want = _mask_words(t["keep"].numpy(), N, V * C)
        assert words.shape == want.shape == (plan.mask_bytes // 8,)
        bad = np.nonzero(words != want)[0]
        assert bad.size == 0, (f"'{c.branch}': keep-bit words {bad[:8].tolist()} (of {words.size}; word = "
                               f"(item * groups + group) * 4 + sub-element) differ from the restated mask: "
                               f"{[hex(int(w)) for w in words[bad[:8]]]} != "
                               f"{[hex(int(w)) for w in want[bad[:8]]]}")

    bars = _bars(c)
    errs = {}
    for name, v in got.items():
        base = name.split("_")[0] if name not in ("dact_w",) else name
        errs[name] = (_rel(v, ref[base]), bars[base])
    print(_case_id(c), f"{plan.fwd}/{plan.bwd}/{plan.finalize}", {n: f"{e:.2e}" for n, (e, _) in errs.items()})
    bad = {n: eb for n, eb in errs.items() if not eb[0] < eb[1]}
    assert not bad, f"'{c.branch}' {_case_id(c)}: relative error above the bound: {bad}"


@pytest.mark.gpu
def test_mask_and_split_rows_are_refused_off_the_fast_route(cuda):
    for C, off in ((6, False), (2, False), (2048, False), (8, True)):
        c = Case("", 2, C, (4, 4, 4), None, False, "identity", 0, P_DROP, set(), {}, ())
        x = _dev(torch.randn(2, 64, C), c, cuda, off)
        assert ops.norm_act_plan(2, 64, C, drop_p=P_DROP, want_mask=True,
                                 unaligned=("x",) if off else ()).fwd == "refused"
        with pytest.raises(_lib.AdellHipError, match="unsupported"):
            ops.norm_act_fwd(x, None, None, "identity", drop_p=P_DROP, seed=SEED, want_mask=True)
        if C == 2048:
            with pytest.raises(_lib.AdellHipError):
                ops.norm_act_fwd(x, None, None, "identity", split_exp=0)


# ---- statistics chains ---------------------------------------------------------------------------

def _chain(N, nt, C, seed):
    """Synthetic partial rows [N, nt, C, 2] of 64 elements each: (sum, sum of squares) of values around
    a per-channel mean with a variance above 1, as fp32."""
    g = torch.Generator().manual_seed(seed)
    mu = 0.5 * torch.randn(1, 1, C, generator=g)
    sig2 = 1.0 + torch.rand(1, 1, C, generator=g)
    s1 = 64.0 * (mu + 0.05 * torch.randn(N, nt, C, generator=g))
    s2 = 64.0 * (mu * mu + sig2) * (1.0 + 0.05 * torch.randn(N, nt, C, generator=g))
    return torch.stack([s1, s2], -1).float()


def _stats64(rows, count, dims):
    s = rows.double().sum(dims)
    n = count * (rows.shape[0] if 0 in dims else 1)
    m = s[..., 0] / n
    var = (s[..., 1] / n - m * m).clamp_min(0.0)
    return s, m, 1.0 / torch.sqrt(var + EPS)


@pytest.mark.gpu
@pytest.mark.parametrize("C", STATS_C)
def test_statistics_chain_matches_the_fp64_sum_of_its_rows(cuda, C):
    """stats_finalize (both modes), bn_stats_sums and bn_stats_from_sums on synthetic rows against the
    fp64 sum of the same fp32 rows. The kernels add fp32 rows in fp64 (the two-level fold rounds its
    256-row sums to fp32 once: 6e-8), so the bar is 1e-6 on mean and rstd."""
    N = 3
    for nt in STATS_NTILES:
        rows = _chain(N, nt, C, 1000 * C + nt)
        rd = rows.to(cuda)
        count = 64 * nt
        sp = ops.norm_act_stats_plan(N, nt, C)
        assert sp.levels == (2 if nt > 512 else 1)
        worst = {}
        _, m, r = _stats64(rows, count, (1,))
        gm, gr = ops.stats_finalize(rd, count, EPS, per_item=True)
        worst["item mean"], worst["item rstd"] = _rel(gm.cpu(), m), _rel(gr.cpu(), r)
        s, m, r = _stats64(rows, count, (0, 1))
        gm, gr = ops.stats_finalize(rd, count, EPS, per_item=False)
        worst["batch mean"], worst["batch rstd"] = _rel(gm.cpu(), m), _rel(gr.cpu(), r)
        rec = ops.bn_stats_sums(rd, count)
        want = torch.cat([s[:, 0], s[:, 1], torch.tensor([float(N * count)], dtype=torch.float64)])
        assert float(rec[2 * C]) == N * count
        worst["record sums"] = _rel(rec.cpu()[:C], want[:C])
        worst["record squares"] = _rel(rec.cpu()[C:2 * C], want[C:2 * C])
        gm, gr = ops.bn_stats_from_sums(rec, EPS)
        worst["record mean"], worst["record rstd"] = _rel(gm.cpu(), m), _rel(gr.cpu(), r)
        bad = {k: v for k, v in worst.items() if not v < 1e-6}
        assert not bad, f"C {C}, {nt} rows ({sp.levels} level(s)): {bad}"


@pytest.mark.gpu
def test_from_dt_folds_wide_rows_at_an_offset(cuda):
    """norm_act_bwd_from_dt on synthetic rows that are columns [poff, poff + C) of rows pstride wide (the
    other columns hold NaN): dx = rstd (dt - c1 - xhat c2) with c1, c2 the fp64 sums of the rows over V."""
    N, C, size, pstride, poff = 2, 32, (4, 4, 3), 44, 5
    V = size[0] * size[1] * size[2]
    c = Case("", N, C, size, "inst", False, "identity", 0, 0.0, set(), {}, ())
    g = torch.Generator().manual_seed(77)
    x = (torch.randn(N, V, C, generator=g) * 1.5 + 0.25).double()
    dt = torch.randn(N, V, C, generator=g).double()
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + EPS)
    mean, rstd = mean.float(), rstd.float()
    for nt in FROM_DT_NTILES:
        assert ops.norm_act_plan(N, V, C).bwd == "fast"
        rows = (_chain(N, nt, C, 500 + nt) * (V / (64.0 * nt))).float()
        wide = torch.full((N, nt, pstride, 2), float("nan"))
        wide[:, :, poff:poff + C] = rows
        s = rows.double().sum(1)
        c1, c2 = s[..., 0] / V, s[..., 1] / V
        xhat = (x - mean.double()[:, None]) * rstd.double()[:, None]
        want = rstd.double()[:, None] * (dt - c1[:, None] - xhat * c2[:, None])
        dtd = _dev(dt, c, cuda)
        got = _nvc(ops.norm_act_bwd_from_dt(_dev(x, c, cuda), dtd, mean.to(cuda), rstd.to(cuda),
                                            wide.to(cuda), poff))
        assert bool(torch.isfinite(got).all()), nt
        e = _rel(got, want)
        assert e < BARS["dx"], (nt, e)


def _slab_emulation(x, V, C):
    """(mean, rstd) per item from per-slab float32 sums (1024 voxels a slab) added in float64: what the
    channel_partials -> stats_finalize chain computes, up to the order within a slab."""
    x = x.numpy().astype(np.float32)
    s1 = np.zeros((x.shape[0], C)), np.zeros((x.shape[0], C))
    for v0 in range(0, V, 1024):
        blk = x[:, v0:v0 + 1024]
        s1[0][:] += blk.sum(1, dtype=np.float32).astype(np.float64)
        s1[1][:] += (blk * blk).sum(1, dtype=np.float32).astype(np.float64)
    m = s1[0] / V
    var = np.maximum(s1[1] / V - m * m, 0.0)
    return torch.from_numpy(m), torch.from_numpy(1.0 / np.sqrt(var + EPS))


# rstd of the slab emulation against fp64 at (m, s) = (20, 1), measured on the build host (C = 3, C = 4)
OFFSET_EMULATION_RSTD = {3: 2.5e-04, 4: 1.6e-04}


def _real(C, m, s):
    g = torch.Generator().manual_seed(100 * C + int(10 * m))
    return (torch.randn(2, 17 * 17 * 17, C, generator=g) * s + m).float()


def test_offset_inputs_lose_m_over_s_squared_in_the_slab_sums():
    """Build host: the recorded emulation error at (20, 1) is what the emulation gives."""
    for C, want in OFFSET_EMULATION_RSTD.items():
        x = _real(C, 20.0, 1.0)
        _, r = _slab_emulation(x, x.shape[1], C)
        r64 = 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + EPS)
        e = _rel(r, r64)
        assert abs(e - want) <= 0.25 * want, (C, e)


@pytest.mark.gpu
@pytest.mark.parametrize("C", (3, 4))
def test_statistics_of_real_tensors(cuda, C):
    """channel_partials (scalar form at C = 3, float4 form at C = 4, and the scalar form on an unaligned
    C = 4 tensor) -> stats_finalize on x = s randn + m, per item and over the batch, against fp64. At
    (20, 1) E[x^2] - E[x]^2 over fp32 slab sums loses about (m / s)^2 of relative precision: the bar for
    rstd there is 4 x the error of the slab emulation (floor 1e-6), a characterisation, not a gate."""
    size = (17, 17, 17)
    c = Case("", 2, C, size, "inst", False, "identity", 0, 0.0, set(), {}, ())
    V = 17 ** 3
    for m, s in ((0.0, 1.0), (1.5, 3.0), (20.0, 1.0)):
        x = _real(C, m, s)
        x64 = x.double()
        for off in ((False, True) if C == 4 else (False,)):
            part = ops.channel_partials(_dev(x64, c, cuda, off))
            assert part.shape == (2, 5, C, 2)
            for per_item in (True, False):
                dims = (1,) if per_item else (0, 1)
                mean = x64.mean(dims)
                rstd = 1.0 / torch.sqrt(((x64 - x64.mean(dims, keepdim=True)) ** 2).mean(dims) + EPS)
                gm, gr = ops.stats_finalize(part, V, EPS, per_item=per_item)
                em, er = _rel(gm.cpu(), mean), _rel(gr.cpu(), rstd)
                bar_m, bar_r = BARS["mean"], BARS["rstd"]
                if m == 20.0:
                    bar_r = max(4 * OFFSET_EMULATION_RSTD[C], 1e-6)
                print(f"C {C} (m, s) ({m}, {s}) offset {off} per_item {per_item}: mean {em:.2e} rstd {er:.2e}")
                assert em < bar_m and er < bar_r, (m, s, off, per_item, em, er, bar_r)
