"""Every launch plan of the two GEMM families behind Linear layers (csrc/gemm.hip adell_gemm_f32_plan;
csrc/gemm_f16x3.hip adell_gemm_h_plan with csrc/gemm_rows.hip adell_gemm_rows_plan), from one case table:

- on the build host (no GPU), each case still gets the route and the plan fields it is in the table for
  in every layout it lists (ops.gemm_plan: the function the launchers and the workspace queries take
  their decisions from), every branch has exactly one case, and the limits the table sits on -- the CU
  count the streaming kernel compares its tile count against, the K at which the fold's thread groups
  change, the K at which the pack rows halve -- are read off the query. A retune that moves a shape onto
  another kernel, or a case deleted from the table, fails here naming the branch;
- on the GPU, each case runs through ops.gemm, ops.gemm_f16x3 or ops.gemm_f16x3_act in each of its
  layouts against fp64 on the CPU; a case the f16x3 family refuses asserts the refusal. The rows that
  came from the shape lists of test_gemm_gpu.py::test_gemm_layouts_match_float64 and
  test_gemm_f16x3_gpu.py::test_layouts_against_fp64 run under those ids, one layout (and one absmax-word
  setting) per id, from this table and through check_f32_case / check_f16x3_case below.

Layouts: "nt" forward X W^T (A and B k-contiguous), "nn" backward-data dY W (B outer-contiguous), "tn"
backward-weight dY^T X (both outer-contiguous), "tt" (A outer-contiguous, B k-contiguous).

Bars and metrics (the ones tests/test_gemm_gpu.py and tests/test_gemm_f16x3_gpu.py held for the shape
lists this table absorbed): fp32 family 2e-6 * max(1, sqrt(K) / 8), the largest error over the largest
reference value, reference = the fp64 product of the fp32 operands; f16x3 family 2e-6, the largest error
over the largest sum |a||b|, with bias and residual. The activation outputs hold the family's bar on the
same scale: |act'| <= 1.13 for GELU and SiLU, so act(C) and C act'(z) carry the GEMM's error times that,
and the GEMM's own error is an order of magnitude inside the bar (printed per case).

The rows cases with K >= 4096 need a 130 - 530 MB operand: it is drawn on the device, and the fp64
reference is taken on four whole 256-row tiles (the first, a middle one, the last two)."""
import collections
from unittest import mock

import numpy as np
import pytest
import torch

from adell_mri_amd import _lib, ops

LAYOUTS = {"nt": (True, True), "nn": (True, False), "tn": (False, False), "tt": (False, True)}
Case = collections.namedtuple("Case", "branch family M N K plan opt")


def F(branch, M, N, K, nt=None, nn=None, tn=None, opt=()):
    """fp32 case; per layout "route[/reduce]" (None: the layout is not run)."""
    return Case(branch, "f32", M, N, K, {k: v for k, v in dict(nt=nt, nn=nn, tn=tn).items() if v}, set(opt))


def H(branch, M, N, K, nt=None, nn=None, tn=None, tt=None, opt=()):
    """f16x3 case; per layout "refused", "rows/R<pack rows>[/gelu]" or "tile/wide|narrow[/s<S>v<V>]" (the
    fold's thread groups and width). opt: "former" (FORMER) a shape of a former list; "offset_a" /
    "offset_bias": that operand one element into its storage; "gelu" / "swish": act_out with that
    activation; "dact": dact_in (GELU)."""
    return Case(branch, "f16x3", M, N, K,
                {k: v for k, v in dict(nt=nt, nn=nn, tn=tn, tt=tt).items() if v}, set(opt))


def _all(spec, layouts="nt nn tn"):
    return {k: spec for k in layouts.split()}


SQ, SK = "tile_square", "tile_skinny"
FORMER = {"former"}      # a shape of one of the two former shape lists: runs under its former test id
W4 = _all("tile/wide", "nt nn tn tt")

CASES = [
    # ---- fp32: the shapes test_gemm_layouts_match_float64 listed, with the routes they take ---------
    F("f32 1x1x1", 1, 1, 1, **_all(SK), opt=FORMER),
    F("f32 tile_skinny, one split, three layouts", 7, 5, 3, **_all(SK), opt=FORMER),
    F("f32 tile_skinny, tree", 16, 1024, 768, **_all(SK + "/tree"), opt=FORMER),
    F("f32 tile_square, one split, three layouts", 33, 130, 50, **_all(SQ), opt=FORMER),
    F("f32 128x768x3072", 128, 768, 3072, **_all(SQ + "/tree"), opt=FORMER),
    F("f32 300x96x384", 300, 96, 384, **_all(SQ + "/flat"), opt=FORMER),
    F("f32 1024x384x1536", 1024, 384, 1536, **_all(SQ + "/tree"), opt=FORMER),
    F("f32 4099x97x96", 4099, 97, 96, **_all(SQ), opt=FORMER),
    F("f32 tall_small: M N below 8", 2, 2, 70000, nt=SK + "/tree", nn=SK + "/tree", tn="tall_small/tree", opt=FORMER),
    F("f32 ragged tile edges", 65, 257, 129, **_all(SQ + "/flat"), opt=FORMER),
    F("f32 flat at its last split count (8)", 864, 512, 512, **_all(SQ + "/flat"), opt=FORMER),
    F("f32 864x1536x512", 864, 1536, 512, **_all(SQ + "/flat"), opt=FORMER),
    F("f32 4100x520x72", 4100, 520, 72, **_all(SQ), opt=FORMER),
    F("f32 rows_small 8 <- 2", 70000, 8, 2, nt="rows_small", nn="rows_small", tn=SQ, opt=FORMER),
    F("f32 rows_small 2 <- 8, odd M", 70001, 2, 8, nt="rows_small", nn="rows_small", tn=SQ, opt=FORMER),
    F("f32 rows_small 32 <- 8: the block cap", 66000, 32, 8, nt="rows_small", nn="rows_small", tn=SQ, opt=FORMER),
    F("f32 rows_small, N not a power of two", 65540, 12, 5, nt="rows_small", nn="rows_small", tn=SQ, opt=FORMER),
    F("f32 tall_lds 2x8", 2, 8, 70000, nt=SK + "/tree", nn=SK + "/tree", tn="tall_lds/tree", opt=FORMER),
    F("f32 tall_lds 8x32", 8, 32, 20000, nt=SK + "/tree", nn=SK + "/tree", tn="tall_lds/tree", opt=FORMER),
    F("f32 tall_small: M N = 1024", 32, 32, 16400, nt=SK + "/tree", nn=SK + "/tree", tn="tall_small/tree", opt=FORMER),
    F("f32 tall_small: not powers of two", 5, 3, 33000, nt=SK + "/tree", nn=SK + "/tree",
      tn="tall_small/tree", opt=FORMER),
    F("f32 rows_small 8 <- 32", 70000, 8, 32, nt="rows_small", nn="rows_small", tn=SQ, opt=FORMER),
    F("f32 rows_small 64 <- 8", 66000, 64, 8, nt="rows_small", nn="rows_small", tn=SQ, opt=FORMER),
    F("f32 rows_small 8 <- 64", 65540, 8, 64, nt="rows_small", nn="rows_small", tn=SQ, opt=FORMER),
    F("f32 rows_small 16 <- 32", 70000, 16, 32, nt="rows_small", nn="rows_small", tn=SQ, opt=FORMER),
    F("f32 tall_lds 8x2: two outputs per thread", 8, 2, 70000, nt=SK + "/tree", nn=SK + "/tree",
      tn="tall_lds/tree", opt=FORMER),
    F("f32 tall_lds 64x8, K % 64 != 0", 64, 8, 16388, nt=SQ + "/tree", nn=SQ + "/tree", tn="tall_lds/tree", opt=FORMER),
    F("f32 tall_lds 8x64", 8, 64, 65600, nt=SK + "/tree", nn=SK + "/tree", tn="tall_lds/tree", opt=FORMER),
    F("f32 tall_lds 32x8", 32, 8, 100000, nt=SK + "/tree", nn=SK + "/tree", tn="tall_lds/tree", opt=FORMER),
    F("f32 tall_lds 16x16 at K 16384", 16, 16, 16384, nt=SK + "/tree", nn=SK + "/tree", tn="tall_lds/tree", opt=FORMER),
    F("f32 tall_lds 2x4, K % 64 != 0", 2, 4, 16388, nt=SK + "/tree", nn=SK + "/tree", tn="tall_lds/tree", opt=FORMER),
    # ---- fp32: branches that had no case ------------------------------------------------------------
    # torch's own fp32 CPU product against fp64 on these inputs, in the test's metric, measured on the build
    # host: flat (2) 4.4e-7, tree 3.3e-7, skinny flat 3.3e-7, M 65536 6.5e-8, M 65535 3.9e-8, N K 512 3.8e-7,
    # N K 513 2.8e-7, tall_lds M N 8 4.1e-7, M N 512 2.7e-7, offset A 4.1e-7, K 16383 5.2e-7: four times
    # each is below the family's bar (2.0e-6 .. 3.2e-5 by K), which holds
    F("f32 flat at its first split count (2)", 128, 128, 128, **_all(SQ + "/flat")),
    F("f32 tree, 16 splits", 128, 128, 1024, **_all(SQ + "/tree")),
    F("f32 tile_skinny, flat", 16, 130, 128, **_all(SK + "/flat")),
    F("f32 rows_small at M 65536, both b_kc", 65536, 2, 2, nt="rows_small", nn="rows_small", tn=SQ),
    F("f32 M 65535: tile neighbour of rows_small", 65535, 2, 2, nt=SQ, nn=SQ),
    F("f32 rows_small at N K 512", 65536, 8, 64, nt="rows_small", nn="rows_small"),
    F("f32 N K 513: tile neighbour of rows_small", 65536, 9, 57, nt=SQ, nn=SQ),
    F("f32 tall_lds at K 16384, M N 8", 2, 4, 16384, tn="tall_lds/tree"),
    F("f32 tall_lds at K 16384, M N 512", 8, 64, 16384, tn="tall_lds/tree"),
    F("f32 tall_small: A one element into its storage", 2, 4, 16384, tn="tall_small/tree", opt={"offset_a"}),
    F("f32 K 16383: tile neighbour of the tall kernels", 2, 4, 16383, tn=SK + "/tree"),
    # ---- f16x3: the shapes test_layouts_against_fp64 listed (each with and without absmax words) ----
    H("f16x3 tile, one split, four layouts, wide", 128, 128, 32, **W4, opt=FORMER),
    H("f16x3 256x384x96", 256, 384, 96, **W4, opt=FORMER),
    H("f16x3 ragged single tile", 100, 36, 64, **W4, opt=FORMER),
    H("f16x3 4x8x4", 4, 8, 4, **W4, opt=FORMER),
    H("f16x3 ragged tiles and stages", 1000, 132, 260, **W4, opt=FORMER),
    H("f16x3 64x3072x768: three splits", 64, 3072, 768, **_all("tile/wide/s1v4", "nt nn tn tt"),
      opt=FORMER),
    H("f16x3 4096x96x384", 4096, 96, 384, **W4, opt=FORMER),
    # ---- f16x3 tile: branches that had no case ------------------------------------------------------
    # torch fp32 CPU against fp64 over sum |a||b| on these inputs (build host): narrow 1.5e-7 / 1.4e-7; fold
    # S 1 / 4 / 16 1.2e-7 / 4.2e-8 / 2.4e-8, at the limits 6.3e-8, 5.7e-8, 2.5e-8, 2.6e-8; width 1 1.1e-7 /
    # 4.2e-8 / 3.0e-8; act_out, dact_in 1.4e-7, through the fold 1.2e-7: four times each is below 2e-6
    H("f16x3 narrow epilogue: N % 4 != 0", 100, 38, 64, nt="tile/narrow", tt="tile/narrow", nn="refused",
      tn="refused"),
    H("f16x3 narrow epilogue: bias one element into its storage", 100, 36, 64, nn="tile/narrow",
      tn="tile/narrow", opt={"offset_bias"}),
    H("f16x3 fold S 1", 128, 128, 512, **_all("tile/wide/s1v4", "nt tn")),
    H("f16x3 fold S 4", 128, 128, 2048, **_all("tile/wide/s4v4", "nt tn")),
    H("f16x3 fold S 16", 128, 128, 8192, **_all("tile/wide/s16v4", "nt tn")),
    H("f16x3 fold: last K with S 1", 128, 128, 1984, nt="tile/wide/s1v4"),
    H("f16x3 fold: first K with S 4", 128, 128, 1988, nt="tile/wide/s4v4"),
    H("f16x3 fold: last K before S 16", 128, 128, 8128, nt="tile/wide/s4v4"),
    H("f16x3 fold: first K with S 16", 128, 128, 8132, nt="tile/wide/s16v4"),
    H("f16x3 fold width 1, S 1", 128, 126, 512, nt="tile/narrow/s1v1", tt="tile/narrow/s1v1"),
    H("f16x3 fold width 1, S 4", 128, 126, 2048, nt="tile/narrow/s4v1"),
    H("f16x3 fold width 1, S 16", 128, 126, 8192, nt="tile/narrow/s16v1"),
    H("f16x3 act_out on the tiles", 100, 36, 64, nt="tile/wide", nn="tile/wide", opt={"swish"}),
    H("f16x3 dact_in on the tiles", 100, 36, 64, nt="tile/wide", nn="tile/wide", opt={"dact"}),
    H("f16x3 dact_in through the fold", 128, 128, 512, nn="tile/wide/s1v4", opt={"dact"}),
    # ---- f16x3 refused ------------------------------------------------------------------------------
    H("f16x3 refused: K % 4", 100, 36, 66, **_all("refused", "nt nn tn tt")),
    H("f16x3 refused: outer-contiguous M % 4", 102, 36, 64, nt="tile/wide", nn="tile/wide", tn="refused",
      tt="refused"),
    H("f16x3 refused: A one element into its storage", 100, 36, 64, **_all("refused", "nt nn tn tt"),
      opt={"offset_a"}),
    # ---- f16x3 rows: 12 column slices x 22 row tiles is the first count of at least 256 CUs ----------
    # torch fp32 CPU against fp64 (build host): limit 2.2e-7, below it 2.1e-7, pack rows 16 / 8 / 4 1.8e-7 /
    # 1.3e-7 / 8.5e-8, GELU pair and the two tile neighbours 2.2e-7 (pack rows 2 and 1: operands drawn on
    # the device, not measured): the bar of 2e-6 holds
    H("f16x3 rows at the tile-count limit, both b_kc", 5377, 1536, 32, nt="rows/R8", nn="rows/R32"),
    H("f16x3 one row tile below the rows limit", 5376, 1536, 32, nt="tile/wide", nn="tile/wide"),
    H("f16x3 rows, pack rows 16 (outer B)", 5377, 1536, 512, nt="rows/R8", nn="rows/R16"),
    H("f16x3 rows, pack rows 8 (outer B)", 5377, 1536, 1024, nt="rows/R8", nn="rows/R8"),
    H("f16x3 rows, pack rows 4", 5377, 1536, 2048, nt="rows/R4", nn="rows/R4"),
    H("f16x3 rows, pack rows 2", 7937, 1024, 4096, nt="rows/R2", nn="rows/R2"),
    H("f16x3 rows, pack rows 1", 16129, 512, 8192, nt="rows/R1", nn="rows/R1"),
    H("f16x3 rows, GELU pair", 5377, 1536, 32, nt="rows/R8/gelu", opt={"gelu"}),
    H("f16x3 rows shape, dact_in: the tiles", 5377, 1536, 32, nn="tile/wide", opt={"dact"}),
    H("f16x3 rows shape, another activation: the tiles", 5377, 1536, 32, nt="tile/wide", opt={"swish"}),
]

# every branch has exactly one case: deleting a case fails test_table_covers_every_branch by name
BRANCHES = [
    "f32 1x1x1", "f32 tile_skinny, one split, three layouts", "f32 tile_skinny, tree",
    "f32 tile_square, one split, three layouts", "f32 128x768x3072", "f32 300x96x384", "f32 1024x384x1536",
    "f32 4099x97x96", "f32 tall_small: M N below 8", "f32 ragged tile edges",
    "f32 flat at its last split count (8)", "f32 864x1536x512", "f32 4100x520x72", "f32 rows_small 8 <- 2",
    "f32 rows_small 2 <- 8, odd M", "f32 rows_small 32 <- 8: the block cap",
    "f32 rows_small, N not a power of two", "f32 tall_lds 2x8", "f32 tall_lds 8x32",
    "f32 tall_small: M N = 1024", "f32 tall_small: not powers of two", "f32 rows_small 8 <- 32",
    "f32 rows_small 64 <- 8", "f32 rows_small 8 <- 64", "f32 rows_small 16 <- 32",
    "f32 tall_lds 8x2: two outputs per thread", "f32 tall_lds 64x8, K % 64 != 0", "f32 tall_lds 8x64",
    "f32 tall_lds 32x8", "f32 tall_lds 16x16 at K 16384", "f32 tall_lds 2x4, K % 64 != 0",
    "f32 flat at its first split count (2)", "f32 tree, 16 splits", "f32 tile_skinny, flat", "f32 rows_small at M 65536, both b_kc",
    "f32 M 65535: tile neighbour of rows_small", "f32 rows_small at N K 512",
    "f32 N K 513: tile neighbour of rows_small", "f32 tall_lds at K 16384, M N 8",
    "f32 tall_lds at K 16384, M N 512", "f32 tall_small: A one element into its storage",
    "f32 K 16383: tile neighbour of the tall kernels",
    "f16x3 tile, one split, four layouts, wide", "f16x3 256x384x96", "f16x3 ragged single tile", "f16x3 4x8x4",
    "f16x3 ragged tiles and stages", "f16x3 64x3072x768: three splits", "f16x3 4096x96x384",
    "f16x3 narrow epilogue: N % 4 != 0", "f16x3 narrow epilogue: bias one element into its storage",
    "f16x3 fold S 1", "f16x3 fold S 4", "f16x3 fold S 16", "f16x3 fold: last K with S 1",
    "f16x3 fold: first K with S 4", "f16x3 fold: last K before S 16", "f16x3 fold: first K with S 16",
    "f16x3 fold width 1, S 1", "f16x3 fold width 1, S 4", "f16x3 fold width 1, S 16",
    "f16x3 act_out on the tiles", "f16x3 dact_in on the tiles", "f16x3 dact_in through the fold",
    "f16x3 refused: K % 4", "f16x3 refused: outer-contiguous M % 4",
    "f16x3 refused: A one element into its storage",
    "f16x3 rows at the tile-count limit, both b_kc", "f16x3 one row tile below the rows limit",
    "f16x3 rows, pack rows 16 (outer B)", "f16x3 rows, pack rows 8 (outer B)", "f16x3 rows, pack rows 4",
    "f16x3 rows, pack rows 2", "f16x3 rows, pack rows 1", "f16x3 rows, GELU pair",
    "f16x3 rows shape, dact_in: the tiles", "f16x3 rows shape, another activation: the tiles",
]


def _case_id(c):
    tags = "".join("_" + t for t in sorted(c.opt - FORMER))
    return f"{c.family}_{c.M}x{c.N}x{c.K}_{'-'.join(c.plan)}{tags}"


def _epilogue(c):
    return "dact" if "dact" in c.opt else "act_gelu" if "gelu" in c.opt else "act" if "swish" in c.opt else "none"


def _plan(c, layout):
    unaligned = tuple(name for name in ("a", "bias") if "offset_" + name in c.opt)
    return ops.gemm_plan(c.family, c.M, c.N, c.K, *LAYOUTS[layout], unaligned=unaligned, epilogue=_epilogue(c))


def _want(c, layout):
    """The fields a case's spec string pins."""
    part = c.plan[layout].split("/")
    if c.family == "f32":
        return dict(route=part[0], reduce=part[1] if len(part) > 1 else "none")
    if part[0] == "refused":
        return dict(route="refused")
    if part[0] == "rows":
        return dict(route="rows", pack_rows=int(part[1][1:]), epilogue="act_gelu" if "gelu" in part else "none",
                    slices=-(-c.N // 128))
    fold = part[2] if len(part) > 2 else "s0v0"
    return dict(route="tile", wide=int(part[1] == "wide"), fold_s=int(fold[1:fold.index("v")]),
                fold_v=int(fold[fold.index("v") + 1:]))


def _mismatch(c):
    bad = []
    for layout in c.plan:
        plan = _plan(c, layout)
        for key, v in _want(c, layout).items():
            if getattr(plan, key) != v:
                bad.append(f"{layout}: {key} {getattr(plan, key)} != {v}")
        if plan.route != "rows" and (plan.splits > 1) != (plan.workspace > 0):
            bad.append(f"{layout}: {plan.splits} splits with {plan.workspace} floats of workspace")
    return bad


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_plan_of_case(case):
    bad = _mismatch(case)
    assert not bad, (f"branch '{case.branch}' lost its case {_case_id(case)}: {bad}; the planner now gives "
                     f"{[_plan(case, l) for l in case.plan]}. Update the case table so the branch keeps a case.")


def test_table_covers_every_branch():
    have = [c.branch for c in CASES]
    assert len(set(have)) == len(have), "a branch has two cases: give each its own tag"
    missing = [b for b in BRANCHES if b not in have]
    assert not missing, f"no case for: {missing}"
    assert not set(have) - set(BRANCHES), f"not in BRANCHES: {sorted(set(have) - set(BRANCHES))}"
    assert len(CASES) <= 80
    ids = [_case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids), "two cases share an id (and with it their inputs)"


def test_table_selects_every_kernel_it_promises():
    """Counted on the plans themselves: every fp32 route (the tile routes in all three layouts with no,
    a flat and a tree reduction; rows_small with both b_kc), every f16x3 tile instance (four layouts x
    wide, the narrow epilogue in all four), every fold (widths 4 and 1 x 1, 4, 16 thread groups), every
    pack-row count of both weight layouts, and both rows epilogues."""
    f32, tile, fold, pack, rows_epi = set(), set(), set(), set(), set()
    for c in CASES:
        for layout in c.plan:
            p = _plan(c, layout)
            if c.family == "f32":
                f32.add((p.route, layout, p.reduce))
            elif p.route == "tile":
                tile.add((layout, p.wide))
                fold.add((p.fold_v, p.fold_s))
            elif p.route == "rows":
                pack.add((layout, p.pack_rows))
                rows_epi.add(p.epilogue)
    for route in ("tile_skinny", "tile_square"):
        for layout in ("nt", "nn", "tn"):
            assert {(route, layout, r) for r in ("none", "flat", "tree")} <= f32, (route, layout)
    assert {("rows_small", "nt", "none"), ("rows_small", "nn", "none"), ("tall_lds", "tn", "tree"),
            ("tall_small", "tn", "tree")} <= f32
    assert tile == {(layout, wide) for layout in LAYOUTS for wide in (0, 1)}
    assert fold == {(0, 0)} | {(v, s) for v in (4, 1) for s in (1, 4, 16)}
    assert pack == {("nt", r) for r in (8, 4, 2, 1)} | {("nn", r) for r in (32, 16, 8, 4, 2, 1)}
    assert rows_epi == {"none", "act_gelu"}
    refused = {c.branch for c in CASES if c.family == "f16x3" and all(v == "refused" for v in c.plan.values())}
    assert len(refused) == 2 and any(c.plan.get("tn") == "refused" and c.plan.get("nt") != "refused"
                                     for c in CASES if c.family == "f16x3")


def test_rows_tile_limit_is_read_off_the_query():
    """The streaming kernel wants a (256-row tile, 128-column slice) pair per CU; the CU count is the
    query's. The table's limit case is the first M with enough tiles at 12 slices, its neighbour the
    last M of the row tile before."""
    cu = ops.gemm_plan("f16x3", 5377, 1536, 32).cu
    row_tiles = -(-cu // 12)
    first = (row_tiles - 1) * 256 + 1
    assert ops.gemm_plan("f16x3", first, 1536, 32).route == "rows"
    assert ops.gemm_plan("f16x3", first - 1, 1536, 32).route == "tile"
    at = {(c.M, c.plan.get("nt", "").split("/")[0]) for c in CASES
          if c.family == "f16x3" and (c.N, c.K) == (1536, 32) and not c.opt}
    assert {(first, "rows"), (first - 1, "tile")} <= at, (cu, first, at)
    p = ops.gemm_plan("f16x3", first, 1536, 32)
    assert p.blocks * p.tiles_per_block >= row_tiles * 12 > (p.blocks - 1) * p.tiles_per_block
    assert p.blocks <= cu


def test_fold_limits_are_read_off_the_query():
    """On one 128 x 128 tile: the first K at which the fold takes 4 and 16 thread groups, and the K
    before each, have a case."""
    first = {}
    for K in range(4, 8193, 4):
        first.setdefault(ops.gemm_plan("f16x3", 128, 128, K).fold_s, K)
    assert sorted(first) == [0, 1, 4, 16]
    have = {(c.K, _want(c, "nt")["fold_s"]) for c in CASES
            if c.family == "f16x3" and (c.M, c.N) == (128, 128) and "nt" in c.plan and not c.opt}
    for S in (4, 16):
        below = ops.gemm_plan("f16x3", 128, 128, first[S] - 4).fold_s
        assert {(first[S], S), (first[S] - 4, below)} <= have, (S, first[S], have)
    for K, S in ((512, 1), (2048, 4), (8192, 16)):
        assert ops.gemm_plan("f16x3", 128, 128, K).fold_s == S


def test_pack_row_limits_are_read_off_the_query():
    """Each K (a multiple of 32) at which the pack kernel's rows per block halve has a rows case."""
    for layout in ("nt", "nn"):
        halvings, last = [], None
        for K in range(32, 8193, 32):
            N = min(1536, (4 << 20) // K // 128 * 128)
            p = ops.gemm_plan("f16x3", 1 << 20, N, K, *LAYOUTS[layout])
            assert p.route == "rows"
            if last is not None and p.pack_rows != last:
                halvings.append((K, p.pack_rows))
            last = p.pack_rows
        have = {(c.K, _want(c, layout)["pack_rows"]) for c in CASES
                if c.family == "f16x3" and c.plan.get(layout, "").startswith("rows")}
        assert halvings and set(halvings) <= have, (layout, halvings, have)


def test_f32_limits_are_read_off_the_query():
    """rows_small starts at the table's M and ends at the table's N K; the tall kernels start at the
    table's K."""
    P = ops.gemm_plan
    m = next(M for M in range(65000, 66000) if P("f32", M, 2, 2).route == "rows_small")
    nk = max(n * 64 for n in range(1, 65) if P("f32", m, n, 64).route == "rows_small")
    k = next(K for K in range(16000, 17000, 1) if P("f32", 2, 4, K, False, False).route != "tile_skinny")
    have = {(c.M, c.N, c.K): c.plan for c in CASES if c.family == "f32" and not c.opt}
    assert have[(m, 2, 2)]["nt"] == "rows_small" and have[(m - 1, 2, 2)]["nt"] == "tile_square"
    assert nk == 512 and have[(m, 8, 64)]["nt"] == "rows_small"
    assert have[(2, 4, k)]["tn"] == "tall_lds/tree" and have[(2, 4, k - 1)]["tn"] == "tile_skinny/tree"


def test_shape_only_workspace_queries_cover_every_plan():
    h = _lib.lib()
    for c in CASES:
        query = (h.adell_gemm_f32_workspace_floats if c.family == "f32"
                 else h.adell_gemm_f16x3_workspace_floats)(c.M, c.N, c.K)
        for layout in c.plan:
            assert query >= _plan(c, layout).workspace, (c.branch, layout)


def test_norows_switch_sends_every_rows_case_to_the_tiles():
    rows = [(c, l) for c in CASES for l in c.plan if c.family == "f16x3" and c.plan[l].startswith("rows")]
    assert len(rows) >= 10
    for c, layout in rows:
        assert _plan(c, layout).route == "rows"
        with _lib.tuning(gemm_norows=1):
            p = _plan(c, layout)
            assert p.route == "tile" and p.wide, (c.branch, layout, p)
    assert _plan(*rows[0]).route == "rows"


def test_f16x3_ok_is_policy_on_top_of_the_plans(monkeypatch):
    t = torch.zeros(8)
    ok = lambda M, N, K, a_kc=True, A=t: ops.gemm_f16x3_ok(M, N, K, A, K if a_kc else M, a_kc, t, K, True)
    monkeypatch.setitem(ops.FLAGS, "gemm_f16x3", True)
    monkeypatch.setitem(ops.FLAGS, "gemm_f16x3_min_k", 0)
    monkeypatch.setitem(ops.FLAGS, "gemm_f16x3_min_mn", 64)
    assert ok(120, 384, 96) and not ok(120, 48, 96)           # the size rule
    assert ok(524288, 32, 128) and not ok(524288, 24, 128)     # the streaming regime below it
    assert not ok(120, 384, 98) and not ok(102, 384, 96, a_kc=False)      # refused by the f16x3 plan
    assert not ok(120, 384, 96, A=t[1:])
    monkeypatch.setitem(ops.FLAGS, "gemm_f16x3_min_mn", 0)
    assert ok(120, 48, 96) and not ok(65536, 8, 64) and ok(65535, 8, 64)  # rows_small stays on fp32
    monkeypatch.setitem(ops.FLAGS, "gemm_f16x3_min_k", 128)
    assert not ok(120, 384, 96)
    monkeypatch.setitem(ops.FLAGS, "gemm_f16x3", False)
    assert not ok(120, 384, 512)


# ---- GPU: every case in every layout it lists against fp64 on the CPU -------------------------------

F16_BAR = 2e-6
SAMPLED_ABOVE = 1 << 24        # A operands above 64 MB: drawn on the device, reference on four row tiles


def _dev(t, cuda, offset=False):
    """`t` as an fp32 device tensor; `offset`: contiguous, but one element (4 bytes) into a 16-byte
    aligned storage, as a view that starts inside a larger buffer is."""
    t = t.float()
    if not offset:
        return t.to(cuda)
    buf = torch.zeros(t.numel() + 1, device=cuda, dtype=torch.float32)
    view = buf[1:].view(t.shape)
    view.copy_(t.to(cuda))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _operands(A, B, layout, cuda, c):
    """Device operands of a layout from A [M, K] and B [K, N], with their leading dimensions."""
    a_kc, b_kc = LAYOUTS[layout]
    Ad = _dev((A if a_kc else A.t()).contiguous(), cuda, "offset_a" in c.opt)
    Bd = _dev((B.t() if b_kc else B).contiguous(), cuda)
    return Ad, (c.K if a_kc else c.M), a_kc, Bd, (c.K if b_kc else c.N), b_kc


def run_f32_case(c, cuda):
    """{layout: output} and the fp64 reference of an fp32 case (inputs: those of the former
    test_gemm_layouts_match_float64 always drew)."""
    rng = np.random.default_rng(c.M * 131 + c.N * 17 + c.K)
    a = rng.standard_normal((c.M, c.K)).astype(np.float32)
    b = rng.standard_normal((c.K, c.N)).astype(np.float32)
    ref = a.astype(np.float64) @ b.astype(np.float64)
    A, B = torch.from_numpy(a), torch.from_numpy(b)
    return {layout: ops.gemm(c.M, c.N, c.K, *_operands(A, B, layout, cuda, c)) for layout in c.plan}, ref


def f16_inputs(c, cuda):
    """A [M, K], B [K, N], bias, residual (and the saved pre-activation of a dact case): those of the
    former test_layouts_against_fp64; the large rows cases on the device."""
    if c.M * c.K > SAMPLED_ABOVE:
        g = torch.Generator(device=cuda).manual_seed(c.M + c.N + c.K)
        return [torch.randn(*s, generator=g, device=cuda) for s in ((c.M, c.K), (c.K, c.N), (c.N,), (c.M, c.N))]
    g = torch.Generator().manual_seed(c.M + c.N + c.K)
    t = [torch.randn(*s, generator=g) for s in ((c.M, c.K), (c.K, c.N), (c.N,), (c.M, c.N))]
    if "dact" in c.opt:
        t.append(torch.randn(c.M, c.N, generator=g))
    return t


def run_f16_layout(c, layout, cuda, t, words=False):
    """(C, act(C) or None) of one layout of an f16x3 case; raises what the library raises."""
    A, B, bias, res = t[:4]
    Ad, lda, a_kc, Bd, ldb, b_kc = _operands(A, B, layout, cuda, c)
    bd, rd = _dev(bias, cuda, "offset_bias" in c.opt), res.to(cuda)
    epi = _epilogue(c)
    if epi == "none":
        wa, wb = (ops.absmax_word(Ad), ops.absmax_word(Bd)) if words else (None, None)
        return ops.gemm_f16x3(c.M, c.N, c.K, Ad, lda, a_kc, Bd, ldb, b_kc, wa, wb, bias=bd, residual=rd), None
    act = "swish" if epi == "act" else "gelu"
    return ops.gemm_f16x3_act(c.M, c.N, c.K, Ad, lda, a_kc, Bd, ldb, b_kc, act, bias=bd, residual=rd,
                              want_act=epi != "dact", dact_in=t[4].to(cuda) if epi == "dact" else None)


def _f16_reference(c, t):
    """fp64 (rows, C, act(C) or None, sum |a||b|): all rows, or four whole row tiles of a sampled case."""
    A, B, bias, res = t[:4]
    rows = torch.arange(c.M)
    if c.M * c.K > SAMPLED_ABOVE:
        tiles = -(-c.M // 256)
        rows = torch.cat([torch.arange(256 * i, min(256 * i + 256, c.M)) for i in (0, tiles // 2, tiles - 2, tiles - 1)])
    a64, b64 = A[rows.to(A.device)].cpu().double(), B.cpu().double()
    want = a64 @ b64 + bias.cpu().double() + res[rows.to(res.device)].cpu().double()
    scale = float((a64.abs() @ b64.abs()).max())
    post = None
    if "dact" in c.opt:
        z = t[4].double().requires_grad_(True)
        torch.nn.functional.gelu(z).sum().backward()
        want = want * z.grad
    elif _epilogue(c) != "none":
        post = (torch.nn.functional.silu if "swish" in c.opt else torch.nn.functional.gelu)(want)
    return rows, want, post, scale


def case_of(family, M, N, K):
    """The table's row of a shape (the one without an operand offset or an epilogue)."""
    hit = [c for c in CASES if (c.family, c.M, c.N, c.K) == (family, M, N, K) and not c.opt - FORMER]
    assert len(hit) == 1, f"the case table has {len(hit)} plain rows for {family} {M}x{N}x{K}"
    return hit[0]


def check_f32_case(c, cuda, layouts=None):
    """Run the case's layouts (or the ones given) and hold them to the fp32 family's bar."""
    c = c._replace(plan={l: c.plan[l] for l in layouts or c.plan})
    assert not _mismatch(c)
    outs, ref = run_f32_case(c, cuda)
    tol = 2e-6 * max(1.0, np.sqrt(c.K) / 8)
    errs = {l: float(np.abs(o.cpu().numpy() - ref).max() / (np.abs(ref).max() + 1e-30)) for l, o in outs.items()}
    print(_case_id(c), {l: f"{c.plan[l]} {e:.2e}" for l, e in errs.items()}, f"bar {tol:.2e}")
    bad = {l: e for l, e in errs.items() if not e < tol}
    assert not bad, f"'{c.branch}' {_case_id(c)}: relative error above {tol:.2e}: {bad}"


def check_f16x3_case(c, cuda, layouts=None, words=(False,)):
    """Run the case's layouts (or the ones given), each with the absmax-word settings given, and hold
    them to the f16x3 family's bar; a refused layout asserts the refusal."""
    c = c._replace(plan={l: c.plan[l] for l in layouts or c.plan})
    assert not _mismatch(c)
    t = f16_inputs(c, cuda)
    ref = None
    errs = {}
    for layout, spec in c.plan.items():
        if spec == "refused":
            Ad, lda, a_kc, Bd, ldb, b_kc = _operands(t[0], t[1], layout, cuda, c)
            with mock.patch.dict(ops.FLAGS, gemm_f16x3=True, gemm_f16x3_min_mn=0, gemm_f16x3_min_k=0):
                assert not ops.gemm_f16x3_ok(c.M, c.N, c.K, Ad, lda, a_kc, Bd, ldb, b_kc)   # not by policy
            with pytest.raises(_lib.AdellHipError, match="unsupported"):
                run_f16_layout(c, layout, cuda, t)
            continue
        ref = ref or _f16_reference(c, t)
        rows, want, post, scale = ref
        for w in words:
            pre, act = run_f16_layout(c, layout, cuda, t, w)
            key = layout + ("+words" if w else "")
            errs[key] = float((pre[rows.to(cuda)].cpu().double() - want).abs().max() / scale)
            if post is not None:
                errs[key + " act"] = float((act[rows.to(cuda)].cpu().double() - post).abs().max() / scale)
    print(_case_id(c), {k: f"{e:.2e}" for k, e in errs.items()})
    bad = {k: e for k, e in errs.items() if not e < F16_BAR}
    assert not bad, f"'{c.branch}' {_case_id(c)}: error over sum |a||b| above {F16_BAR}: {bad}"


# The rows marked "former" run, one layout at a time, under the test ids they have always had:
# test_gemm_gpu.py::test_gemm_layouts_match_float64 and test_gemm_f16x3_gpu.py::test_layouts_against_fp64
# take their row from this table (case_of) and call the two functions above.
@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.family == "f32" and "former" not in c.opt], ids=_case_id)
def test_f32_case_matches_fp64(cuda, case):
    check_f32_case(case, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.family == "f16x3" and "former" not in c.opt],
                         ids=_case_id)
def test_f16x3_case_matches_fp64(cuda, case):
    check_f16x3_case(case, cuda)
