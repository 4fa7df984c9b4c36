"""Every launch plan of the f16x3 implicit-GEMM convolution (csrc/conv3d.hip adell_plan_f16) and of
the z-ring weight gradient, from one case table:

- on the build host (no GPU), each case still gets the plan it is in the table for
  (ops.conv3d_plan / ops.convtranspose3d_plan / ops.conv3d_bwd_weight_plan), and every branch of the
  planner has at least one case. A retune that moves a shape onto another branch fails here, naming
  the branch, so the table is updated on purpose instead of the branch losing its coverage (such a
  retune also regenerates the dense record of tests/test_conv_plan_sweep.py: tools/conv_plan_sweep.py);
- on the GPU, each case runs through functional.conv3d / conv_transpose3d (forward with its
  statistics partials, backward-data for both concat sources, dW, db) against torch's fp64
  convolution on the CPU; split-K launches must also be bit-identical across two calls (the fold
  order is fixed).

Shapes are the smallest that select their branch, batch 1 where the branch allows it; each case has a
neighbour just across the threshold that selects it. (D, H, W) order throughout."""
import collections
import ctypes
import os
import re
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from adell_mri_amd import _lib, ops
from adell_mri_amd._lib import AdellHipError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# direction: "fwd" / "bwd" (adell_conv3d_f16x3_plan, backward_data = 0 / 1), "convt" (transposed-conv
# forward: c0 = Cin, cout = Cs, k = the factors), "wgrad" (ops.conv3d_bwd_weight_plan). cfg: the plan's
# config, None = refused; for "wgrad" the route: "small" (<= 4 input channels), "zring" (32 x 32
# tiles), "zring:1seg" / "zring:segs" (one / several z segments), "zring:t16" (16 x 16 tiles), "s2"
# (the stride-2 sub-lattice kernel), "plane" (the per-plane kernel, any instance) or
# "plane:MAXJ,PFX,PFY" (that instance of it). split: the K shares > 1 (True / False), or the exact
# share count.
Case = collections.namedtuple("Case", "branch direction N size c0 c1 cout k s p cfg split")

CASES = [
    # 1. 16 -> 16, 3^3 stride 1, Wo, Ho >= 8, Do >= 4: the z-marching 16-column kernel (cfg 8)
    Case("zring16", "fwd", 1, (4, 8, 8), 16, 0, 16, 3, 1, 1, 8, False),
    Case("zring16", "bwd", 1, (4, 8, 8), 16, 0, 16, 3, 1, 1, 8, False),
    Case("zring16 neighbour: Do = 3", "fwd", 1, (3, 8, 8), 16, 0, 16, 3, 1, 1, 3, False),
    Case("zring16 neighbour: C1 > 0", "fwd", 1, (4, 8, 8), 16, 16, 16, 3, 1, 1, 3, False),
    # 2. kernel == stride > 1 (the transposed conv's backward-data): two-wave 64 x 32 bricks for <= 32
    # outputs, 64 x 64 above -- at sizes where the heuristic alone would take 256-voxel bricks
    Case("kernel == stride, Cout <= 32", "fwd", 1, (64, 64, 128), 32, 0, 32, 2, 2, 0, 6, False),
    Case("kernel == stride, Cout > 32", "fwd", 2, (64, 64, 64), 32, 0, 48, 2, 2, 0, 2, False),
    # 3. strided k > s with <= 32 outputs: two-wave bricks (the heuristic would take cfg 3)
    Case("strided k > s, Cout <= 32", "fwd", 1, (9, 9, 9), 16, 0, 32, 3, (2, 2, 1), 1, 6, False),
    Case("strided k > s, Cout <= 32", "fwd", 1, (10, 10, 10), 24, 0, 24, 3, 2, 1, 6, False),
    Case("strided k > s neighbour: Cout > 32", "fwd", 1, (9, 9, 9), 16, 0, 48, 3, (2, 2, 1), 1, 2,
         False),
    # 4. 5^3 stride 1 on >= 65 536 output voxels: 128-voxel x 32-column bricks; exactly at the threshold
    # and one row below it (where the heuristic gives 64 x 64 bricks)
    Case("5^3 stride 1, >= 65536 voxels", "fwd", 1, (32, 32, 64), 64, 0, 64, 5, 1, 2, 3, False),
    Case("5^3 stride 1, >= 65536 voxels", "bwd", 1, (32, 32, 64), 64, 0, 64, 5, 1, 2, 3, False),
    Case("5^3 neighbour: < 65536 voxels", "fwd", 1, (32, 31, 64), 64, 0, 64, 5, 1, 2, 2, False),
    # 5. 3^3 stride 1, <= 32 outputs on [4 096, 262 144) voxels: retiled 256-voxel bricks, not cfg 4
    Case("3^3 Cout <= 32, 4k-256k voxels", "fwd", 1, (16, 16, 16), 32, 0, 32, 3, 1, 1, 1, False),
    Case("3^3 Cout <= 32, 4k-256k voxels", "fwd", 1, (16, 16, 16), 24, 0, 24, 3, 1, 1, 1, False),
    Case("3^3 Cout <= 32 neighbour: < 4096 voxels", "fwd", 1, (15, 16, 16), 32, 0, 32, 3, 1, 1, 3,
         False),
    # 6. 3^3 stride 1, > 32 outputs on < 4 096 voxels
    Case("3^3 wide < 4096 voxels, Cin >= 512, >= 2048 voxels", "fwd", 1, (9, 9, 26), 512, 0, 512, 3,
         1, 1, 0, True),
    Case("3^3 wide < 4096 voxels neighbour: < 2048 voxels", "fwd", 1, (8, 8, 31), 512, 0, 64, 3, 1,
         1, 2, True),
    Case("3^3 wide < 4096 voxels, >= 512 voxels", "fwd", 2, (8, 8, 8), 256, 0, 256, 3, 1, 1, 2, True),
    Case("3^3 wide < 4096 voxels, < 512 voxels", "fwd", 1, (7, 7, 7), 64, 0, 64, 3, 1, 1, 6, True),
    Case("3^3 wide < 4096 voxels, < 512 voxels", "fwd", 1, (7, 8, 8), 64, 0, 48, 3, 1, 1, 6, False),
    Case("3^3 wide < 512 voxels neighbour: 512 voxels", "fwd", 1, (8, 8, 8), 96, 0, 96, 3, 1, 1, 2,
         False),
    # 7. 3^3 stride 1 on [4 096, 32 768) voxels: 512 outputs take 64-column bricks, the rest 32-column
    # ones + split-K
    Case("3^3 4k-32k voxels, Cout >= 512", "fwd", 1, (16, 16, 16), 256, 0, 512, 3, 1, 1, 0, True),
    Case("3^3 4k-32k voxels neighbour: Cout < 512", "fwd", 1, (16, 16, 16), 64, 0, 496, 3, 1, 1, 1,
         False),
    Case("3^3 4k-32k voxels, split-K", "fwd", 2, (16, 16, 16), 128, 0, 128, 3, 1, 1, 1, True),
    # 8. 3^3 stride 1 on [32 768, 262 144) voxels with <= 64 outputs: retiled 256-voxel bricks
    Case("3^3 32k-256k voxels, Cout <= 64", "fwd", 1, (32, 32, 32), 64, 0, 64, 3, 1, 1, 1, True),
    Case("3^3 32k-256k voxels, Cout <= 64", "fwd", 1, (32, 32, 32), 48, 0, 48, 3, 1, 1, 1, False),
    Case("3^3 32k-256k voxels neighbour: Cout > 64", "fwd", 1, (32, 32, 32), 64, 0, 80, 3, 1, 1, 0,
         False),
    # 9. the heuristic's 256-voxel x 32-column brick becomes the 8 x 8 x 8 SPEC instance (cfg 4) when
    # both sources are whole 16-channel chunks
    Case("SPEC 8x8x8 (cfg 4)", "fwd", 2, (32, 64, 64), 32, 0, 32, 3, 1, 1, 4, False),
    Case("SPEC 8x8x8 (cfg 4)", "bwd", 2, (32, 64, 64), 24, 0, 32, 3, 1, 1, 4, False),
    Case("SPEC 8x8x8 neighbour: C0 % 16 != 0", "fwd", 2, (32, 64, 64), 24, 0, 32, 3, 1, 1, 1,
         False),
    # 10. split-K at its edges
    Case("split-K, Cin % 16 != 0", "fwd", 1, (8, 8, 8), 72, 0, 64, 3, 1, 1, 2, 5),
    Case("split-K, short last share", "fwd", 1, (16, 32, 32), 80, 0, 64, 3, 1, 1, 1, 3),
    Case("split-K, short last share", "fwd", 1, (16, 32, 32), 72, 0, 64, 3, 1, 1, 1, 3),
    Case("split-K refused: 256 % (Cout / 4) != 0", "fwd", 1, (8, 8, 8), 96, 0, 96, 3, 1, 1, 2,
         False),
    Case("split-K, backward-data with concat sources", "bwd", 1, (8, 8, 8), 32, 32, 128, 3, 1, 1, 2,
         True),
    Case("split-K, backward-data with concat sources", "bwd", 1, (8, 8, 8), 48, 16, 128, 3, 1, 1, 2,
         True),
    # 11. transposed-conv forward, pixel-shuffle store with F * Cs >= 128 columns: 256-column tiles.
    # Cin 40 / 48: not the streaming k = 2 kernels (csrc/convt_k2.hip, 32 / 64 input channels)
    Case("convT 256-column tile", "convt", 1, (4, 4, 4), 48, 0, 32, (2, 2, 2), None, None, 5, False),
    Case("convT 256-column tile, ragged", "convt", 1, (3, 4, 4), 40, 0, 20, (2, 2, 2), None, None, 5,
         False),
    Case("convT 256-column tile, ragged", "convt", 1, (4, 4, 4), 48, 0, 48, (2, 2, 2), None, None, 5,
         False),
    Case("convT 256-column tile", "convt", 1, (4, 4, 4), 48, 0, 32, (2, 2, 1), None, None, 5, False),
    Case("convT neighbour: F * Cs < 128", "convt", 1, (4, 4, 4), 48, 0, 31, (2, 2, 1), None, None, 2,
         False),
    # 12. the LDS fallback at the bottom of adell_plan_f16 (every step it takes: FALLBACK_PATHS), and a
    # conv whose halo does not fit even the smallest brick. The 64 x 64 -> 64 x 32 step and the third
    # pass were missing: those layers were refused. No kernel takes the last one: the library refuses
    # and functional.conv3d raises (there is no eager fallback)
    Case("LDS fallback, 256 x 64 -> 64 x 64", "fwd", 1, (64, 64, 64), 16, 0, 80, 5, 2, 2, 2, False),
    Case("LDS fallback, 64 x 64 -> 64 x 32", "fwd", 1, (33, 33, 33), 32, 0, 64, 7, 2, 3, 6, False),
    Case("LDS fallback, 256 x 64 -> 64 x 64 -> 64 x 32", "fwd", 1, (63, 63, 63), 16, 0, 80, 7, 2, 3,
         6, False),
    Case("LDS fallback, 128 x 32 -> 64 x 32", "fwd", 1, (2, 2, 8192), 16, 0, 32, 7, 1, 3, 6, False),
    Case("LDS fallback, 256 x 32 -> 128 x 32 -> 64 x 32", "fwd", 1, (2, 2, 16384), 16, 0, 32, 7, 1,
         3, 6, False),
    Case("LDS fallback neighbour: 32 outputs, no fallback", "fwd", 1, (33, 33, 33), 32, 0, 32, 7, 2,
         3, 6, False),
    Case("refused", "fwd", 1, (20, 20, 20), 16, 0, 48, 7, 3, 3, None, False),
    # 13. weight packing (conv_igemm_f16.h): a GEMM column of taps x K floats is staged in LDS up to
    # kPackLds; K = Cin forward, Cout backward-data
    Case("pack staged / not", "fwd", 1, (4, 4, 4), 512, 0, 544, 3, 1, 1, 6, False),
    Case("pack staged / not", "bwd", 1, (4, 4, 4), 512, 0, 544, 3, 1, 1, 6, True),
    Case("pack staged / not", "fwd", 1, (4, 4, 4), 544, 0, 512, 3, 1, 1, 6, True),
    Case("pack staged / not", "fwd", 1, (8, 8, 8), 112, 0, 128, 5, 1, 2, 2, True),
    Case("pack staged / not", "fwd", 1, (8, 8, 8), 128, 0, 112, 5, 1, 2, 2, False),
    # weight gradient (adell_wgrad_zring_plan)
    Case("wgrad z-ring, one segment", "wgrad", 1, (6, 8, 8), 32, 0, 32, 3, 1, 1, "zring:1seg", False),
    Case("wgrad z-ring, several segments", "wgrad", 1, (16, 16, 16), 32, 0, 32, 3, 1, 1,
         "zring:segs", False),
    Case("wgrad z-ring, 16 x 16 tiles", "wgrad", 1, (16, 16, 16), 16, 0, 48, 3, 1, 1, "zring:t16",
         False),
    Case("wgrad z-ring, 16 x 16 tiles", "wgrad", 1, (4, 8, 8), 16, 0, 16, 3, 1, 1, "zring:t16", False),
    Case("wgrad z-ring, ragged column tiles", "wgrad", 1, (8, 12, 12), 32, 0, 32, 3, 1, 1, "zring",
         False),
    Case("wgrad z-ring, C1 > 0", "wgrad", 1, (8, 8, 12), 32, 16, 32, 3, 1, 1, "zring", False),
    Case("wgrad z-ring, C1 > 0", "wgrad", 1, (16, 16, 16), 48, 16, 32, 3, 1, 1, "zring", False),
    Case("wgrad per-plane: 5^3", "wgrad", 1, (32, 32, 64), 64, 0, 64, 5, 1, 2, "plane", False),
    Case("wgrad per-plane: Do < 4", "wgrad", 1, (3, 8, 8), 16, 0, 16, 3, 1, 1, "plane", False),
    # the eight instances <MAXJ, PFX, PFY> of the per-plane kernel (csrc/conv_wgrad_f16.hip
    # kWgradF16Instances), each with a neighbour just across the threshold that selects it
    Case("wgrad plane <2>", "wgrad", 1, (4, 8, 8), 32, 0, 32, 1, 1, 0, "plane:2,0,0", False),
    Case("wgrad plane <2> neighbour: 9 taps per plane", "wgrad", 1, (3, 4, 8), 32, 0, 32, 3, 1, 1,
         "plane:3,0,0", False),
    Case("wgrad plane <3>", "wgrad", 1, (4, 4, 8), 32, 0, 32, 3, 1, 1, "plane:3,0,0", False),
    Case("wgrad plane <3> neighbour: plane height 5, k-split", "wgrad", 1, (4, 5, 8), 32, 0, 32, 3, 1,
         1, "plane:5,4,2", False),
    Case("wgrad plane <5,4,2>", "wgrad", 1, (3, 8, 8), 32, 0, 32, 3, 1, 1, "plane:5,4,2", False),
    Case("wgrad plane <5,4,2> neighbour: Cin > 32", "wgrad", 1, (3, 8, 8), 48, 0, 32, 3, 1, 1,
         "plane:5,7,2", False),
    Case("wgrad plane <5,7,2>", "wgrad", 1, (3, 8, 8), 64, 0, 32, 3, 1, 1, "plane:5,7,2", False),
    Case("wgrad plane <5,7,2> neighbour: Cout > 32", "wgrad", 1, (3, 8, 8), 64, 0, 48, 3, 1, 1,
         "plane:9,0,0", False),
    Case("wgrad plane <5,4,4>", "wgrad", 1, (3, 8, 8), 32, 0, 64, 3, 1, 1, "plane:5,4,4", False),
    Case("wgrad plane <5,4,4> neighbour: plane height 4, dY brick in two loads", "wgrad", 1,
         (3, 4, 8), 32, 0, 64, 3, 1, 1, "plane:5,7,2", False),
    Case("wgrad plane <9>", "wgrad", 1, (3, 8, 8), 64, 0, 64, 3, 1, 1, "plane:9,0,0", False),
    Case("wgrad plane <9> neighbour: 5^3, one ky row per block", "wgrad", 1, (8, 8, 8), 64, 0, 64, 5,
         1, 2, "plane:5,0,0", False),
    Case("wgrad plane <7>", "wgrad", 1, (8, 8, 8), 32, 0, 32, 5, 1, 2, "plane:7,0,0", False),
    Case("wgrad plane <7> neighbour: Cin > 32", "wgrad", 1, (8, 8, 8), 64, 0, 32, 5, 1, 2,
         "plane:9,0,0", False),
    Case("wgrad plane <5>", "wgrad", 1, (10, 10, 10), 48, 0, 32, 3, 2, 1, "plane:5,0,0", False),
    Case("wgrad plane <5> neighbour: Cout > 32", "wgrad", 1, (10, 10, 10), 48, 0, 64, 3, 2, 1,
         "plane:9,0,0", False),
    # plan only (PLAN_ONLY): these routes have their own GPU tests (tests/test_ops_gpu.py,
    # tests/test_wgrad_s2_gpu.py)
    Case("wgrad small-channel route", "wgrad", 1, (8, 8, 8), 4, 0, 16, 3, 1, 1, "small", False),
    Case("wgrad small-channel neighbour: 5 channels", "wgrad", 1, (8, 8, 8), 5, 0, 16, 3, 1, 1,
         "plane:5,4,2", False),
    Case("wgrad stride-2 route", "wgrad", 2, (64, 128, 128), 32, 0, 32, 3, 2, 1, "s2", False),
    Case("wgrad stride-2 neighbour: < 8 bricks per CU", "wgrad", 2, (64, 64, 64), 32, 0, 32, 3, 2, 1,
         "plane:3,0,0", False),
]

# cases checked on the build host only
PLAN_ONLY = {"wgrad small-channel route", "wgrad small-channel neighbour: 5 channels",
             "wgrad stride-2 route", "wgrad stride-2 neighbour: < 8 bricks per CU"}

# branches the table must cover (each needs at least one case)
BRANCHES = {
    "zring16", "kernel == stride, Cout <= 32", "kernel == stride, Cout > 32",
    "strided k > s, Cout <= 32", "5^3 stride 1, >= 65536 voxels", "3^3 Cout <= 32, 4k-256k voxels",
    "3^3 wide < 4096 voxels, Cin >= 512, >= 2048 voxels", "3^3 wide < 4096 voxels, >= 512 voxels",
    "3^3 wide < 4096 voxels, < 512 voxels", "3^3 4k-32k voxels, Cout >= 512",
    "3^3 4k-32k voxels, split-K", "3^3 32k-256k voxels, Cout <= 64", "SPEC 8x8x8 (cfg 4)",
    "split-K, Cin % 16 != 0", "split-K, short last share", "split-K refused: 256 % (Cout / 4) != 0",
    "split-K, backward-data with concat sources", "convT 256-column tile",
    "convT 256-column tile, ragged", "LDS fallback, 256 x 64 -> 64 x 64",
    "LDS fallback, 64 x 64 -> 64 x 32", "LDS fallback, 256 x 64 -> 64 x 64 -> 64 x 32",
    "LDS fallback, 128 x 32 -> 64 x 32", "LDS fallback, 256 x 32 -> 128 x 32 -> 64 x 32", "refused",
    "pack staged / not", "wgrad z-ring, one segment", "wgrad z-ring, several segments",
    "wgrad z-ring, 16 x 16 tiles", "wgrad z-ring, ragged column tiles", "wgrad z-ring, C1 > 0",
    "wgrad per-plane: 5^3", "wgrad plane <2>", "wgrad plane <3>", "wgrad plane <5,4,2>",
    "wgrad plane <5,7,2>", "wgrad plane <5,4,4>", "wgrad plane <5>", "wgrad plane <7>",
    "wgrad plane <9>", "wgrad small-channel route", "wgrad stride-2 route",
}


# configs each LDS-fallback case passes through (the first is the size heuristic's pick, the last the
# plan)
FALLBACK_PATHS = {
    "LDS fallback, 256 x 64 -> 64 x 64": (0, 2),
    "LDS fallback, 64 x 64 -> 64 x 32": (2, 6),
    "LDS fallback, 256 x 64 -> 64 x 64 -> 64 x 32": (0, 2, 6),
    "LDS fallback, 128 x 32 -> 64 x 32": (3, 6),
    "LDS fallback, 256 x 32 -> 128 x 32 -> 64 x 32": (1, 3, 6),
}


def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3


def _case_id(c):
    s = "" if c.s is None else "_s" + "".join(str(v) for v in _triple(c.s))
    return "{}_n{}_{}_c{}+{}_o{}_k{}{}".format(c.direction, c.N, "x".join(map(str, c.size)), c.c0,
                                             c.c1, c.cout, "".join(map(str, _triple(c.k))), s)


def _out_size(c):
    return ops.conv_out_size(c.size, _triple(c.k), _triple(c.s), _triple(c.p))


def _plan_of(c):
    """(what the planner does now, as the table's cfg / split values)"""
    if c.direction == "wgrad":
        p = ops.conv3d_bwd_weight_plan(c.N, c.size, c.c0, c.c1, c.cout, c.k, c.s, c.p)
        if p.route == "plane":
            return "plane:{},{},{}".format(*p.instance), False
        if p.route == "zring16":
            return "zring:t16", False
        if p.route == "zring32":
            return ("zring:1seg" if p.zring[2] == 1 else "zring:segs"), False
        return p.route, False
    if c.direction == "convt":
        p = ops.convtranspose3d_plan(c.N, c.size, c.c0, c.cout, c.k)
    else:
        p = ops.conv3d_plan(c.N, c.size, c.c0, c.c1, c.cout, c.k, c.s, c.p,
                            backward_data=c.direction == "bwd")
    if p is None:
        return None, False
    return p.cfg, p.shares


def _matches(c, cfg, shares):
    if c.direction == "wgrad":
        want = c.cfg
        return (cfg == want or (want == "zring" and cfg in ("zring:1seg", "zring:segs"))
                or (want == "plane" and cfg.startswith("plane:")))
    if cfg != c.cfg:
        return False
    if cfg is None:
        return True
    if isinstance(c.split, bool):
        return (shares > 1) == c.split
    return shares == c.split


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_plan_of_case(case):
    cfg, shares = _plan_of(case)
    assert _matches(case, cfg, shares), (
        f"branch '{case.branch}' lost its case {_case_id(case)}: the planner now gives cfg {cfg}"
        f"{'' if isinstance(shares, bool) else f' with {shares} K shares'}, the table expects cfg "
        f"{case.cfg}, split {case.split}. Update the case table so the branch keeps a case.")


def test_table_covers_every_branch():
    missing = BRANCHES - {c.branch for c in CASES}
    assert not missing, f"no case for: {sorted(missing)}"


def test_table_straddles_the_weight_pack_staging_limit():
    """Both sides of kPackLds for both pack modes (forward: K = Cin, backward-data: K = Cout), on 27-
    and on 125-tap layers."""
    src = open(os.path.join(ROOT, "adell_mri_amd", "csrc", "conv_igemm_f16.h")).read()
    limit = int(re.search(r"constexpr int kPackLds = (\d+);", src).group(1))
    seen = set()
    for c in CASES:
        if c.branch != "pack staged / not":
            continue
        taps = int(np.prod(_triple(c.k)))
        for mode, K in ((0, c.c0 + c.c1), (1, c.cout)):
            seen.add((taps, mode, taps * K <= limit))
    want = {(t, m, st) for t in (27, 125) for m in (0, 1) for st in (True, False)}
    assert want <= seen, f"pack staging sides not covered: {sorted(want - seen)}"


def _heuristic_cfg(c):
    """adell_pick_tile's size rule: the config a layer starts on when no branch rule applies."""
    Do, Ho, Wo = _out_size(c)
    vox, wide = c.N * Do * Ho * Wo, c.cout > 32
    big = vox * (-(-c.cout // 64) if wide else 1) >= 256 * 256
    return (0 if wide else 1) if big else (2 if wide else 3)


def test_lds_fallback_takes_every_step():
    """Each fallback case starts where its path says and every config before the last is refused on
    its own (adell_debug_force_conv_cfg plans one config with no fallback): the plan really walks the
    whole path."""
    L = _lib.lib()
    cases = {c.branch: c for c in CASES if c.branch in FALLBACK_PATHS}
    assert set(cases) == set(FALLBACK_PATHS)
    for branch, path in FALLBACK_PATHS.items():
        c = cases[branch]
        assert _heuristic_cfg(c) == path[0], f"'{branch}' starts on cfg {_heuristic_cfg(c)}"
        try:
            for i, cfg in enumerate(path):
                L.adell_debug_force_conv_cfg(cfg)
                p = ops.conv3d_plan(c.N, c.size, c.c0, c.c1, c.cout, c.k, c.s, c.p)
                assert (p is None) == (i < len(path) - 1), (
                    f"'{branch}': cfg {cfg} alone is {'refused' if p is None else 'planned'}")
        finally:
            L.adell_debug_force_conv_cfg(-1)
        assert ops.conv3d_plan(c.N, c.size, c.c0, c.c1, c.cout, c.k, c.s, c.p).cfg == path[-1]


def test_plan_query_agrees_with_the_launch_entry_points():
    """Plumbing: the plan query, adell_conv3d_fwd_ntiles_f16x3(_ws) and adell_conv3d_splitk_workspace
    all answer from the same adell_plan_f16 call -- bricks = the plain call's statistics rows (cfg 8:
    8 x 8 column units x z segments), split <=> a workspace, and the _ws call (the one that runs with
    statistics) writes the bricks' rows when it does not split. It does not check the plan itself:
    test_plan_of_case does."""
    for c in CASES:
        if c.direction not in ("fwd", "bwd") or c.cfg is None:
            continue
        p = ops.conv3d_plan(c.N, c.size, c.c0, c.c1, c.cout, c.k, c.s, c.p,
                            backward_data=c.direction == "bwd")
        d = ops.make_conv_desc(c.N, c.size, c.c0, c.c1, c.cout, c.k, c.s, c.p)
        ws = _lib.lib().adell_conv3d_splitk_workspace(ctypes.byref(d), int(c.direction == "bwd"))
        assert (ws > 0) == (p.shares > 1), _case_id(c)
        if c.direction == "fwd" and p.cfg != 8:
            Do, Ho, Wo = _out_size(c)
            bricks = (-(-Wo // (1 << p.lTX))) * (-(-Ho // (1 << p.lTY))) * (-(-Do // (1 << p.lTZ)))
            assert bricks == _lib.lib().adell_conv3d_fwd_ntiles_f16x3(ctypes.byref(d)), _case_id(c)
            if p.shares == 1:
                assert bricks == _lib.lib().adell_conv3d_fwd_ntiles_f16x3_ws(ctypes.byref(d)), \
                    _case_id(c)
        assert 0 <= p.lds <= 160 * 1024, _case_id(c)
    refused = [c for c in CASES if c.direction == "fwd" and c.cfg is None]
    for c in refused:
        d = ops.make_conv_desc(c.N, c.size, c.c0, c.c1, c.cout, c.k, c.s, c.p)
        assert _lib.lib().adell_conv3d_fwd_ntiles_f16x3(ctypes.byref(d)) == _lib.E_UNSUPPORTED


# ---- GPU: every case against torch fp64 on the CPU ----------------------------------------------

def _tol(K, K0):
    """The sweep's 2e-5 of the output scale, widened by sqrt(K / K0) for longer accumulations (K0:
    what the sweep's cases accumulate -- 27 taps x 32 channels for y / dX, 3 x 32^3 voxels for
    dW / db)."""
    return 2e-5 * max(1.0, float(np.sqrt(K / K0)))


def _rel(a, b):
    b = b.double()
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-30))


def _conv_shapes():
    """The distinct conv problems of the table (a shape listed for several branches runs once)."""
    seen, out = set(), []
    for c in CASES:
        if c.direction == "convt" or c.cfg is None or c.branch in PLAN_ONLY:
            continue
        key = (c.N, c.size, c.c0, c.c1, c.cout, _triple(c.k), _triple(c.s), _triple(c.p))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


def _gpu_conv(cuda, x0, x1, w, b, r, s, p):
    from adell_mri_amd import functional as HF

    hx0 = ops.ndhwc(x0.to(cuda)).requires_grad_(True)
    hx1 = ops.ndhwc(x1.to(cuda)).requires_grad_(True) if x1 is not None else None
    hw, hb = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    y = HF.conv3d(hx0, hw, hb, s, p, x1=hx1)
    (y * ops.ndhwc(r.to(cuda))).sum().backward()
    torch.cuda.synchronize()
    part = getattr(y, "_adell_partials", None)
    return (y.detach(), part, hx0.grad, None if hx1 is None else hx1.grad, hw.grad, hb.grad)


@pytest.mark.gpu
@pytest.mark.parametrize("case", _conv_shapes(), ids=_case_id)
def test_case_matches_torch_fp64(cuda, case):
    c = case
    k, s, p = _triple(c.k), _triple(c.s), _triple(c.p)
    d = ops.make_conv_desc(c.N, c.size, c.c0, c.c1, c.cout, k, s, p)
    # (the layer must reach the implicit-GEMM kernel, not one of the kernels with their own tests)
    assert c.c0 > 4 and not _lib.lib().adell_conv3d_fwd_s2_fused_applicable(ctypes.byref(d))
    cin, taps = c.c0 + c.c1, int(np.prod(k))
    g = torch.Generator().manual_seed(zlib.crc32(_case_id(c).encode()))
    x0 = torch.randn(c.N, c.c0, *c.size, generator=g)
    x1 = torch.randn(c.N, c.c1, *c.size, generator=g) * 0.5 if c.c1 else None
    w = torch.randn(c.cout, cin, *k, generator=g) / np.sqrt(cin * taps)
    b = torch.randn(c.cout, generator=g)
    xin = x0 if x1 is None else torch.cat([x0, x1], 1)
    ref = [t.double().requires_grad_(True) for t in (xin, w, b)]
    y_ref = F.conv3d(ref[0], ref[1], ref[2], stride=s, padding=p)
    r = torch.randn(y_ref.shape, generator=g)
    (y_ref * r.double()).sum().backward()

    y, part, dx0, dx1, dw, db = _gpu_conv(cuda, x0, x1, w, b, r, s, p)
    assert tuple(y.shape) == tuple(y_ref.shape)
    vox = int(np.prod(y_ref.shape[2:]))
    errs = {
        "y": (_rel(y.cpu(), y_ref.detach()), _tol(taps * cin, 864)),
        "dx0": (_rel(dx0.cpu(), ref[0].grad[:, :c.c0]), _tol(taps * c.cout, 864)),
        "dw": (_rel(dw.cpu(), ref[1].grad), _tol(c.N * vox, 98304)),
        "db": (_rel(db.cpu(), ref[2].grad), _tol(c.N * vox, 98304)),
    }
    if c.c1:
        errs["dx1"] = (_rel(dx1.cpu(), ref[0].grad[:, c.c0:]), _tol(taps * c.cout, 864))
    print(_case_id(c), {n: f"{e:.2e}" for n, (e, _) in errs.items()})
    bad = {n: (e, t) for n, (e, t) in errs.items() if not e < t}
    assert not bad, f"{_case_id(c)}: relative error above the bound: {bad}"

    # statistics partials of the forward epilogue (the fused norm reads them)
    assert part is not None and part.numel() > 0
    mean, rstd = ops.stats_finalize(part, vox, 1e-5)
    yr = y_ref.detach().flatten(2)
    want_mean, want_var = yr.mean(-1), yr.var(-1, unbiased=False)
    assert float((mean.cpu().double() - want_mean).abs().max()) < 1e-5 * float(yr.abs().max() + 1.0)
    var = 1.0 / rstd.cpu().double() ** 2 - 1e-5
    assert float(((var - want_var).abs() / want_var).max()) < 1e-4

    # split-K folds its shares in a fixed order: a second call is bit-identical
    fwd_split = ops.conv3d_plan(c.N, c.size, c.c0, c.c1, c.cout, k, s, p).shares > 1
    bwd_split = ops.conv3d_plan(c.N, c.size, c.c0, c.c1, c.cout, k, s, p,
                                backward_data=True).shares > 1
    if fwd_split or bwd_split:
        y2, part2, dx0b, dx1b, _, _ = _gpu_conv(cuda, x0, x1, w, b, r, s, p)
        if fwd_split:
            assert torch.equal(y, y2) and torch.equal(part, part2)
        if bwd_split:
            assert torch.equal(dx0, dx0b) and (dx1 is None or torch.equal(dx1, dx1b))


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.direction == "convt"], ids=_case_id)
def test_convt_case_matches_torch_fp64(cuda, case):
    from adell_mri_amd import functional as HF

    c = case
    g = torch.Generator().manual_seed(zlib.crc32(_case_id(c).encode()))
    x = torch.randn(c.N, c.c0, *c.size, generator=g)
    w = torch.randn(c.c0, c.cout, *c.k, generator=g) / np.sqrt(c.c0)
    b = torch.randn(c.cout, generator=g)
    assert not ops.convt_k2_ok(tuple(x.shape), w)
    ref = [t.double().requires_grad_(True) for t in (x, w, b)]
    y_ref = F.conv_transpose3d(ref[0], ref[1], ref[2], stride=c.k)
    r = torch.randn(y_ref.shape, generator=g)
    (y_ref * r.double()).sum().backward()

    hx = ops.ndhwc(x.to(cuda)).requires_grad_(True)
    hw, hb = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    y = HF.conv_transpose3d(hx, hw, hb)
    (y * ops.ndhwc(r.to(cuda))).sum().backward()
    torch.cuda.synchronize()
    F_ = int(np.prod(c.k))
    errs = {
        "y": (_rel(y.detach().cpu(), y_ref.detach()), _tol(c.c0, 864)),
        "dx": (_rel(hx.grad.cpu(), ref[0].grad), _tol(F_ * c.cout, 864)),
        "dw": (_rel(hw.grad.cpu(), ref[1].grad), _tol(c.N * int(np.prod(c.size)), 98304)),
        "db": (_rel(hb.grad.cpu(), ref[2].grad), _tol(c.N * int(np.prod(y_ref.shape[2:])), 98304)),
    }
    print(_case_id(c), {n: f"{e:.2e}" for n, (e, _) in errs.items()})
    bad = {n: (e, t) for n, (e, t) in errs.items() if not e < t}
    assert not bad, f"{_case_id(c)}: relative error above the bound: {bad}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in CASES if c.cfg is None], ids=_case_id)
def test_refused_case_raises(cuda, case):
    """No kernel takes a conv whose halo does not fit even the smallest brick: functional.conv3d
    reports it (there is no eager fallback) instead of launching anything."""
    from adell_mri_amd import functional as HF

    c = case
    x = torch.randn(c.N, c.c0, *c.size)
    w = torch.randn(c.cout, c.c0, *_triple(c.k))
    with pytest.raises(AdellHipError, match="unsupported"):
        HF.conv3d(ops.ndhwc(x.to(cuda)), w.to(cuda), None, c.s, c.p)
    torch.cuda.synchronize()
