"""Every launch plan of the depthwise convolution (csrc/ssl.hip adell_dw_plan_fwd / adell_dw_plan_wgrad,
with csrc/dw_dense.hip, dw_mfma.hip and dw_wgrad_mfma.hip), from one case table:

- on the build host (no GPU), each case still gets the plans it is in the table for
  (ops.dwconv3d_plan: the function the launchers take their decisions from), every branch has exactly
  one case, and the thresholds too big to run are checked on the plan alone. A retune that moves a
  shape onto another form, or a case deleted from the table, fails here naming the branch;
- on the GPU, each case runs forward (with and without bias), backward-data, dW and db through
  ops.dwconv3d_fwd / _bwd_data / _bwd_weight against torch's fp64 depthwise conv3d on the CPU, twice
  (bit-identical), dW with and without db, and one case per form through functional.dwconv3d.

Bars (the ones tests/test_dw_mfma_gpu.py and tests/test_ssl.py hold): 2e-6 of the channel's largest
reference value for y and dX; 3e-6 of the largest value for dW / db of the MFMA weight gradient, 5e-6
for the tile and generic ones. The f16x3 MFMA forward scales its operands per (item, channel)
(csrc/dw_mfma.hip), so its 22 bits hold relative to the largest value of that (item, channel) column:
the MFMA cases are also held to 2e-6 per (item, channel), which is what shows a scale or a column
carried over from the item a persistent block met one round earlier.

The weight-gradient cases stay at or below 13 824 voxels per tap, the longest reduction those bars were
set on -- with three exceptions. "config 4 stage 1" needs 11 items of 16^3 voxels before a block of
the persistent forward or a chunk of the MFMA weight gradient meets a second item (45 056 voxels per
tap): it keeps the 3e-6 bar. The two long 2-D generic cases ("generic: realistic 2-D layer", "generic:
grid-stride loop") reduce 65 536 and 1 114 112 voxels per tap: their dW / db bar is 4 x the error of
torch's own fp32 CPU depthwise conv against the same fp64 reference on the same inputs (4 x: another,
equally legitimate summation order), or the standing 5e-6 if that is larger.

(D, H, W) order throughout."""
import collections
import ctypes
import zlib

import pytest
import torch
import torch.nn.functional as F

from adell_mri_amd import _lib, ops

MFMA_FWD = ("mfma", "mfma_stream")


def _cus_grid():
    """The persistent grid of the resident MFMA kernel (one block per CU), from the plan query."""
    try:
        return ops.dwconv3d_plan(65535, 4, (1, 9, 9), 7).blocks
    except _lib.AdellHipError:       # (library not built: every test of this file fails on its own)
        return 256


def _rounds_n(C, rounds=3):
    """Smallest N for which the C / 4 channel groups of N items are `rounds` rounds of the resident
    MFMA kernel's grid with a ragged last one."""
    groups, grid = C // 4, _cus_grid()
    n = ((rounds - 1) * grid) // groups + 1
    while (n * groups) % grid == 0:
        n += 1
    return n


# fwd / wg: the fields of ops.dwconv3d_plan(...) / (..., backward_weight=True) the case is in the table
# for; "min_loop": the plan's loop count is at least this, "ragged": its last round / chunk / split is
# short. opt: "bad" badly scaled operands (below), "fp32" runs under conv precision "fp32",
# "functional" also runs through functional.dwconv3d, "long" the fp32-CPU-derived dW / db bar.
Case = collections.namedtuple("Case", "branch N C size k fwd wg opt")


def _t(K, WT, nseg=1, **kw):
    return dict(form="tile", K=K, WT=WT, nseg=nseg, **kw)


ONE = dict(loop=1)
WG_MFMA1 = dict(form="wgrad_mfma", loop=1)
GEN = dict(form="generic")

CASES = [
    # ---- dense small volumes (7^3 on <= 4^3 voxels, more than 16 of them) -------------------------
    Case("dense", 3, 8, (4, 4, 4), 7, dict(form="dense"), _t(7, 4, **ONE), {"functional"}),
    Case("dense neighbour: 2^3", 2, 8, (2, 2, 2), 7, _t(7, 4), _t(7, 4, **ONE), set()),
    Case("dense neighbour: 5 x 4 x 4", 2, 8, (5, 4, 4), 7, _t(7, 4), _t(7, 4, **ONE), set()),
    # ---- config 4 (ConvNeXt / VICReg) stage shapes, N as small as keeps the form and > 1 item per loop
    Case("config 4 stage 1: 96 x 16^3 (MFMA resident, 2 rounds; wgrad MFMA, 2 items per chunk)", 11,
         96, (16, 16, 16), 7, dict(form="mfma", min_loop=2, ragged=True),
         dict(form="wgrad_mfma", min_loop=2, ragged=True), set()),
    Case("config 4 stage 2: 192 x 8^3 (tile <7,8>; wgrad tile <7,8>, >= 2 items per split)", 22, 192,
         (8, 8, 8), 7, _t(7, 8), _t(7, 8, min_loop=2, ragged=True), set()),
    Case("config 4 stage 3: 384 x 4^3 (dense, ragged item tile; wgrad tile <7,4>, >= 2 items per split)",
         46, 384, (4, 4, 4), 7, dict(form="dense", parts=3), _t(7, 4, min_loop=2, ragged=True), set()),
    Case("config 4 stage 4: 768 x 2^3 (tile <7,4>)", 23, 768, (2, 2, 2), 7, _t(7, 4),
         _t(7, 4, min_loop=2, ragged=True), set()),
    # ---- Toeplitz MFMA form (7^3, rows and columns of 9 .. 16 voxels, C % 4 == 0) ------------------
    Case("MFMA resident, one round; wgrad MFMA, one item per chunk", 2, 8, (5, 12, 13), 7,
         dict(form="mfma", loop=1), WG_MFMA1, {"functional", "bad"}),
    Case("MFMA resident, >= 3 rounds, ragged last round", _rounds_n(28), 28, (2, 9, 9), 7,
         dict(form="mfma", min_loop=3, ragged=True), dict(form="wgrad_mfma"), {"bad"}),
    Case("MFMA streamed (D > 16)", 1, 4, (17, 9, 16), 7, dict(form="mfma_stream", loop=1), WG_MFMA1,
         {"functional", "bad"}),
    Case("MFMA streamed neighbour: D = 16", 1, 4, (16, 9, 16), 7, dict(form="mfma", loop=1), WG_MFMA1,
         {"bad"}),
    Case("wgrad MFMA, >= 3 items per chunk, ragged last chunk", 5, 384, (3, 9, 10), 7,
         dict(form="mfma"), dict(form="wgrad_mfma", min_loop=3, ragged=True), {"functional"}),
    # ---- z-marching ring as the default path (7^3, W in 9 .. 16, D >= 4, not the MFMA form's) -----
    Case("z-ring: H <= 8, one z segment, C % 16 != 0", 2, 24, (5, 8, 12), 7,
         dict(form="zring", nseg=1, vec=1), _t(7, 16, **ONE), {"functional"}),
    Case("z-ring: H > 16, H % 8 != 0, several z segments, D % seglen != 0", 1, 16, (19, 17, 9), 7,
         dict(form="zring", nseg=2, seg=10, vec=1), _t(7, 16, **ONE), set()),
    Case("z-ring: C % 4 != 0 (scalar loads)", 1, 18, (5, 10, 13), 7,
         dict(form="zring", nseg=1, vec=0), _t(7, 16, vec=0, **ONE), set()),
    Case("z-ring: fp32 conv precision", 1, 8, (6, 12, 12), 7, dict(form="zring"), _t(7, 16, **ONE),
         {"fp32"}),
    Case("z-ring neighbour: D = 3 (tile <7,16>)", 1, 16, (3, 8, 12), 7, _t(7, 16), _t(7, 16, **ONE),
         set()),
    Case("z-ring neighbour: W = 8 (tile <7,8>)", 1, 16, (5, 8, 8), 7, _t(7, 8), _t(7, 8, **ONE), set()),
    Case("z-ring neighbour: W = 17 (tile <7,16>, several segments)", 1, 16, (5, 8, 17), 7,
         _t(7, 16, nseg=2, seg=10), _t(7, 16, nseg=2, **ONE), set()),
    # ---- the nine tile instantiations <K, WT>, one x segment (ragged D and H, D < K, ragged channels)
    Case("tile <3,4>: D < K", 2, 8, (2, 5, 4), 3, _t(3, 4), _t(3, 4, **ONE), {"functional"}),
    Case("tile <3,8>: C % 16 != 0", 1, 20, (6, 7, 8), 3, _t(3, 8), _t(3, 8, **ONE), set()),
    Case("tile <3,16>: one segment", 1, 16, (5, 6, 13), 3, _t(3, 16), _t(3, 16, **ONE), set()),
    Case("tile <5,4>: C % 4 != 0, D < K", 2, 6, (3, 5, 3), 5, _t(5, 4, vec=0), _t(5, 4, vec=0, **ONE),
         set()),
    Case("tile <5,8>", 1, 16, (7, 9, 6), 5, _t(5, 8), _t(5, 8, **ONE), set()),
    Case("tile <5,16>: one segment", 1, 12, (6, 5, 9), 5, _t(5, 16), _t(5, 16, **ONE), set()),
    Case("tile <7,4>: C % 4 != 0", 2, 10, (6, 7, 4), 7, _t(7, 4, vec=0), _t(7, 4, vec=0, **ONE), set()),
    Case("tile <7,8>: ragged D and H", 1, 16, (5, 6, 7), 7, _t(7, 8), _t(7, 8, **ONE), set()),
    # ---- WT = 16 with several x segments, the last of one voxel ----------------------------------
    Case("tile <3,16>: several segments, last of one voxel", 1, 16, (5, 6, 29), 3,
         _t(3, 16, nseg=3, seg=14), _t(3, 16, nseg=3, **ONE), set()),
    Case("tile <5,16>: several segments, last of one voxel", 1, 8, (4, 5, 25), 5,
         _t(5, 16, nseg=3, seg=12), _t(5, 16, nseg=3, **ONE), set()),
    Case("tile <7,16>: several segments, last of one voxel", 1, 20, (4, 6, 21), 7,
         _t(7, 16, nseg=3, seg=10), _t(7, 16, nseg=3, **ONE), set()),
    Case("wgrad tile <3,16>: several segments, >= 2 items per split", 1, 256, (12, 20, 29), 3,
         _t(3, 16, nseg=3), _t(3, 16, nseg=3, min_loop=2, ragged=True), set()),
    # ---- generic kernels (non-cubic taps: every 2-D depthwise layer arrives as (1, k, k)) ----------
    Case("generic: (1,3,3) on D = 1", 2, 8, (1, 10, 11), (1, 3, 3), GEN, GEN, {"functional"}),
    Case("generic: (1,7,7) on D = 1", 1, 16, (1, 12, 9), (1, 7, 7), GEN, GEN, set()),
    Case("generic: non-cubic 3-D kernel", 1, 8, (7, 6, 9), (3, 1, 5), GEN, GEN, set()),
    Case("generic: C > 64, C % 64 != 0", 1, 72, (1, 6, 7), (1, 3, 3), dict(form="generic", vec=1),
         dict(form="generic", parts=2), set()),
    Case("generic: C % 4 != 0", 2, 6, (4, 5, 6), (3, 3, 5), dict(form="generic", vec=0), GEN, set()),
    # 65 536 voxels per tap. torch's fp32 CPU conv on these inputs, measured on the build host: dW
    # 9.5e-7, db 3.6e-7 of the largest value; 4 x that is below the standing 5e-6 -> bars 5e-6, 5e-6
    Case("generic: realistic 2-D layer", 4, 32, (1, 128, 128), (1, 7, 7), GEN, GEN, {"long"}),
    # more than 16 384 blocks x 256 threads of work: the forward's grid-stride loop runs twice; 1 114 112
    # voxels per tap. torch's fp32 CPU conv, measured on the build host: dW 1.6e-6, db 1.3e-6 -> bars
    # 6.4e-6 (dW) and 5.0e-6 (db); the test recomputes both from the machine it runs on. (The generic
    # weight gradient missed them while its lanes summed in fp32: dW 1.1e-5, db 9.9e-6; fp64 now.)
    Case("generic: grid-stride loop", 17, 16, (1, 256, 256), (1, 3, 3),
         dict(form="generic", blocks=16384, min_loop=2), GEN, {"long"}),
]

# every branch has exactly one case: deleting a case fails test_table_covers_every_branch by name
BRANCHES = [
    "dense", "dense neighbour: 2^3", "dense neighbour: 5 x 4 x 4",
    "config 4 stage 1: 96 x 16^3 (MFMA resident, 2 rounds; wgrad MFMA, 2 items per chunk)",
    "config 4 stage 2: 192 x 8^3 (tile <7,8>; wgrad tile <7,8>, >= 2 items per split)",
    "config 4 stage 3: 384 x 4^3 (dense, ragged item tile; wgrad tile <7,4>, >= 2 items per split)",
    "config 4 stage 4: 768 x 2^3 (tile <7,4>)",
    "MFMA resident, one round; wgrad MFMA, one item per chunk",
    "MFMA resident, >= 3 rounds, ragged last round", "MFMA streamed (D > 16)",
    "MFMA streamed neighbour: D = 16", "wgrad MFMA, >= 3 items per chunk, ragged last chunk",
    "z-ring: H <= 8, one z segment, C % 16 != 0",
    "z-ring: H > 16, H % 8 != 0, several z segments, D % seglen != 0",
    "z-ring: C % 4 != 0 (scalar loads)", "z-ring: fp32 conv precision",
    "z-ring neighbour: D = 3 (tile <7,16>)", "z-ring neighbour: W = 8 (tile <7,8>)",
    "z-ring neighbour: W = 17 (tile <7,16>, several segments)",
    "tile <3,4>: D < K", "tile <3,8>: C % 16 != 0", "tile <3,16>: one segment",
    "tile <5,4>: C % 4 != 0, D < K", "tile <5,8>", "tile <5,16>: one segment",
    "tile <7,4>: C % 4 != 0", "tile <7,8>: ragged D and H",
    "tile <3,16>: several segments, last of one voxel",
    "tile <5,16>: several segments, last of one voxel",
    "tile <7,16>: several segments, last of one voxel",
    "wgrad tile <3,16>: several segments, >= 2 items per split",
    "generic: (1,3,3) on D = 1", "generic: (1,7,7) on D = 1", "generic: non-cubic 3-D kernel",
    "generic: C > 64, C % 64 != 0", "generic: C % 4 != 0", "generic: realistic 2-D layer",
    "generic: grid-stride loop",
]


def _triple(k):
    return (k,) * 3 if isinstance(k, int) else tuple(k)


def _case_id(c):
    return "n{}_c{}_{}_k{}{}".format(c.N, c.C, "x".join(map(str, c.size)),
                                     "".join(map(str, _triple(c.k))), "_fp32" if "fp32" in c.opt else "")


class _precision:
    """conv precision "fp32" for the cases that ask for it, restored on the way out."""

    def __init__(self, case):
        self.on = "fp32" in case.opt

    def __enter__(self):
        from adell_mri_amd import functional as HF

        self.old = HF.CONV_PRECISION
        if self.on:
            HF.set_conv_precision("fp32")

    def __exit__(self, *exc):
        from adell_mri_amd import functional as HF

        if self.on:
            HF.set_conv_precision(self.old)


def _plans(c, aligned=(True, True)):
    with _precision(c):
        return (ops.dwconv3d_plan(c.N, c.C, c.size, c.k, aligned=aligned),
                ops.dwconv3d_plan(c.N, c.C, c.size, c.k, backward_weight=True, aligned=aligned))


def _work(c, plan, wgrad):
    """(work items, blocks / chunks / splits that share them) of a plan with a loop."""
    if plan.form in MFMA_FWD:
        return plan.parts, plan.blocks
    if plan.form == "wgrad_mfma":
        return c.N, plan.parts
    if plan.form == "tile" and wgrad:
        D, H, _ = c.size
        return c.N * (-(-D // 4)) * (-(-H // 4)) * plan.nseg, plan.parts
    if plan.form == "dense":
        return c.N, plan.parts
    raise AssertionError(f"no loop in form {plan.form}")


def _mismatch(c, plan, want, wgrad):
    bad = []
    for key, v in want.items():
        if key == "min_loop":
            if plan.loop < v:
                bad.append(f"loop {plan.loop} < {v}")
        elif key == "ragged":
            total, groups = _work(c, plan, wgrad)
            if (groups * plan.loop != total) != v:
                bad.append(f"{total} items over {groups} x {plan.loop}: ragged is {not v}")
        elif getattr(plan, key) != v:
            bad.append(f"{key} {getattr(plan, key)} != {v}")
    return bad


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_plan_of_case(case):
    fwd, wg = _plans(case)
    bad = [f"forward / backward-data: {m}" for m in _mismatch(case, fwd, case.fwd, False)]
    bad += [f"backward-weight: {m}" for m in _mismatch(case, wg, case.wg, True)]
    assert not bad, (f"branch '{case.branch}' lost its case {_case_id(case)}: {bad}; the planner now "
                     f"gives {fwd} and {wg}. Update the case table so the branch keeps a case.")
    if fwd.form in MFMA_FWD or wg.form == "wgrad_mfma":
        assert case.C % 4 == 0


def test_table_covers_every_branch():
    have = [c.branch for c in CASES]
    assert len(set(have)) == len(have), "a branch has two cases: give each its own tag"
    missing = [b for b in BRANCHES if b not in have]
    assert not missing, f"no case for: {missing}"
    assert not set(have) - set(BRANCHES), f"not in BRANCHES: {sorted(set(have) - set(BRANCHES))}"


def test_table_selects_every_form_and_tile_instantiation():
    """What the tags promise, counted on the plans themselves: every form by shape alone (no tuning
    switch, default precision); all nine <K, WT> with one segment; K = 3, 5, 7 at WT = 16 with several
    segments and a last segment of one voxel; the weight gradient of every instantiation the forward
    cases select with one item per split; <7,8>, <7,4> and a several-segment K = 3 with more."""
    fwd_forms, wg_forms, single, multi, wg_one, wg_many = set(), set(), set(), set(), set(), set()
    for c in CASES:
        if "fp32" in c.opt:
            continue
        fwd, wg = _plans(c)
        fwd_forms.add(fwd.form)
        wg_forms.add(wg.form)
        if fwd.form == "tile":
            (single if fwd.nseg == 1 else multi).add((fwd.K, fwd.WT))
            if fwd.nseg > 1 and c.size[2] - (fwd.nseg - 1) * fwd.seg == 1:
                multi.add((fwd.K, "last segment of one voxel"))
        if wg.form == "tile":
            (wg_one if wg.loop == 1 else wg_many).add((wg.K, wg.WT, wg.nseg > 1))
    assert fwd_forms == {"dense", "mfma", "mfma_stream", "zring", "tile", "generic"}
    assert wg_forms == {"wgrad_mfma", "tile", "generic"}
    nine = {(K, WT) for K in (3, 5, 7) for WT in (4, 8, 16)}
    assert single == nine, f"tile instantiations without a one-segment case: {sorted(nine - single)}"
    want = {(K, v) for K in (3, 5, 7) for v in (16, "last segment of one voxel")}
    assert want <= multi, f"several-segment cases missing: {sorted(map(str, want - multi))}"
    assert {(K, WT) for K, WT, _ in wg_one} >= single | {(K, 16) for K in (3, 5, 7)}
    assert {(K, 16, True) for K in (3, 5, 7)} <= wg_one
    assert {(7, 8, False), (7, 4, False), (3, 16, True)} <= wg_many


def test_host_only_thresholds():
    """Limits too large to run: N = 65 536 leaves the MFMA forward (its grid's y extent), a ring or
    tile grid of more than 2^31 - 1 blocks falls through to the next form."""
    P = ops.dwconv3d_plan
    assert P(65535, 8, (1, 9, 9), 7).form == "mfma"
    assert P(65536, 8, (1, 9, 9), 7).form == "tile"          # (D < 4: not the ring's either)
    assert P(65536, 8, (4, 9, 9), 7).form == "zring"
    # ring: N x 1 row tile x 3 channel blocks x 1 segment
    n = (2 ** 31 - 1) // 3
    ring = P(n, 48, (4, 8, 16), 7)
    assert ring.form == "zring" and ring.blocks == 3 * n <= 2 ** 31 - 1
    assert P(n + 1, 48, (4, 8, 16), 7).form == "generic"     # (the tile grid is larger still)
    # tile: N x 2 channel blocks
    tile = P(2 ** 30 - 1, 32, (4, 4, 4), 3)
    assert tile.form == "tile" and tile.blocks == 2 ** 31 - 2
    assert P(2 ** 30, 32, (4, 4, 4), 3).form == "generic"
    assert P(2 ** 30 - 1, 32, (4, 4, 4), 3, backward_weight=True).form == "tile"
    assert P(2 ** 30, 32, (4, 4, 4), 3, backward_weight=True).form == "generic"
    # dense: 65 535 item blocks of 16
    assert P(16 * 65535, 4, (4, 4, 4), 7).form == "dense"
    assert P(16 * 65535 + 1, 4, (4, 4, 4), 7).form == "tile"


def test_plan_honours_alignment_switches_and_precision():
    from adell_mri_amd import functional as HF

    P = ops.dwconv3d_plan
    mf, dn, tl = (2, 8, (5, 12, 13), 7), (3, 8, (4, 4, 4), 7), (1, 16, (5, 6, 7), 7)
    gn = (2, 8, (1, 10, 11), (1, 3, 3))
    assert P(*mf).form == "mfma" and P(*mf, backward_weight=True).form == "wgrad_mfma"
    for al in ((False, True), (True, False)):
        assert P(*mf, aligned=al).form == "zring"
        assert P(*mf, backward_weight=True, aligned=al).form == "tile"
        assert P(*mf, backward_weight=True, aligned=al).vec == 0
        assert P(*dn, aligned=al).form == "tile"
        assert P(*gn, aligned=al).vec == 0
    # the ring and the forward tiles stage the input only; the weight gradient stages both tensors
    assert P(*mf, aligned=(False, True)).vec == 0 and P(*mf, aligned=(True, False)).vec == 1
    assert P(*tl, aligned=(False, True)).vec == 0 and P(*tl, aligned=(True, False)).vec == 1
    with _lib.tuning(dw_nomfma=1):
        assert P(*mf).form == "zring" and P(*mf, backward_weight=True).form == "tile"
        assert P(*dn).form == "tile"
    with _lib.tuning(dw_wgrad_nomfma=1):
        assert P(*mf).form == "mfma" and P(*mf, backward_weight=True).form == "tile"
    old = HF.CONV_PRECISION
    try:
        HF.set_conv_precision("fp32")
        assert P(*mf).form == "zring" and P(*dn).form == "tile"
        assert P(*mf, backward_weight=True).form == "tile"
        HF.set_conv_precision("f16x3")
        assert P(*mf).form == "mfma"
    finally:
        HF.set_conv_precision(old)


def test_plan_query_agrees_with_the_other_entry_points():
    """Plumbing: adell_dw_mfma_ok / adell_dw_dense_ok / adell_dw_wgrad_mfma_ok and the workspace query
    answer from the functions the plan query calls."""
    L = _lib.lib()
    buf = (ctypes.c_float * 16)()                 # never dereferenced
    base = ctypes.addressof(buf)
    p0 = base + (-base) % 16
    for c in CASES:
        with _precision(c):
            k = _triple(c.k)
            for off in (0, 4):
                al = off == 0
                fwd = ops.dwconv3d_plan(c.N, c.C, c.size, k, aligned=(al, al))
                wg = ops.dwconv3d_plan(c.N, c.C, c.size, k, backward_weight=True, aligned=(al, al))
                args = (c.N, c.C, *c.size, *k, p0 + off, p0 + off)
                assert bool(L.adell_dw_mfma_ok(*args)) == (fwd.form in MFMA_FWD), c.branch
                assert bool(L.adell_dw_dense_ok(*args)) == (fwd.form == "dense"), c.branch
                assert bool(L.adell_dw_wgrad_mfma_ok(*args)) == (wg.form == "wgrad_mfma"), c.branch
            need = max(ops.dwconv3d_plan(c.N, c.C, c.size, k, backward_weight=True,
                                         aligned=(a, a)).workspace for a in (True, False))
            got = L.adell_dwconv3d_bwd_weight_workspace_floats(c.N, c.C, *c.size, *k)
            assert got == need, c.branch


# ---- GPU: every case against torch fp64 on the CPU ----------------------------------------------

def _inputs(c):
    """fp32-representable operands as fp64 tensors (the reference sees exactly what the kernels do).
    "bad": the x300 channel and x50 plane of tests/test_dw_mfma_gpu.py, plus items 1e4 / 1e-4 apart
    that one block of the persistent kernel meets in consecutive rounds (x and dy the other way round,
    so both orders occur and dW sees balanced products)."""
    k = _triple(c.k)
    g = torch.Generator().manual_seed(zlib.crc32(_case_id(c).encode()))
    x = torch.randn(c.N, c.C, *c.size, generator=g)
    dy = torch.randn(c.N, c.C, *c.size, generator=g)
    w = torch.randn(c.C, 1, *k, generator=g) / float(k[0] * k[1] * k[2]) ** 0.5
    b = torch.randn(c.C, generator=g)
    if "bad" in c.opt:
        for t in (x, dy):
            t[:, 1] *= 300.0
            t[0, :, c.size[0] // 2] *= 50.0
        w[2] *= 1e-3
        groups, grid = c.C // 4, _cus_grid()
        if c.N * groups > grid:
            first = 1                                      # its channel groups are works first * groups ..
            later = sorted({(first * groups + gq + grid) // groups for gq in range(groups)})
            assert first not in later and later[-1] < c.N
            x[first] *= 1e4
            dy[first] *= 1e-4
            for n in later:
                x[n] *= 1e-4
                dy[n] *= 1e4
    return [t.double() for t in (x, dy, w, b)]


def _reference(x, dy, w, b, k, dtype=torch.float64):
    xr, wr, br = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    y = F.conv3d(xr, wr, br, padding=[q // 2 for q in k], groups=x.shape[1])
    y.backward(dy.to(dtype))
    return y.detach(), xr.grad, wr.grad, br.grad


def _rel(a, b):
    b = b.double()
    return float((a.double() - b).abs().max() / (b.abs().max() + 1e-300))


def _rel_over(a, b, dims):
    """Largest error relative to the reference's largest value, separately along the kept dims."""
    b = b.double()
    return float(((a.double() - b).abs().amax(dims) / (b.abs().amax(dims) + 1e-300)).max())


def _run(cuda, c, x, dy, w, b, want_db=True, bias=True):
    xd, dyd = ops.ndhwc(x.float().to(cuda)), ops.ndhwc(dy.float().to(cuda))
    wd, bd = w.float().to(cuda), b.float().to(cuda)
    k = _triple(c.k)
    y = ops.dwconv3d_fwd(xd, wd, bd if bias else None)
    dx = ops.dwconv3d_bwd_data(dyd, wd)
    dw, db = ops.dwconv3d_bwd_weight(xd, dyd, k, want_db)
    torch.cuda.synchronize()
    return y, dx, dw, db


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_case_matches_torch_fp64(cuda, case):
    c = case
    k = _triple(c.k)
    x, dy, w, b = _inputs(c)
    y_ref, dx_ref, dw_ref, db_ref = _reference(x, dy, w, b, k)
    y0_ref = y_ref - b.view(1, -1, 1, 1, 1)
    with _precision(c):
        fwd, wg = _plans(c)
        assert not _mismatch(c, fwd, c.fwd, False) and not _mismatch(c, wg, c.wg, True), (fwd, wg)
        y, dx, dw, db = _run(cuda, c, x, dy, w, b)
        y0, _, dw_nodb, none = _run(cuda, c, x, dy, w, b, want_db=False, bias=False)
        again = _run(cuda, c, x, dy, w, b)
        if "functional" in c.opt:
            from adell_mri_amd import functional as HF

            leaves = [ops.ndhwc(x.float().to(cuda)).requires_grad_(True),
                      w.float().to(cuda).requires_grad_(True), b.float().to(cuda).requires_grad_(True)]
            fy = HF.dwconv3d(*leaves)
            fy.backward(ops.ndhwc(dy.float().to(cuda)))
            torch.cuda.synchronize()
            for got, want in zip((fy.detach(), *[t.grad for t in leaves]), (y, dx, dw, db)):
                assert torch.equal(got, want)
    # a second call is bit-identical (fixed fold orders, no atomics); db is optional
    for got, want in zip(again, (y, dx, dw, db)):
        assert torch.equal(got, want)
    assert none is None and torch.equal(dw_nodb, dw)

    chan = (0, 2, 3, 4)
    wg_bar = 3e-6 if wg.form == "wgrad_mfma" else 5e-6
    dw_bar = db_bar = wg_bar
    if "long" in c.opt:
        _, _, dw32, db32 = _reference(x, dy, w, b, k, torch.float32)
        e_dw, e_db = _rel(dw32, dw_ref), _rel(db32, db_ref)
        dw_bar, db_bar = max(wg_bar, 4 * e_dw), max(wg_bar, 4 * e_db)
        print(f"{_case_id(c)}: torch fp32 CPU dW {e_dw:.2e} db {e_db:.2e} -> bars {dw_bar:.2e} {db_bar:.2e}")
    errs = {
        "y": (_rel_over(y.cpu(), y_ref, chan), 2e-6),
        "y, no bias": (_rel_over(y0.cpu(), y0_ref, chan), 2e-6),
        "dx": (_rel_over(dx.cpu(), dx_ref, chan), 2e-6),
        "dw": (_rel(dw.cpu(), dw_ref), dw_bar),
        "db": (_rel(db.cpu(), db_ref), db_bar),
    }
    if fwd.form in MFMA_FWD:
        errs["y, no bias, per (item, channel)"] = (_rel_over(y0.cpu(), y0_ref, (2, 3, 4)), 2e-6)
        errs["dx, per (item, channel)"] = (_rel_over(dx.cpu(), dx_ref, (2, 3, 4)), 2e-6)
    print(_case_id(c), fwd.form, wg.form, {n: f"{e:.2e}" for n, (e, _) in errs.items()})
    bad = {n: (e, t) for n, (e, t) in errs.items() if not e < t}
    assert not bad, f"'{c.branch}' {_case_id(c)}: relative error above the bound: {bad}"


# one case per vector-capable form, C % 4 == 0, with every tensor 4 bytes into its buffer: the scalar
# fallback of adell_dw_load_quad behind an unaligned base, which a torch allocation never has
MISALIGNED = [
    Case("z-ring, unaligned base", 2, 24, (5, 8, 12), 7, dict(form="zring", vec=0), _t(7, 16, vec=0),
         set()),
    Case("tile, unaligned base", 1, 20, (6, 7, 8), 3, _t(3, 8, vec=0), _t(3, 8, vec=0), set()),
    Case("generic, unaligned base", 2, 8, (1, 10, 11), (1, 3, 3), dict(form="generic", vec=0), GEN,
         set()),
]


@pytest.mark.parametrize("case", MISALIGNED, ids=_case_id)
def test_plan_of_unaligned_case(case):
    fwd, wg = _plans(case, aligned=(False, False))
    assert not _mismatch(case, fwd, case.fwd, False), (case.branch, fwd)
    assert not _mismatch(case, wg, case.wg, True), (case.branch, wg)
    assert _plans(case)[0].vec == 1


def _offset_buffer(t, cuda):
    """`t` (logical NCDHW, or any shape for the outputs) as dense NDHWC memory that starts 4 bytes into
    a 16-byte aligned allocation."""
    flat = t.permute(0, 2, 3, 4, 1).contiguous().float().reshape(-1)
    buf = torch.zeros(flat.numel() + 4, device=cuda, dtype=torch.float32)
    view = buf[1:1 + flat.numel()]
    view.copy_(flat.to(cuda))
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    return buf, view


@pytest.mark.gpu
@pytest.mark.parametrize("case", MISALIGNED, ids=_case_id)
def test_unaligned_base_through_the_raw_abi(cuda, case):
    c = case
    k = _triple(c.k)
    N, C, (D, H, W) = c.N, c.C, c.size
    x, dy, w, b = _inputs(c)
    y_ref, dx_ref, dw_ref, db_ref = _reference(x, dy, w, b, k)
    L = _lib.lib()
    xb, xv = _offset_buffer(x, cuda)
    dyb, dyv = _offset_buffer(dy, cuda)
    yb, yv = _offset_buffer(torch.zeros_like(x), cuda)
    dxb, dxv = _offset_buffer(torch.zeros_like(x), cuda)
    wd, bd = w.float().to(cuda).contiguous(), b.float().to(cuda)
    dw = torch.empty((C, 1, *k), device=cuda, dtype=torch.float32)
    db = torch.empty((C,), device=cuda, dtype=torch.float32)
    nws = L.adell_dwconv3d_bwd_weight_workspace_floats(N, C, D, H, W, *k)
    ws = torch.empty((max(nws, 1),), device=cuda, dtype=torch.float32)
    dims = (N, C, D, H, W, *k)
    st = ops._stream()
    _lib.check(L.adell_dwconv3d_fwd(*dims, xv.data_ptr(), wd.data_ptr(), bd.data_ptr(), yv.data_ptr(),
                                    st))
    _lib.check(L.adell_dwconv3d_bwd_data(*dims, dyv.data_ptr(), wd.data_ptr(), dxv.data_ptr(), st))
    _lib.check(L.adell_dwconv3d_bwd_weight(*dims, xv.data_ptr(), dyv.data_ptr(), dw.data_ptr(),
                                           db.data_ptr(), ws.data_ptr(), st))
    torch.cuda.synchronize()
    # nothing was written in front of or behind the tensors
    for buf in (yb, dxb):
        assert float(buf[0]) == 0.0 and float(buf[-3:].abs().max()) == 0.0
    y = yv.view(N, D, H, W, C).permute(0, 4, 1, 2, 3).cpu()
    dx = dxv.view(N, D, H, W, C).permute(0, 4, 1, 2, 3).cpu()
    chan = (0, 2, 3, 4)
    errs = {"y": (_rel_over(y, y_ref, chan), 2e-6), "dx": (_rel_over(dx, dx_ref, chan), 2e-6),
            "dw": (_rel(dw.cpu(), dw_ref), 5e-6), "db": (_rel(db.cpu(), db_ref), 5e-6)}
    print(_case_id(c), {n: f"{e:.2e}" for n, (e, _) in errs.items()})
    bad = {n: (e, t) for n, (e, t) in errs.items() if not e < t}
    assert not bad, f"'{c.branch}' {_case_id(c)}: relative error above the bound: {bad}"
