#!/usr/bin/env python3
"""Dense pin of the f16x3 conv launch planner (csrc/conv3d.hip adell_plan_f16): the answers of the
host-only query entries over a fixed grid of descriptors.

    python tools/conv_plan_sweep.py        -> tests/golden/conv_f16x3_plan_sweep.npz
    python tools/conv_plan_sweep.py wgrad  -> tests/golden/conv_wgrad_plan_sweep.npz

Per conv descriptor (ANSWER_COLUMNS): adell_conv3d_f16x3_plan forward and backward-data,
adell_conv3d_splitk_workspace in both directions, adell_conv3d_fwd_ntiles_f16x3 and its _ws form,
adell_conv3d_f16x3_rows_ok and adell_conv3d_bwd_data_f16x3_adn_ntiles; per transposed-conv
descriptor adell_convtranspose3d_f16x3_plan. The grid holds the conv cases of tests/test_conv_plans.py,
the case lists of tests/test_adn_fused_gpu.py and tests/test_split_rows_gpu.py, a product of batch
sizes, volumes, channel counts and (kernel, stride, padding) triples, and the 3^3 stride-1 part of
that product again under each launch-plan switch.

The weight-gradient section pins the host path of csrc/conv_wgrad_f16.hip and csrc/conv_wgrad.hip
the same way (WGRAD_COLUMNS): both workspace queries, adell_conv3d_bwd_weight_f16x3_rows_ok,
adell_wgrad_zring_plan and every entry of adell_conv3d_bwd_weight_f16x3_plan (route, regions,
per-plane instance and geometry, fp32 instance), over the conv product above plus rows of <= 4 input
channels, the shapes of tests/test_wgrad_s2_gpu.py, test_wgrad_zring_gpu.py and
test_wgrad_zring_shape_gpu.py and the "wgrad" cases of tests/test_conv_plans.py, each under no switch,
wgrad_nozring and wgrad_no16; and adell_convtranspose3d_bwd_weight_workspace over the transposed grid.

No GPU is needed and the planner reads no device property, so the file is the same on the build
host and on the MI355X. The one exception is the stride-2 weight-gradient route, which reads the CU
count: adell_cu_count() answers 256 without a device and 256 on the MI355X, so that file is the same
on both too. The script uses the C ABI only, and ADELL_HIP_LIBRARY selects the library:
a refactor of the planner generates the file from the build of its PARENT commit and must then
reproduce it (tests/test_conv_plan_sweep.py). A deliberate retune regenerates the file with this
tool, as it updates the case table of tests/test_conv_plans.py.
"""
import ctypes
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_f16x3_plan_sweep.npz")
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

# launch-plan switches (adell_set_tuning) a descriptor is planned under; 0 = none
SWITCHES = (None, "igemm_nospec", "igemm_no8", "no_splitk", "igemm_no16")
# conv descriptor row: switch index, N, D, H, W, C0, C1, Cout, k (3), stride (3), padding (3)
ANSWER_COLUMNS = (
    ["fwd_rc", "fwd_cfg", "fwd_BM", "fwd_BN", "fwd_lTX", "fwd_lTY", "fwd_lTZ", "fwd_shares", "fwd_lds",
     "bwd_rc", "bwd_cfg", "bwd_BM", "bwd_BN", "bwd_lTX", "bwd_lTY", "bwd_lTZ", "bwd_shares", "bwd_lds",
     "ws_fwd", "ws_bwd", "ntiles", "ntiles_ws", "rows_ok", "adn_ntiles"])
# transposed-conv descriptor row: switch index, N, D, H, W, Cin, Cout, FD, FH, FW
CONVT_COLUMNS = ["rc", "cfg", "BM", "BN", "lTX", "lTY", "lTZ", "shares", "lds"]

SIZES = [(4, 4, 4), (8, 8, 8), (16, 16, 16), (32, 32, 32), (64, 64, 64), (128, 128, 128),
         (3, 8, 8), (9, 9, 33), (8, 12, 20), (16, 32, 32), (32, 64, 64)]
CHANNELS = [(8, 0), (16, 0), (24, 0), (32, 0), (48, 0), (64, 0), (128, 0), (256, 0), (512, 0),
            (16, 16), (32, 16), (32, 32), (64, 64), (128, 128), (256, 256)]
COUTS = [16, 24, 32, 48, 64, 96, 128, 256, 512]
KSP = [((3, 3, 3), (1, 1, 1), (1, 1, 1)), ((1, 1, 1), (1, 1, 1), (0, 0, 0)),
       ((5, 5, 5), (1, 1, 1), (2, 2, 2)), ((3, 3, 3), (2, 2, 2), (1, 1, 1)),
       ((2, 2, 2), (2, 2, 2), (0, 0, 0)), ((7, 7, 7), (2, 2, 2), (3, 3, 3)),
       ((3, 3, 3), (1, 2, 2), (1, 1, 1))]
# ---- weight gradient ------------------------------------------------------------------------------
WGRAD_GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_wgrad_plan_sweep.npz")
WGRAD_SWITCHES = (None, "wgrad_nozring", "wgrad_no16")
PLAN_COLUMNS = (["route", "R", "ws_lo", "ws_hi", "rows_ok_q", "MAXJ", "PFX", "PFY", "lTY", "TCI", "TCO",
                 "ksplit", "lds", "grid_x", "grid_y", "grid_z"] + [f"q_zr{i}" for i in range(8)]
                + ["fp32_maxj"])
WGRAD_COLUMNS = (["ws_f16x3", "ws_fp32", "rows_ok", "zr_rc"] + [f"zr{i}" for i in range(8)]
                 + ["plan_rc"] + PLAN_COLUMNS)
WGRAD_SMALL_CHANNELS = [(1, 0), (2, 0), (4, 0), (2, 2), (3, 1)]
# tests/test_wgrad_s2_gpu.py: its 32 -> 32 stride-2 shapes and the shapes that keep their kernels
WGRAD_S2_SHAPES = ([(n, size, 32, 32, 2, 1) for n, size in
                    [(2, (16, 16, 16)), (1, (12, 20, 10)), (1, (8, 8, 72)), (3, (2, 2, 2)),
                     (1, (64, 64, 64)), (5, (8, 16, 8)), (2, (64, 64, 64)), (2, (64, 128, 128))]]
                   + [(1, (12, 12, 12), 64, 32, 2, 1), (1, (12, 12, 12), 32, 32, 2, 0),
                      (1, (12, 12, 12), 32, 32, 1, 1)])
ROUTES = {"small": 0, "zring32": 1, "zring16": 2, "s2": 3, "plane": 4}
F16_INSTANCES = {(2, 0, 0), (3, 0, 0), (5, 4, 2), (5, 7, 2), (5, 4, 4), (5, 0, 0), (7, 0, 0), (9, 0, 0)}

CONVT_SIZES = [(4, 4, 4), (8, 8, 8), (16, 16, 16), (32, 32, 32), (3, 4, 4), (8, 12, 20)]
CONVT_CIN = [16, 32, 40, 48, 64, 128, 256]
CONVT_COUT = [8, 16, 20, 31, 32, 48, 64, 128]


def _triple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 3


def grid():
    """(conv descriptors [n, 17], transposed-conv descriptors [m, 10]) as int32 arrays."""
    import test_adn_fused_gpu
    import test_conv_plans
    import test_split_rows_gpu

    conv, convt = [], []
    for c in test_conv_plans.CASES:
        if c.direction in ("fwd", "bwd"):
            conv.append((0, c.N, *c.size, c.c0, c.c1, c.cout, *_triple(c.k), *_triple(c.s),
                         *_triple(c.p)))
        elif c.direction == "convt":
            convt.append((0, c.N, *c.size, c.c0, c.cout, *c.k))
    for n, c0, c1, cout, size, _ in test_adn_fused_gpu.FUSED_CASES + test_split_rows_gpu.FORWARD_CASES:
        conv.append((0, n, *size, c0, c1, cout, 3, 3, 3, 1, 1, 1, 1, 1, 1))
    for sw in range(len(SWITCHES)):
        for n, size, (c0, c1), cout, (k, s, p) in itertools.product((1, 2), SIZES, CHANNELS, COUTS,
                                                                    KSP if sw == 0 else KSP[:1]):
            conv.append((sw, n, *size, c0, c1, cout, *k, *s, *p))
    for n, size, cin, cout, f in itertools.product((1, 2), CONVT_SIZES, CONVT_CIN, CONVT_COUT,
                                                   itertools.product((1, 2), repeat=3)):
        convt.append((0, n, *size, cin, cout, *f))
    return np.asarray(conv, np.int32), np.asarray(convt, np.int32)


def answers(conv, convt):
    """The library's answers for the two descriptor tables: int64 [n, 24] and [m, 9]."""
    from adell_mri_amd import _lib, ops

    L = _lib.lib()
    out = (ctypes.c_int * 8)()
    a = np.zeros((len(conv), len(ANSWER_COLUMNS)), np.int64)
    t = np.zeros((len(convt), len(CONVT_COLUMNS)), np.int64)
    for sw, name in enumerate(SWITCHES):
        rows = np.nonzero(conv[:, 0] == sw)[0]
        trows = np.nonzero(convt[:, 0] == sw)[0]
        with _lib.tuning(**({name: 1} if name else {})):
            for i in rows:
                r = [int(v) for v in conv[i]]
                d = ops.make_conv_desc(r[1], tuple(r[2:5]), r[5], r[6], r[7], tuple(r[8:11]),
                                       tuple(r[11:14]), tuple(r[14:17]))
                ref = ctypes.byref(d)
                for direction in (0, 1):
                    out[:] = [0] * 8
                    rc = L.adell_conv3d_f16x3_plan(ref, direction, out)
                    a[i, 9 * direction] = rc
                    if rc == 0:
                        a[i, 9 * direction + 1:9 * direction + 9] = list(out)
                a[i, 18] = L.adell_conv3d_splitk_workspace(ref, 0)
                a[i, 19] = L.adell_conv3d_splitk_workspace(ref, 1)
                a[i, 20] = L.adell_conv3d_fwd_ntiles_f16x3(ref)
                a[i, 21] = L.adell_conv3d_fwd_ntiles_f16x3_ws(ref)
                a[i, 22] = L.adell_conv3d_f16x3_rows_ok(ref)
                a[i, 23] = L.adell_conv3d_bwd_data_f16x3_adn_ntiles(ref)
            for i in trows:
                r = [int(v) for v in convt[i]]
                out[:] = [0] * 8
                rc = L.adell_convtranspose3d_f16x3_plan(*r[1:10], out)
                t[i, 0] = rc
                if rc == 0:
                    t[i, 1:] = list(out)
    return a, t


def _parametrized(fn):
    """The argvalues of a test's single parametrize mark."""
    (mark,) = [m for m in fn.pytestmark if m.name == "parametrize"]
    return mark.args[1]


def wgrad_grid():
    """Weight-gradient descriptors [n, 17] (layout of the conv table; column 0 indexes
    WGRAD_SWITCHES): the same descriptors, in the same order, under each switch."""
    import test_conv_plans
    import test_wgrad_zring_gpu
    import test_wgrad_zring_shape_gpu

    base = []
    for c in test_conv_plans.CASES:
        if c.direction == "wgrad":
            base.append((c.N, *c.size, c.c0, c.c1, c.cout, *_triple(c.k), *_triple(c.s), *_triple(c.p)))
    for n, c0, c1, cout, size, pad in (
            list(_parametrized(test_wgrad_zring_gpu.test_zring_matches_plane_kernel_and_fp32))
            + list(test_wgrad_zring_shape_gpu.CASES)):
        base.append((n, *size, c0, c1, cout, 3, 3, 3, 1, 1, 1, pad, pad, pad))
    for n, c0, c1, cout, size in _parametrized(test_wgrad_zring_gpu.test_zring16_against_fp64):
        base.append((n, *size, c0, c1, cout, 3, 3, 3, 1, 1, 1, 1, 1, 1))
    for n, size, c0, cout, s, p in WGRAD_S2_SHAPES:
        base.append((n, *size, c0, 0, cout, 3, 3, 3, s, s, s, p, p, p))
    for n, size, (c0, c1), cout, (k, s, p) in itertools.product((1, 2), SIZES, CHANNELS, COUTS, KSP):
        base.append((n, *size, c0, c1, cout, *k, *s, *p))
    for n, size, (c0, c1), cout, (k, s, p) in itertools.product((1, 2), SIZES, WGRAD_SMALL_CHANNELS,
                                                                (16, 32), KSP):
        base.append((n, *size, c0, c1, cout, *k, *s, *p))
    return np.asarray([(sw, *r) for sw in range(len(WGRAD_SWITCHES)) for r in base], np.int32)


def wgrad_answers(wg, convt):
    """The library's weight-gradient answers: int64 [n, len(WGRAD_COLUMNS)] for the descriptors and
    [m] workspace bytes for the transposed-conv table."""
    from adell_mri_amd import _lib, ops

    L = _lib.lib()
    zr = (ctypes.c_int * 8)()
    out = (ctypes.c_int * 25)()
    a = np.zeros((len(wg), len(WGRAD_COLUMNS)), np.int64)
    for sw, name in enumerate(WGRAD_SWITCHES):
        with _lib.tuning(**({name: 1} if name else {})):
            for i in np.nonzero(wg[:, 0] == sw)[0]:
                r = [int(v) for v in wg[i]]
                d = ops.make_conv_desc(r[1], tuple(r[2:5]), r[5], r[6], r[7], tuple(r[8:11]),
                                       tuple(r[11:14]), tuple(r[14:17]))
                ref = ctypes.byref(d)
                a[i, 0] = L.adell_conv3d_bwd_weight_f16x3_workspace(ref)
                a[i, 1] = L.adell_conv3d_bwd_weight_workspace(ref)
                a[i, 2] = L.adell_conv3d_bwd_weight_f16x3_rows_ok(ref)
                zr[:] = [0] * 8
                a[i, 3] = L.adell_wgrad_zring_plan(*r[1:5], r[5], r[6], r[7], *r[8:14], d.Do, d.Ho,
                                                   d.Wo, zr)
                a[i, 4:12] = list(zr)
                rc = L.adell_conv3d_bwd_weight_f16x3_plan(ref, out)
                a[i, 12] = rc
                if rc == 0:
                    a[i, 13:] = list(out)
    t = np.asarray([L.adell_convtranspose3d_bwd_weight_workspace(*(int(v) for v in r[1:10]))
                    for r in convt], np.int64)
    return a, t


def check_wgrad_coverage(wg, a, t):
    """What the weight-gradient grid must exercise, and that the queries agree with each other."""
    col = WGRAD_COLUMNS.index
    ok = a[:, col("plan_rc")] == 0
    route = a[:, col("route")]
    # (the f16x3 planner refuses nothing up to 7^3 taps; the fp32 one refuses 5^3 and wider)
    assert ((a[:, col("ws_fp32")] < 0) == (ok & (route != ROUTES["small"])
                                          & (a[:, col("fp32_maxj")] == 0))).all()
    assert (a[:, col("ws_fp32")] < 0).any(), "no fp32 refusal"
    assert set(route[ok].tolist()) == set(ROUTES.values()), sorted(set(route[ok].tolist()))
    plane = ok & (route == ROUTES["plane"])
    inst = {tuple(v) for v in a[plane][:, [col("MAXJ"), col("PFX"), col("PFY")]].tolist()}
    assert inst == F16_INSTANCES, sorted(inst ^ F16_INSTANCES)
    assert {2, 5, 7, 9} <= set(a[ok, col("fp32_maxj")].tolist())
    assert set(a[:, col("rows_ok")].tolist()) == {0, 1}
    # the query repeats the other entries' answers
    ws_q = a[:, col("ws_lo")] + (a[:, col("ws_hi")] << 31)
    assert (ws_q[ok] == a[ok, col("ws_f16x3")]).all() and (a[~ok, col("ws_f16x3")] < 0).all()
    assert (a[ok, col("rows_ok_q")] == a[ok, col("rows_ok")]).all()
    zring = ok & ((route == ROUTES["zring32"]) | (route == ROUTES["zring16"]))
    assert ((a[:, col("zr_rc")] == 1) == zring).all()
    assert (a[zring][:, col("q_zr0"):col("q_zr0") + 8] == a[zring][:, col("zr0"):col("zr0") + 8]).all()
    assert (t > 0).any()
    # the workspace rule: slabs for the larger of the route's regions and the per-plane plan's (the
    # same descriptor under wgrad_nozring), with both sides present
    n = len(wg) // len(WGRAD_SWITCHES)
    assert (wg[:n, 1:] == wg[n:2 * n, 1:]).all() and (wg[:n, 0] == 0).all() and (wg[n:2 * n, 0] == 1).all()
    fast = np.nonzero(ok[:n] & np.isin(route[:n], [ROUTES["zring32"], ROUTES["zring16"], ROUTES["s2"]]))[0]
    assert (route[n + fast] == ROUTES["plane"]).all()
    r_route, r_plane = a[fast, col("R")], np.where(ok[n + fast], a[n + fast, col("R")], 0)
    d = wg[fast].astype(np.int64)
    per_region = d[:, 8] * d[:, 9] * d[:, 10] * (d[:, 5] + d[:, 6]) * d[:, 7] + d[:, 7]
    assert (a[fast, col("ws_f16x3")] == (np.maximum(r_route, r_plane) * per_region + 4) * 4).all()
    assert (r_route > r_plane).any() and (r_plane > r_route).any()
    for s in (ROUTES["zring32"], ROUTES["zring16"], ROUTES["s2"]):
        assert (route[fast] == s).any()


def check_coverage(a, t):
    """What the grid must exercise for the file to pin the planner."""
    col = ANSWER_COLUMNS.index
    for d in ("fwd", "bwd"):
        ok = a[:, col(d + "_rc")] == 0
        cfgs = set(a[ok, col(d + "_cfg")].tolist())
        assert {0, 1, 2, 3, 4, 6, 8} <= cfgs, (d, sorted(cfgs))
        assert (a[ok, col(d + "_shares")] > 1).any(), f"{d}: no split-K plan"
    assert (a[:, col("fwd_rc")] != 0).any(), "no refusal"
    assert 5 in set(t[t[:, 0] == 0, 1].tolist()), "no cfg 5 in the transposed grid"
    assert set(a[:, col("rows_ok")].tolist()) == {0, 1}
    assert (a[:, col("adn_ntiles")] == 0).any() and (a[:, col("adn_ntiles")] > 0).any()
    assert (a[:, col("ntiles")] != a[:, col("ntiles_ws")]).any()


def wgrad_main():
    _, convt = grid()
    wg = wgrad_grid()
    a, t = wgrad_answers(wg, convt)
    check_wgrad_coverage(wg, a, t)
    # (the two big tables are stored column by column: a quarter of the row-major file's size)
    np.savez_compressed(WGRAD_GOLDEN, wgrad=np.ascontiguousarray(wg.T),
                        wgrad_answers=np.ascontiguousarray(a.T), convt=convt, convt_workspace=t)
    from adell_mri_amd import _lib
    print(f"{len(wg)} weight-gradient + {len(convt)} transposed-conv descriptors from {_lib.LIB_PATH} "
          f"-> {os.path.relpath(WGRAD_GOLDEN, ROOT)} ({os.path.getsize(WGRAD_GOLDEN)} bytes)")


def main():
    if sys.argv[1:] == ["wgrad"]:
        return wgrad_main()
    conv, convt = grid()
    a, t = answers(conv, convt)
    check_coverage(a, t)
    np.savez_compressed(GOLDEN, conv=conv, conv_answers=a, convt=convt, convt_answers=t)
    from adell_mri_amd import _lib
    print(f"{len(conv)} conv + {len(convt)} transposed-conv descriptors from {_lib.LIB_PATH} -> "
          f"{os.path.relpath(GOLDEN, ROOT)} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
