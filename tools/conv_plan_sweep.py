#!/usr/bin/env python3
"""Dense pin of the f16x3 conv launch planner (csrc/conv3d.hip adell_plan_f16): the answers of the
host-only query entries over a fixed grid of descriptors.

    python tools/conv_plan_sweep.py        -> tests/golden/conv_f16x3_plan_sweep.npz

Per conv descriptor (ANSWER_COLUMNS): adell_conv3d_f16x3_plan forward and backward-data,
adell_conv3d_splitk_workspace in both directions, adell_conv3d_fwd_ntiles_f16x3 and its _ws form,
adell_conv3d_f16x3_rows_ok and adell_conv3d_bwd_data_f16x3_adn_ntiles; per transposed-conv
descriptor adell_convtranspose3d_f16x3_plan. The grid holds the conv cases of tests/test_conv_plans.py,
the case lists of tests/test_adn_fused_gpu.py and tests/test_split_rows_gpu.py, a product of batch
sizes, volumes, channel counts and (kernel, stride, padding) triples, and the 3^3 stride-1 part of
that product again under each launch-plan switch.

No GPU is needed and the planner reads no device property, so the file is the same on the build
host and on the MI355X. The script uses the C ABI only, and ADELL_HIP_LIBRARY selects the library:
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


def main():
    conv, convt = grid()
    a, t = answers(conv, convt)
    check_coverage(a, t)
    np.savez_compressed(GOLDEN, conv=conv, conv_answers=a, convt=convt, convt_answers=t)
    from adell_mri_amd import _lib
    print(f"{len(conv)} conv + {len(convt)} transposed-conv descriptors from {_lib.LIB_PATH} -> "
          f"{os.path.relpath(GOLDEN, ROOT)} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
