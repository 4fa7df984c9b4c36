"""The share hint of the z-ring weight gradient (adell_wgrad_zring_share_plan, host only): where the
library takes it, the dynamic LDS an accepted launch requests -- two such blocks must not fit a CU,
one of them and the largest specialised implicit-GEMM block must -- and that no hint touches the
plan itself. No GPU needed."""
import ctypes

import pytest

from adell_mri_amd import _lib, ops

LDS_PER_CU = 160 * 1024      # gfx950
NONE, AUTO, ALWAYS = 0, 1, 2

# N, C0, C1, Cout, size: what the z-ring does with it, whether AUTO / ALWAYS are accepted
CASES = [
    (2, 32, 0, 32, (128, 128, 128), "zring32", True, True),    # 512 blocks, 128 planes each
    (2, 64, 0, 64, (128, 128, 128), "zring32", True, True),    # 128 regions x 4 channel tiles
    (2, 32, 32, 64, (128, 128, 128), "zring32", True, True),   # the concat conv of a decoder level
    (2, 32, 32, 32, (128, 128, 128), "zring32", True, True),
    (2, 64, 0, 64, (64, 64, 64), "zring32", False, True),      # 512 blocks of 64 planes: too short
    (2, 32, 32, 64, (64, 64, 64), "zring32", False, True),
    (1, 32, 0, 32, (128, 128, 128), "zring32", False, True),   # two 64-plane segments per column
    (1, 32, 0, 32, (32, 32, 32), "zring32", False, True),      # 128 blocks: one to a CU anyway
    (1, 32, 0, 32, (100, 32, 32), "zring32", False, True),     # long columns, 16 blocks
    (1, 32, 0, 32, (6, 16, 24), "zring32", False, True),       # six blocks
    (2, 16, 0, 16, (128, 128, 128), "zring16", False, False),  # a 16-channel layer: the 16 x 16 form
    (2, 32, 0, 16, (64, 64, 64), "zring16", False, False),
    (1, 32, 0, 32, (8, 6, 6), None, False, False),             # a plane too small for the z-ring
    (2, 32, 0, 32, (2, 64, 64), None, False, False),           # too few planes
]


def _plan(case, share):
    N, C0, C1, Cout, size = case[:5]
    return ops.conv3d_bwd_weight_share_plan(N, size, C0, C1, Cout, 3, 1, 1, share)


def _zring_plan(case):
    N, C0, C1, Cout, size = case[:5]
    out = (ctypes.c_int * 8)()
    D, H, W = size
    if not _lib.lib().adell_wgrad_zring_plan(N, D, H, W, C0, C1, Cout, 3, 3, 3, 1, 1, 1, D, H, W, out):
        return None
    return tuple(out)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}x({c[1]}+{c[2]})->{c[3]}@{c[4]}")
def test_where_the_hint_is_taken(case):
    N, C0, C1, Cout, size, route, auto, always = case
    w = ops.conv3d_bwd_weight_plan(N, size, C0, C1, Cout, 3, 1, 1)
    assert (w.route if w.route.startswith("zring") else None) == route
    plain = _plan(case, NONE)
    if route is None:
        assert plain is None and _plan(case, AUTO) is None and _plan(case, ALWAYS) is None
        return
    # no hint: the plan of adell_wgrad_zring_plan, the kernel's own LDS, two (three) blocks per CU
    assert plain.zring == _zring_plan(case) == w.zring
    assert plain.blocks_per_cu == (3 if route == "zring16" else 2)
    assert plain.blocks_per_cu * plain.lds <= LDS_PER_CU
    for share, taken in ((AUTO, auto), (ALWAYS, always)):
        p = _plan(case, share)
        assert p.zring == plain.zring, "a hint must not change regions, units or segments"
        if not taken:
            assert p == plain
            continue
        assert p.blocks_per_cu == 1
        assert p.lds >= plain.lds, "the kernel still needs its own LDS"
        assert 2 * p.lds > LDS_PER_CU, "two blocks must not fit a CU"
        assert p.room == LDS_PER_CU - p.lds - (-p.lds % 1280)    # (1280 B: the allocation unit)
        # the partner: the specialised implicit-GEMM instances at the same shape, forward and
        # backward-data (SPEC 3: 8x8x8 bricks, cfg 4; SPEC 1: 8x8x4 bricks, cfg 0 / 1)
        for bwd in (False, True):
            cin, cout = (Cout, C0 + C1) if bwd else (C0 + C1, Cout)
            for tune in ({}, {"igemm_no8": 1}):
                with _lib.tuning(**tune):
                    c = ops.conv3d_plan(N, size, cin, 0, cout, 3, 1, 1, backward_data=bwd)
                if auto:     # (the small ALWAYS-only shapes run smaller bricks)
                    assert c.cfg in (0, 1, 4), c
                assert p.lds + c.lds <= LDS_PER_CU, (c, p)
                assert c.lds <= p.room, (c, p)


def test_the_rule_has_both_sides():
    taken = [c for c in CASES if c[6]]
    refused = [c for c in CASES if c[5] == "zring32" and not c[6]]
    assert taken and refused and any(c[5] == "zring16" for c in CASES) and any(c[5] is None for c in CASES)


def test_the_partner_is_the_largest_specialised_plan():
    """78 400 B: the 8x8x8-brick instance; the request leaves that much, rounded up to the 1280-byte
    allocation unit, and no more than one unit of slack goes unused on either side."""
    p = _plan(CASES[0], AUTO)
    c = ops.conv3d_plan(2, (128, 128, 128), 32, 0, 32, 3, 1, 1)
    assert c.cfg == 4 and c.lds == 78400
    assert p.lds % 1280 == 0 and p.lds - LDS_PER_CU // 2 <= 1280
    assert p.room >= c.lds + (-c.lds % 1280)


def test_unknown_hints_are_refused_before_any_launch():
    d = ops.make_conv_desc(1, (6, 16, 24), 32, 0, 32, 3, 1, 1)
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    L = _lib.lib()
    assert L.adell_conv3d_bwd_weight_f16x3_share(ctypes.byref(d), p, None, p, p, None, None, None,
                                                 p, 64, None, 7) == _lib.E_BADARG
    assert b"hint" in L.adell_last_error()
    assert L.adell_conv3d_bwd_weight_f16x3_rows_share(ctypes.byref(d), p, p, None, None, p, p, None,
                                                      None, None, p, 64, None, -1) == _lib.E_BADARG


def test_a_hint_is_not_a_tuning_switch():
    L = _lib.lib()
    e0 = L.adell_plan_epoch()
    _plan(CASES[0], AUTO)
    _plan(CASES[0], ALWAYS)
    assert L.adell_plan_epoch() == e0
    assert L.adell_set_tuning(b"wgrad_share", 1) != _lib.OK     # no such switch
    assert L.adell_plan_epoch() == e0
