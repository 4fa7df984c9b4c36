"""Bank check of the z-ring weight gradient's LDS images (conv_wgrad_zring.hip, 32 x 32 tile form) on
the CPU: every transposed fragment read (ds_read_b64_tr_b16: two 32-lane halves, bank = (byte / 4)
mod 64) of every (tap, k-step, channel half, hi | lo, first | second read) for the input images,
and of every k-step for the dY images, must touch 64 different banks per half. The staging stores
(ds_write_b64: four groups of 16 lanes, bank = (byte / 4) mod 32) are counted for the record.
usage: zring_lds_banks.py"""
HX, HV = 10, 100
XIMG, YIMG = HV * 32 + 64, 8 * 320 + 64
GY = (0, 2, 1, 3)      # brick row of the k-block that lane group g takes


def xrow(hy, hx):
    return (hy * HX + hx) * 32


def yrow(y, x):
    return (y * HX + x) * 32


def read_conflicts(addr_of_lane):
    worst = 1
    for half in range(2):
        banks = {}
        for lane in range(32 * half, 32 * half + 32):
            a = addr_of_lane(lane)
            assert a % 8 == 0
            for d in (0, 1):
                banks.setdefault((a // 4 + d) % 64, set()).add(a + 4 * d)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


worst_x = worst_y = 1
for tap in range(27):
    ky, kx = (tap % 9) // 3, tap % 3
    for s in range(2):
        for img in range(4):                 # [hi | lo][channel half]: a constant offset
            for second in range(2):
                def addr(lane):
                    g, tq, tp = lane >> 4, (lane >> 2) & 3, lane & 3
                    return img * XIMG + xrow(GY[g] + ky, tq + kx) + tp * 8 + s * 4 * HX * 32 + second * 128
                worst_x = max(worst_x, read_conflicts(addr))
for s in range(2):
    for img in range(4):
        for second in range(2):
            def addr(lane):
                g, tq, tp = lane >> 4, (lane >> 2) & 3, lane & 3
                return img * YIMG + yrow(GY[g], tq) + tp * 8 + s * 4 * HX * 32 + second * 128
            worst_y = max(worst_y, read_conflicts(addr))
print(f"transposed reads: input images worst {worst_x}-way, dY images worst {worst_y}-way (1 = conflict-free)")
assert worst_x == 1 and worst_y == 1

# staging stores, fp32 path: thread tid stores 8 bytes (hi; lo the same at a constant offset) of piece
# c4 = tid & 7 of row tid / 8 + 32 u
hist = {}
for u in range(4):
    for grp in range(16):                    # 16-lane groups of the 256 threads
        banks = {}
        for tid in range(16 * grp, 16 * grp + 16):
            c4, hv = tid & 7, (tid >> 3) + 32 * u
            if hv >= HV:
                continue
            a = (c4 >> 2) * XIMG + (c4 & 3) * 8 + xrow(hv // HX, hv % HX)
            for d in (0, 1):
                banks.setdefault((a // 4 + d) % 32, set()).add(a + 4 * d)
        if banks:
            w = max(len(v) for v in banks.values())
            hist[w] = hist.get(w, 0) + 1
print("input staging stores (ds_write_b64, per 16-lane group), ways -> groups:", dict(sorted(hist.items())))
hist = {}
for u in range(2):
    for grp in range(16):
        banks = {}
        for tid in range(16 * grp, 16 * grp + 16):
            c4, v = tid & 7, (tid >> 3) + 32 * u
            a = (c4 >> 2) * YIMG + (c4 & 3) * 8 + yrow(v >> 3, v & 7)
            for d in (0, 1):
                banks.setdefault((a // 4 + d) % 32, set()).add(a + 4 * d)
        w = max(len(v) for v in banks.values())
        hist[w] = hist.get(w, 0) + 1
print("dY staging stores, ways -> groups:", dict(sorted(hist.items())))
