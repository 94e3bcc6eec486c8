#!/usr/bin/env python3
"""LDS banks of the exchange buffer of the F(6x6) output stage (csrc/b2f_wino6.hip, wino6_output), lane by lane, on the CPU.

    python tools/wino6_banks.py            # both forms, every instruction of a pass

The exchange buffer holds planes X[a 8][j 6] of XPS bytes, a plane = [tile 16][32 outputs]: the 16-byte unit of output quad q of tile t
sits at t * 128 + (q ^ (t & 7)) * 16.  Every access moves one 8-byte half of a unit:
  * the dump (ds_write_b64): lane (tile t = lane & 15, q4 = lane >> 4) of wave a writes half hf of quad 4 mtp + q4 to the planes (a, j = 0..5);
  * a round (ds_read_b64): item idx = (tid & 255) + 256 rr = (quad, x parity, ...) reads half k of the unit of its pixel x of tile row tyy from
    the planes (a = 1..6 and 0 or 7, j = x % 6) of tile 8 tyy + x / 6.
Banking (MI355X): ds_read_b64 is served in two groups of 32 lanes over 64 banks of 4 bytes, ds_write_b64 in four groups of 16 lanes over 32
banks; distinct addresses on one bank inside a group take one LDS cycle each.

Forms:
  plain    (the kernel's first version) half hf of a unit at byte 8 hf; items (quad = idx & 7, xl = (idx >> 3) & 1, mm = idx >> 4), tile row
           mm / 24, x = 2 (mm % 24) + xl.  Pixels x and x + 2 of a 32-lane read group lie 2 XPS = 0 (mod 256) bytes apart, or in the next
           tile with the same effect: the same banks, while the banks of the other halves idle -- 2-way on every read.  Tiles t and
           t + 8 of a 16-lane write group hit the same banks: 2-way on every write.
  rows     (shipped) half hf of a unit of tile t at byte 8 (hf ^ (t >> 3)): tiles t and t + 8 of a write group move different halves.
           Items (quad = idx & 7, xl = (idx >> 3) & 1, tyy = (idx >> 4) & 1, x2 = idx >> 5), x = 2 x2 + xl: a 32-lane read group is the pixel
           pair (x, x + 1) -- XPS = 128 (mod 256) apart -- in BOTH tile rows, tiles t and t + 8, whose halves are swapped.  No conflicts in
           either direction, and every lane still gets half k in step k.
"""
import sys

XPS = 2176


def unit_offset(t, q):
    return t * 128 + ((q ^ (t & 7)) * 16)


def write_addresses(form, wave, mtp, hf, j):
    """byte address of every lane of one ds_write_b64 of the dump"""
    out = []
    for lane in range(64):
        t, q4 = lane & 15, lane >> 4
        half = hf ^ (t >> 3) if form == "rows" else hf
        out.append((wave * 6 + j) * XPS + unit_offset(t, mtp * 4 + q4) + 8 * half)
    return out


def item(form, tid, rr):
    """(quad, pixel x of the 48-wide row, tile row) of a thread's item of round rr"""
    idx = (tid & 255) + 256 * rr
    quad, xl = idx & 7, (idx >> 3) & 1
    if form == "rows":
        tyy, x2 = (idx >> 4) & 1, idx >> 5
    else:
        mm = idx >> 4
        tyy = 1 if mm >= 24 else 0
        x2 = mm - 24 * tyy
    return quad, 2 * x2 + xl, tyy


def read_addresses(form, wave, rr, k, a):
    """byte address of every lane of the ds_read_b64 of half k, plane row a, round rr"""
    out = []
    for lane in range(64):
        quad, x, tyy = item(form, wave * 64 + lane, rr)
        tile = tyy * 8 + x // 6
        half = k ^ tyy if form == "rows" else k
        out.append((a * 6 + x % 6) * XPS + unit_offset(tile, quad) + 8 * half)
    return out


def degree(addrs, group, nbanks):
    """largest number of distinct 8-byte addresses on one bank inside a lane group"""
    worst = 1
    for g in range(0, 64, group):
        banks = {}
        for a in addrs[g:g + group]:
            for b in ((a // 4) % nbanks, (a // 4 + 1) % nbanks):
                banks.setdefault(b, set()).add(a)
        worst = max(worst, max(len(v) for v in banks.values()))
    return worst


def worst_degrees(form):
    """(reads, writes): the worst conflict degree over every instruction of a pass -- both parities, all rounds, waves and planes"""
    rd = wr = 1
    for wave in range(8):
        for rr in range(3):
            for k in range(2):
                for a in range(8):
                    rd = max(rd, degree(read_addresses(form, wave, rr, k, a), 32, 64))
        for mtp in range(2):
            for hf in range(2):
                for j in range(6):
                    wr = max(wr, degree(write_addresses(form, wave, mtp, hf, j), 16, 32))
    return rd, wr


def roundtrip_ok(form):
    """a round reads half k of (plane, tile, quad) where the dump wrote it, and the items of a parity cover every (quad, pixel, tile row) once"""
    where = {}
    for wave in range(8):
        for mtp in range(2):
            for hf in range(2):
                for j in range(6):
                    for lane, ad in enumerate(write_addresses(form, wave, mtp, hf, j)):
                        if ad in where:
                            return False
                        where[ad] = (wave, j, lane & 15, mtp * 4 + (lane >> 4), hf)
    for par in range(2):
        items = set()
        for wave in range(4 * par, 4 * par + 4):
            for rr in range(3):
                for lane in range(64):
                    items.add(item(form, wave * 64 + lane, rr))
                for k in range(2):
                    for a in range(8):
                        for lane, ad in enumerate(read_addresses(form, wave, rr, k, a)):
                            quad, x, tyy = item(form, wave * 64 + lane, rr)
                            if where.get(ad) != (a, x % 6, tyy * 8 + x // 6, quad, k):
                                return False
        if items != {(q, x, ty) for q in range(8) for x in range(48) for ty in range(2)}:
            return False
    return True


if __name__ == "__main__":
    for form in sys.argv[1:] or ("plain", "rows"):
        rd, wr = worst_degrees(form)
        print("%-8s ds_read_b64 (32 lanes, 64 banks): %d-way   ds_write_b64 (16 lanes, 32 banks): %d-way   round trip %s"
              % (form, rd, wr, "ok" if roundtrip_ok(form) else "BROKEN"))
