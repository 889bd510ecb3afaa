"""CPU model of the online LDS engine's layout chooser (lws_amd/csrc/lws_online.hip: shape_of, shape4_try / shape4_of, pick_layout),
next to the chooser as it was while the retired third layout (k_online3: shape3_of) still existed.  Shows that the two rules give
the same layout, lag, slots, ring and LDS size in every cell where the old rule did not answer 3, and prints the cells where it did
(docs/DESIGN_APPENDIX.md, Appendix B lists them).  L = 5 (the only stencil layouts 2 and 3 took), T = 500, no switches set.
usage: python tools/online_layout_model.py [--all]     (--all: every iteration count from 1 to 100 instead of 19 of them)"""
import sys

L, SKB, SKS, NW, LDS_MAX = 5, 8, 4, 16, 160 * 1024


def common(F, Q, n_thr):
    return (SKB * (Q - 1) + L + 3) // 2, F + 2 * L, n_thr + 1, (F + 1) // 2      # DS_MIN, Np, per, NU


def too_long(DS, T, per, NU):
    return DS * T * per + SKS * T + NU > 1.0e9


def shape2(F, T, Q, LA, n_thr):                      # -> (DS, NSW, threads, lds) or None
    DS_MIN, Np, per, NU = common(F, Q, n_thr)
    if LA + Q > NW:                                  # (a shortcut, here and below: the window is LA + Q frames at least)
        return None
    DS = next((d for d in range(DS_MIN, 4 * DS_MIN + 1) if ((NU - 1 + SKS * LA) // d + 2) * (LA + 1) * Q * 2 <= 1024), 0)
    if DS == 0:
        return None
    NSW = (NU - 1 + SKS * LA) // DS + 2
    threads = (NSW * (LA + 1) * Q * 2 + 63) // 64 * 64
    lds = (NW * Np + 2) * 8 + NW * Np * 4 + 8 + 3 * Q * Q * (L + 1) * 8 + Q * 8 + n_thr * 4
    if threads > 1024 or (DS * (per - 1) + NU) // (DS * per + SKS) + LA + Q > NW or lds > LDS_MAX or too_long(DS, T, per, NU):
        return None
    return DS, NSW, threads, lds


def shape3(F, T, Q, LA, n_thr):                      # the retired layout
    DS_MIN, Np, per, NU = common(F, Q, n_thr)
    if LA > 63 or LA + Q > NW:
        return None
    NSW = 64 // (LA + 1)
    DS = max(DS_MIN if 2 * DS_MIN >= SKB * Q + 2 else (SKB * Q + 3) // 2, (SKS * LA + NU + NSW - 1) // NSW)
    lds = 2 * (2 * Q - 1) * 64 * 16 + (192 + 64) * 8 + (NW * Np + 2) * 8 + NW * Np * 4 + 8 + 3 * Q * Q * (L + 1) * 8 + Q * 8 + n_thr * 4
    if (DS * (per - 1) + NU + 1) // (DS * per + SKS) + LA + Q > NW or F - 1 < 2 * (L + 3) or lds > LDS_MAX or too_long(DS, T, per, NU):
        return None
    return DS, NSW, (9 if Q == 4 else 2 * Q) * 64, lds


def shape4_try(F, T, Q, LA, n_thr, big, serial):
    DS_MIN, Np, per, NU = common(F, Q, n_thr)
    if LA > 63 or F - 1 < 2 * (L + 3) or LA + Q > 16:
        return None
    NSW = 64 // (LA + 1)
    DS = max(DS_MIN if 2 * DS_MIN >= SKB * Q + 2 else (SKB * Q + 3) // 2, (SKS * LA + NU + 2 + NSW - 1) // NSW)
    if not (Q in (2, 4) and not serial):
        DS += DS & 1
    NPS = Np + (Np & 1)
    lds_of = lambda nwr: (2 * (2 * Q - 1) * 64 * 16 + (224 + 64) * 8 + (nwr * NPS + 8) * 8 + (0 if big else nwr * NPS * 4) +
                          3 * Q * Q * (L + 1) * 8 + Q * 8 + n_thr * 4 + 16 + (0 if big else NU * 16))
    nwr_max = 16
    while nwr_max > 0 and lds_of(nwr_max) > LDS_MAX:
        nwr_max -= 1
    window_of = lambda ds: (ds * (per - 1) + NU + 3) // (ds * per + SKS) + LA + Q
    DS0 = DS
    while window_of(DS) > nwr_max and DS < 16 * DS0:
        DS += 2
    window = window_of(DS)
    if window > nwr_max:
        return None
    NWR = window + 1 if window + 1 <= nwr_max else window
    if NWR == window + 1 and lds_of(window + 1) > 80 * 1024 and lds_of(window) <= 80 * 1024:
        NWR = window
    return None if too_long(DS, T, per, NU) else (DS, NSW, 2 * Q * 64, lds_of(NWR), NWR, NPS, big)


def shape4(F, T, Q, LA, n_thr, serial):
    r = shape4_try(F, T, Q, LA, n_thr, False, serial)
    return r if r or serial else shape4_try(F, T, Q, LA, n_thr, True, serial)


def pick_old(s2, s3, s4):
    if s4 and (not s2 or 2 * s4[0] <= 3 * s2[0]): return 4, s4
    if s3 and (not s2 or 2 * s3[0] <= 3 * s2[0]): return 3, s3
    return (2, s2) if s2 else (0, None)


def pick_new(s2, s4):
    if s4 and (not s2 or 2 * s4[0] <= 3 * s2[0]): return 4, s4
    return (2, s2) if s2 else (0, None)


if __name__ == "__main__":
    sizes = sorted(set(range(16, 1601, 4)) | set(range(1600, 4401, 100)) | {2048, 4096})
    ITERS = range(1, 101) if "--all" in sys.argv else [*range(1, 13), 16, 20, 25, 32, 50, 64, 100]   # (--all: two minutes)
    cells = differ = 0
    sliver = {}
    for serial in (False, True):
        for Q in (2, 4, 8):
            for N in sizes:
                for LA in range(64):
                    for it in ITERS:
                        F = N // 2 + 1
                        s2, s3, s4 = shape2(F, 500, Q, LA, it), shape3(F, 500, Q, LA, it), shape4(F, 500, Q, LA, it, serial)
                        old, new = pick_old(s2, s3, s4), pick_new(s2, s4)
                        cells += 1
                        if old[0] == 3:
                            sliver.setdefault((serial, Q, N, LA, s3[0], s4[0] if s4 else None, new[0], new[1][0] if new[1] else None), []).append(it)
                        elif old != new:
                            differ += 1
    print(f"{cells} cells; old rule != 3 and new rule differs: {differ}; old rule == 3: {sum(len(v) for v in sliver.values())}")
    for (serial, Q, N, LA, d3, d4, lay, d), its in sorted(sliver.items()):
        print(f"  serial={int(serial)} Q={Q} N={N} LA={LA}: lag {d3} on layout 3, {d4} on layout 4 -> now layout {lay}, lag {d}; iterations {its[0]}..{its[-1]} ({len(its)})")
    sys.exit(1 if differ or any(k[6] == 0 for k in sliver) else 0)
