"""Deterministic inputs for the shifted form of the score-only sweep (align_bitvec.h: bitvec_pass with SHIFT, csrc/lane_shift.h):
lane k holds superblock s_cl + k, and every close moves the lanes' state one lane up.  No GPU and no oracle in here: the CPU
file (test_lane_shift_inputs_cpu.py) proves what each input is planted for, the GPU file (test_gpu_lane_shift.py) runs it.

  wrap_batch      true pairs whose longer side has 64 RB - 1, 64 RB, 64 RB + 1, 65 RB + 1 and 128 RB + 1 rows (the first close
                  with a refill, the second revolution of the columns), the shorter side shorter by 0, 1, w - 1, w and w + 40
                  (w: the window's wide side, towards the free end); either sequence is the longer one
  seg_batch       pairs over {A, C} with a burst of G / T in one of them: every G / T costs one edit whatever the path does, so
                  the first failing diagonal row is known without a matrix.  It lies in the 32-row segment whose end the
                  schedule judges one step before, at, and one step behind the close of superblock 0, 63 and 64 -- the
                  read of the segment's word from "the lane of superblock s" across a move of the lanes
  alias_batch     m = 66 RB + 24: the free end's minimum planted from row m down into the last superblock, after 60 closes
  stale_batch     32 long and short pairs, for 640 repetitions through every wavefront
  driver_case     a reference and reads for k_locate and the spaced round"""
import numpy as np

import align_rings as ar
from diag_collect_inputs import hug_pair

WRAP_R = 0.06
SEG_R = 0.05
ALIAS_R = 0.05
DRIVER_R = 0.12


def wrap_rows(NB):
    RB = 32 * NB
    return (64 * RB - 1, 64 * RB, 64 * RB + 1, 65 * RB + 1, 128 * RB + 1)


def wide_side(m, n, R, NB):
    return ar.bv_pass1_w(ar.max_dst_of(m, n, R), NB)


def short_side(n, R, NB, off):
    """the longest m <= n with n - m >= w(m) + off, w the wide side of the pair's own first window"""
    m = n
    while n - m < wide_side(m, n, R, NB) + off:
        m -= 1
    return m


def subs_copy(rng, x: bytes, e: float, head: int = 60) -> bytes:
    """a copy of x with substitutions at rate e behind a clean head: the diagonal's cost is their count"""
    y = bytearray(x)
    for k in np.nonzero(rng.rand(len(x)) < e)[0]:
        if k >= head:
            y[k] = ar.ALPHA[(int(np.searchsorted(ar.ALPHA, x[k])) + 1 + rng.randint(3)) % 4]
    return bytes(y)


def wrap_batch(NB) -> ar.Batch:
    rng = np.random.RandomState(9300 + NB)
    B = ar.Batch()
    k = 0
    for n in wrap_rows(NB):
        for name, m in (("0", n), ("1", n - 1), ("w-1", short_side(n, WRAP_R, NB, -1)), ("w", short_side(n, WRAP_R, NB, 0)),
                        ("w+40", short_side(n, WRAP_R, NB, 40))):
            x = ar.rand_seq(rng, m)
            y = ar.fit(rng, subs_copy(rng, x, WRAP_R / 3), n)
            a_longer = k % 2 == 1
            a, b = (y, x) if a_longer else (x, y)
            B.add_pair(B.place(rng, a, False, ar.MODS[k % 3]), B.place(rng, b, False, ar.MODS[(k + 1) % 3]), False, False,
                       kind="true", rows=n, m=m, delta=name, a_longer=a_longer, tag=f"wrap{NB}:{n}-{name}")
            k += 1
    return B


# ----------------------------------------------------------------------------- a failing row next to a close
SEG_CLOSES = (0, 63, 64)
SEG_DD = (-1, 0, 1)


def t_seg(i, RB):
    return i + (i - 1) // RB + 1


def t_close(c, m, w_narrow, RB):
    return min(m, c * RB + RB + w_narrow) + c + 1


def first_fail(p, R):
    """first row whose diagonal cell fails when rows p + 1, p + 2, .. cost one edit each and the rows before them none"""
    j = 1
    while not (float(j) > float(p + j) * R and p + j > 10):
        j += 1
    return p + j, j


def seg_case(NB, c, dd):
    """(m, i, f, p, k): a shorter side m whose max_dst puts the end of the segment of rows i - 31 .. i at step close(c) + dd
    in ring NB, a failing row f inside that segment, and the burst y[p : p + k] that makes it the first one"""
    RB = 32 * NB
    for md in range(200, 420):
        m = int(np.ceil((md - 1) / SEG_R))
        while ar.max_dst_of(m, m + 1, SEG_R) < md:
            m += 1
        if ar.max_dst_of(m, m + 1, SEG_R) != md:
            continue
        wn = ar.bv_pass1_wl(md, NB)
        tc = t_close(c, m, wn, RB)
        for i in range(32, m - 64, 32):
            if t_seg(i, RB) == tc + dd:
                for p in range(i - 31 - 400, i):
                    f, j = first_fail(p, SEG_R)
                    if i - 24 <= f <= i - 6:
                        return m, i, f, p, j + 2
    raise AssertionError((NB, c, dd))


def seg_batch(NB) -> ar.Batch:
    rng = np.random.RandomState(9320 + NB)
    AC, GT = np.frombuffer(b"AC", np.uint8), np.frombuffer(b"GT", np.uint8)
    B = ar.Batch()
    k = 0
    for c in SEG_CLOSES:
        for dd in SEG_DD:
            m, i, f, p, kb = seg_case(NB, c, dd)
            x = AC[rng.randint(0, 2, m)].tobytes()
            y = x[:p] + GT[rng.randint(0, 2, kb)].tobytes() + x[p + kb:] + AC[rng.randint(0, 2, 12)].tobytes()
            a_longer = k % 2 == 1
            a, b = (y, x) if a_longer else (x, y)
            B.add_pair(B.place(rng, a, False, ar.MODS[k % 3]), B.place(rng, b, False, ar.MODS[(k + 1) % 3]), False, False,
                       kind="fail", m=m, seg_end=i, f=f, close=c, dd=dd, tag=f"seg{NB}:close{c}{dd:+d}:row{f}")
            k += 1
    return B


# ----------------------------------------------------------------------------- fin words found by column
def alias_m(NB):
    return 66 * 32 * NB + 24


def alias_batch(NB) -> ar.Batch:
    """the longer side is the shorter one with d bases inserted at even spacing behind a clean head, so the free end's first
    minimum lies about d rows below m; then a random tail up to n = m + delta.  Where the minimum falls is the oracle's to say."""
    rng = np.random.RandomState(9340 + NB)
    m = alias_m(NB)
    md = ar.max_dst_of(m, m + 1, ALIAS_R)
    B = ar.Batch()
    k = 0
    for d in (0, 1, md // 3, 2 * md // 3, md - 8):
        x = ar.rand_seq(rng, m)
        y = bytearray(x)
        for q in range(d):
            at = 40 + (q * (m - 60)) // max(d, 1) + q
            y[at:at] = bytes([ar.ALPHA[rng.randint(4)]])
        y = bytes(y)
        for delta in sorted({0, 1, md - 1, md, md + 40, d, d + 1}):
            b = ar.fit(rng, y, m + delta)
            a_, b_ = (b, x) if k % 2 else (x, b)
            B.add_pair(B.place(rng, a_, False, ar.MODS[k % 3]), B.place(rng, b_, False, ar.MODS[(k + 1) % 3]), False, False,
                       kind="alias", d=d, delta=delta, tag=f"alias{NB}:d{d}+{delta}")
            k += 1
    return B


# ----------------------------------------------------------------------------- every wavefront, many times
def stale_batch(NB, R) -> ar.Batch:
    """32 distinct pairs, long (300 .. 424: a dozen closes in ring 1, half a dozen in ring 2) and short (31 .. 65) in turn, true
    ones and strangers"""
    rng = np.random.RandomState(9360 + NB)
    B = ar.Batch()
    for k in range(32):
        m = (300 + 4 * k) if k % 2 == 0 else (31, 32, 33, 63, 64, 65)[(k // 2) % 6]
        if k % 8 < 6:
            x, y = hug_pair(rng, m, R, m)
            kind = "true"
        else:
            x, y = ar.rand_seq(rng, m), ar.rand_seq(rng, m)
            kind = "fail"
        tail = (0, 1, ar.max_dst_of(m, m + 1, R) - 1, ar.max_dst_of(m, m + 1, R) + 9)[k % 4]
        B.add_pair(B.place(rng, x, False, ar.MODS[k % 3]), B.place(rng, y + ar.rand_seq(rng, tail), False, ar.MODS[(k + 1) % 3]),
                   False, False, kind=kind, m=m, tag=f"shifted{NB}:{k}:m{m}:{kind}")
    return B


# ----------------------------------------------------------------------------- the drivers
def driver_ms(NB):
    RB = 32 * NB
    return (63, 64, 65, 129, 300, 301, 64 * RB - 1, 64 * RB + 1, 65 * RB + 1)


def driver_case(NB):
    """A reference that holds, between spacers, the longer sides of true pairs (the read, substitutions only, and max_dst more
    bases) and of strangers that share only a 24-base head with their read; the shorter sides are the reads.  Ring 2 behind
    an unrelated filler read that sizes the plan."""
    R = DRIVER_R
    rng = np.random.RandomState(9380 + NB)
    parts, reads, meta = [ar.rand_seq(rng, 200)], [], []

    def plant(x, y, **m):
        pos = sum(len(p) for p in parts)
        parts.extend([y, ar.rand_seq(rng, 150)])
        reads.append(x)
        meta.append(dict(pos=pos, **m))

    for m in driver_ms(NB):
        x, y = hug_pair(rng, m, R, m)
        plant(x, y + ar.rand_seq(rng, ar.max_dst_of(m, m + 1, R)), kind="true", m=m)
    for m in (160, 161, 420, 2100):
        x = ar.rand_seq(rng, m)
        plant(x, x[:24] + ar.rand_seq(rng, m + 6), kind="fail", m=m)
    if NB == 2:
        reads.append(ar.pilot(ar.row_of(2, 2)[0], R, seed=5)[0])
        meta.append(dict(kind="filler"))
    return np.frombuffer(b"".join(parts), np.uint8), reads, meta
