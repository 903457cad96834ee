"""Deterministic inputs for the event schedule of the bit-vector sweep (align_bitvec.h: bitvec_pass): paths that run along the
far edge of every superblock's window -- through the columns where the lane above has already closed -- and short pairs whose
lengths make several kinds of event (segment end, close, open, diagonal entry) fall on one step.  No GPU in here:
test_event_schedule_cpu.py proves from the oracle what each input is, test_gpu_event_schedule.py runs the kernels on them.

Windows and rings come from align_rings.py, i.e. from the constants of align_bitvec.h."""
import numpy as np

import align_rings as ar

HUG_R = 0.36
# ring -> length of the shorter side of the edge-hugging pairs: past the first ring wrap (64 superblocks of 32 NB rows), and
# with a max_dst (1 + int(m R)) whose first-pass window is the ring's own room: (w, wl) = (1384, 693) and (2728, 1365).
# R = 0.36 is small enough for the rows behind the gap (m - g / R of them, ~0.51 edits per row if the path stayed on the
# diagonal of two unrelated stretches) to cost more than the gap itself, so the planted path is the cheapest one.
HUG_M = {1: 6800, 2: 13400}


def hug_window(NB):
    md = ar.max_dst_of(HUG_M[NB], HUG_M[NB] + 1, HUG_R)
    assert ar.nb1(md) == NB
    return ar.first_window(md)


def hug_gaps(NB):
    w, wl = hug_window(NB)
    RB = 32 * NB
    return [w - RB - 1, w - RB, w - RB + 1, w - 1, w], [wl - 1, wl]


def hug_pairs(NB: int):
    """(certified batch, uncertified batch).  Deletions: the shorter side is its partner minus one block of g bases at row
    p = g / R + 2 (the first row at which the reference's check lets the diagonal cost g); from there the only cheap path
    runs g rows ahead of the columns, cost g <= w: along the last columns of each window for g = w - RB - 1 .. w.
    Insertions (the wl side): the shorter side carries g random bases at p1 that its partner lacks, and lacks g bases at p2;
    the path runs g columns ahead between the two and pays 2 g.  2 (wl - 1) <= w is certified, 2 wl > w is not (second batch)."""
    w, wl = hug_window(NB)
    m = HUG_M[NB]
    rng = np.random.RandomState(8100 + NB)
    dels, ins = hug_gaps(NB)
    ok, redo = ar.Batch(), ar.Batch()
    for k, g in enumerate(dels):
        p = int(g / HUG_R) + 2
        x = ar.rand_seq(rng, m + g)
        y = x[:p] + x[p + g:]
        a, b = (x, y) if k % 2 else (y, x)
        ok.add_pair(ok.place(rng, a, False, ar.MODS[k % 3]), ok.place(rng, b, False, ar.MODS[(k + 1) % 3]), False, False,
                    kind="del", g=g, p=p, m=m, a_rows=bool(k % 2), tag=f"hug{NB}:del{g}")
    for k, g in enumerate(ins):
        p2 = m - 300
        p1 = p2 - int(4.4 * g)                                    # staying on the diagonal between the two would cost ~2.2 g
        x = ar.rand_seq(rng, m + 60)                              # rows
        y = (x[:p1] + ar.rand_seq(rng, g) + x[p1:p2] + x[p2 + g:])[:m]     # columns: g extra bases at p1, g fewer at p2
        B = ok if 2 * g <= min(w, 2 * wl + 1) else redo
        a, b = (x, y) if k % 2 else (y, x)
        B.add_pair(B.place(rng, a, False, ar.MODS[k % 3]), B.place(rng, b, False, ar.MODS[(k + 2) % 3]), False, False,
                   kind="ins", g=g, p1=p1, p2=p2, m=m, a_rows=bool(k % 2), tag=f"hug{NB}:ins{g}")
    return ok, redo


# ----------------------------------------------------------------------------- coinciding events
COIN_R = 0.27      # every row of FAIL_ROWS can be the FIRST failing one: an integer c with c <= (f-1) R and c + 1 > f R exists
FAIL_ROWS = (11, 32, 33, 64, 65)


def coin_ms(NB):
    """shorter-side lengths: multiples of RB and of 32 and their neighbours, just above 10 (rows <= 10 are never checked), and
    lengths whose m + max_dst is a multiple of RB (the last superblock exactly full at n = m + w)"""
    RB = 32 * NB
    ms = {11, 12, 31, 32, 33, RB - 1, RB, RB + 1, 2 * RB - 1, 2 * RB, 2 * RB + 1, 4 * RB}
    for m in range(3 * RB, 7 * RB):
        if (m + ar.max_dst_of(m, m + 1, COIN_R)) % RB == 0:
            ms.add(m)
            break
    return sorted(ms)


def fail_at(rng, f, m, R=COIN_R):
    """two sequences of length m, equal up to base k and without a common base after it, so that cost(i, i) = i - k for i > k:
    the reference's check (cost > i R, rows above 10) fails first at row f"""
    c = int((f - 1) * R)
    k = f - 1 - c
    assert k >= 0 and m >= f and c + 1 > f * R
    x = ar.rand_seq(rng, k) + np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, m - k)].tobytes()
    y = x[:k] + np.frombuffer(b"GT", np.uint8)[rng.randint(0, 2, m - k)].tobytes()
    return x, y


def coin_pairs(NB: int) -> ar.Batch:
    """Short pairs, each in its whole band (w = max_dst): every m of coin_ms with n - m in {0, w, w + 40} as a true pair (2 % edits
    behind a clean head: it passes), and pairs that fail at rows 11, 32, 33, 64, 65 and in the first segment after the ring
    wrap (row 64 RB + 20), the failing row being the last row, the one before it, or well inside.  (m < w does not exist at
    R < 1: max_dst <= m.  The windows' "one event per step" regime at both ends is what the m <= RB pairs run in.)"""
    RB = 32 * NB
    rng = np.random.RandomState(8200 + NB)
    B = ar.Batch()
    for m in coin_ms(NB):
        md = ar.max_dst_of(m, m + 1, COIN_R)
        for extra in (0, md, md + 40):
            x = ar.rand_seq(rng, m)
            y = ar.fit(rng, ar.mutate(rng, x, 0.02, head=12), m + extra)
            a_longer = bool(rng.randint(2))
            a, b = (y, x) if a_longer else (x, y)
            B.add_pair(B.place(rng, a, False, ar.MODS[m % 3]), B.place(rng, b, False, ar.MODS[(m + 1) % 3]), False, False,
                       kind="true", m=m, extra=extra, tag=f"coin{NB}:m{m}+{extra}")
    for f in FAIL_ROWS + (64 * RB + 20,):
        for m in sorted({f, f + 1, max(f, 2 * RB), f + RB}):
            x, y = fail_at(rng, f, m)
            y = y + ar.rand_seq(rng, int(rng.randint(0, 3)) * 20)
            B.add_pair(B.place(rng, x, False, ar.MODS[f % 3]), B.place(rng, y, False, ar.MODS[(f + 1) % 3]), False, False,
                       kind="fail", f=f, m=m, tag=f"coin{NB}:fail{f}:m{m}")
    return B


def forced(NB, B):
    """ring 1 holds short pairs by themselves; ring 2 behind a pilot of the first max_dst of its plan row"""
    return B if NB == 1 else B.with_pilot(ar.pilot(ar.row_of(2, 2)[0], COIN_R))
