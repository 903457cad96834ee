"""Inputs of tests/test_gpu_schedule_folds.py: the shapes at which the two folded events of the bit-vector sweep's schedule
(align_bitvec.h: the hand-off's end in the close event -- `live` --, the diagonal's entry in the segment end in front of it --
the 64-bit `one`) can go wrong.  From the constants of align_bitvec.h (tests/align_rings.py) alone; test_schedule_folds_cpu.py
proves from the oracle that every pair is what it is named for."""
import functools

import numpy as np

import align_rings as ar

FOLD_R = 0.30
FAIL_RS = (0.27, 0.29, 0.31, 0.33, 0.25, 0.23)       # a row can be a FIRST failing one under at least one of them
RING_ROW = {1: (1, 1), 2: (2, 2), 3: (3, 4)}         # the plan row whose narrow launch runs in the ring
BURST_TAIL = 70                                      # clean rows behind a burst that is not the pair's end


def forced(NB, B, R):
    """ring 1 holds short pairs by themselves; the others behind a pilot of the first max_dst of their plan row"""
    return B if NB == 1 else B.with_pilot(ar.pilot(ar.row_of(*RING_ROW[NB])[0], R))


def geometry(NB, la, lb, R=FOLD_R):
    """(m, n, w, nr, S) of the narrow sweep of a pair in ring NB (align_bitvec: rows = the longer side, down to m + w)"""
    m, n = min(la, lb), max(la, lb)
    w = ar.bv_pass1_w(ar.max_dst_of(la, lb, R), NB)
    nr = min(n, m + w)
    return m, n, w, nr, (nr + 32 * NB - 1) // (32 * NB)


def true_pair(rng, m, extra, e=0.05):
    """x of m bases and a copy at error rate e cut or filled to m + extra: (shorter, longer)"""
    x = ar.rand_seq(rng, m)
    return x, ar.fit(rng, ar.mutate(rng, x, e, head=12), m + extra)


def add(B, rng, short, long, a_longer, **meta):
    a, b = (long, short) if a_longer else (short, long)
    k = len(B.pairs)
    B.add_pair(B.place(rng, a, False, ar.MODS[k % 3]), B.place(rng, b, False, ar.MODS[(k + 1) % 3]), False, False, a_rows=a_longer, **meta)


# ----------------------------------------------------------------------------- 1 + 4: m at the superblock edges, the last column
def edge_ms(NB):
    RB = 32 * NB
    return (RB - 1, RB, RB + 1, 2 * RB, 2 * RB + 1, 64 * RB, 64 * RB + 1, 65 * RB + 1)


@functools.lru_cache(maxsize=None)
def edge_pairs(NB):
    """every m of edge_ms as a true pair at 5 % error with n - m = 0, 1 and w (the sweep's nr - m: the superblocks at and below
    row m close on the last column, alone, with one row below it, and over the whole window), the longer side as a and as b"""
    rng = np.random.RandomState(8300 + NB)
    B = ar.Batch()
    for m in edge_ms(NB):
        w = ar.bv_pass1_w(ar.max_dst_of(m, m + 1, FOLD_R), NB)
        for extra in (0, 1, w):
            for a_longer in (False, True):
                s, l = true_pair(rng, m, extra)
                add(B, rng, s, l, a_longer, kind="true", m=m, extra=extra, tag=f"fold{NB}:m{m}+{extra}:{'a' if a_longer else 'b'}")
    return B


# ----------------------------------------------------------------------------- 2: first failing rows around a fold
def burst_rows(NB):
    """the row just before and just after a superblock edge, and rows of the first segment behind it: at the first edge, the
    second, and the ring's wrap"""
    RB = 32 * NB
    return tuple(sorted({e + d for e in (RB, 2 * RB, 64 * RB) for d in (0, 1, 2, 20, 32)}))


def r_of(f):
    """the first R of FAIL_RS under which row f can be the first failing one: an integer cost c + 1 with c <= (f - 1) R and
    c + 1 > f R"""
    for R in FAIL_RS:
        if int((f - 1) * R) + 1 > f * R:
            return R
    raise ValueError(f)


def burst(rng, f, m, R):
    """two sequences of length m, equal but for the rows f - c .. f, where one has A / C and the other G / T: cost(i, i) first
    exceeds i R at row f, and only in the few rows from f on -- a sweep that collects the diagonal a row off passes the pair"""
    c = int((f - 1) * R)
    assert f - c >= 1 and m >= f and c + 1 > f * R
    x = bytearray(ar.rand_seq(rng, m))
    y = bytearray(x)
    x[f - c - 1:f] = np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, c + 1)].tobytes()
    y[f - c - 1:f] = np.frombuffer(b"GT", np.uint8)[rng.randint(0, 2, c + 1)].tobytes()
    return bytes(x), bytes(y)


@functools.lru_cache(maxsize=None)
def burst_groups(NB):
    """{R: batch}: every row of burst_rows as the pair's last row and with clean rows behind it"""
    out = {}
    for f in burst_rows(NB):
        R = r_of(f)
        B = out.setdefault(R, ar.Batch())
        rng = np.random.RandomState(8400 + 7 * f + NB)
        for m in (f, f + BURST_TAIL):
            x, y = burst(rng, f, m, R)
            add(B, rng, x, y + ar.rand_seq(rng, 20 * (f % 3) if m > f else 0), f % 2 == 0, kind="fail", f=f, m=m, tag=f"fold{NB}:burst{f}:m{m}")
    return out


# ----------------------------------------------------------------------------- 3: S around the ring size
S_EDGES = (1, 2, 63, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def ring_fill_pairs(NB):
    """true pairs whose sweeps have S superblocks, the last one full (nr = S RB) and holding one row (nr = (S - 1) RB + 1);
    n - m = 5 <= w, so nr = n"""
    RB = 32 * NB
    rng = np.random.RandomState(8500 + NB)
    B = ar.Batch()
    for S in S_EDGES:
        for n in sorted({S * RB, max((S - 1) * RB + 1, 17)}):
            s, l = true_pair(rng, n - 5, 5)
            add(B, rng, s, l, bool(S % 2), kind="true", S=S, m=n - 5, extra=5, tag=f"fold{NB}:S{S}:n{n}")
    return B


# ----------------------------------------------------------------------------- 6: an all-vs-all that parks and resumes
WALK_R, WALK_L, WALK_ROW = 0.90, 3040, (2, 3)        # max_dst 2 737: the first launch in ring 2, the reference band in ring 3
WALK_MIN = 64
WALK_LONG = {"w1": 12, "w1+1": 12, "band": 8}        # planted pairs of WALK_L bases per cost (walk_costs)
WALK_SHORT = 114                                     # planted pairs of 2 000 .. 3 000 bases, each in its whole band


def walk_costs():
    """{name: cost} of the long pairs: at ring 2's first window (certified there), one above it and five below the band's
    largest accepted cost (both parked, resumed in ring 3)"""
    md = ar.max_dst_of(WALK_L, WALK_L, WALK_R)
    w1 = ar.bv_pass1_w(md, WALK_ROW[0])
    assert ar.nb1(md) == WALK_ROW[0] and ar.nb2(md) == WALK_ROW[1] and w1 + 1 < md - 5
    return {"w1": w1, "w1+1": w1 + 1, "band": md - 5}


@functools.lru_cache(maxsize=None)
def walk_set():
    """292 reads of 2 - 3 kb: every target read x (40 random bases, then A / C) has one query y, x with a planted number of
    G / T (walk_ring_inputs.plant: one edit each, whatever the path), behind the target range; one probe per read, so a pair
    is one candidate of one work item.  The long pairs come first, interleaved by cost, so that parked items lie between
    items that are decided narrowly; short[k] / long[name]: (x, y) read indices."""
    import walk_ring_inputs as wi
    S = wi.Set(12900)
    pairs, long, short = [], {n: [] for n in WALK_LONG}, []
    costs = walk_costs()
    for k in range(max(WALK_LONG.values())):
        for name, n in WALK_LONG.items():
            if k < n:
                x = wi.two_letter(S, WALK_L)
                pairs.append((name, x, wi.plant(x, costs[name], WALK_R)))
    for k in range(WALK_SHORT):
        L = 2000 + (997 * k) % 1001
        x = wi.two_letter(S, L)
        pairs.append((None, x, wi.plant(x, 2 + int(L * (0.02 + 0.28 * S.rng.rand())), WALK_R)))
    at = [S.add(x) for _, x, _ in pairs]
    t_hi = len(S.texts)
    for (name, _, y), ix in zip(pairs, at):
        iy = S.add(y, query=True)
        (long[name] if name else short).append((ix, iy))
    return wi.case_of(S, "fold_walk", WALK_R, 1, WALK_MIN, 0, t_hi, long=long, short=short)
