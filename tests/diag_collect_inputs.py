"""The inputs that say where the diagonal's D0 bits are collected (align_bitvec.h: bitvec_pass), shared by
test_gpu_diag_collect.py (the scalar one-hot, through align_pairs, the traced forms and locate) and walk_ring_inputs.py (the
lane-held one-hot of the all-vs-all walk): the failing rows at the edges of every block, the R under which each can be the
first failing one, and pairs whose diagonal runs on the bound (hug_pair).  No GPU and no engine in here."""
import numpy as np

import align_rings as ar

HEAD = 16                     # clean rows in front of every planted substitution: the seed of a probe lies in them
BEHIND = 45                   # rows behind a failing row that is not the pair's last
POS = (1, 2, 31, 32)          # rows of a block, counted from 1
SUPERBLOCKS = {1: (1, 2, 64, 65), 2: (1, 2, 64, 65), 3: (0, 1, 2)}
ROW = {1: (1, 1), 2: (2, 2), 3: (3, 4)}        # the plan row whose narrow launch runs in the ring


def fail_rows(NB):
    RB = 32 * NB
    return sorted(f for s in SUPERBLOCKS[NB] for nb in range(NB) for p in POS for f in [s * RB + 32 * nb + p] if f > 10)


def can_fail_first(f, R):
    """row f can be the FIRST failing one iff cost(f-1, f-1) = floor((f-1) R) passes and one more does not pass row f"""
    return int((f - 1) * R) + 1 > f * R


def greedy_groups(rows):
    """[(R, rows)]: the rows, each under an R at which it can be the first failing one.  Greedy over a 0.0005 grid of
    0.08 .. 0.30: the R that takes the most of what is left, the larger one on a tie."""
    left, out = list(rows), []
    while left:
        R = max((k * 0.0005 for k in range(160, 600)), key=lambda R: (sum(can_fail_first(f, R) for f in left), R))
        took = [f for f in left if can_fail_first(f, R)]
        assert took
        out.append((R, took))
        left = [f for f in left if f not in took]
    return out


def groups_of(NB):
    """[(R, rows)]: the rows of fail_rows, each under an R at which it can be the first failing one.  Greedy over a 0.0005 grid
    of 0.08 .. 0.30 (the pilots of rings 2 and 3 stay within the engine's sequence limit above 0.076): the R that takes the most
    of what is left, the larger one on a tie.  One R takes all the rows of rings 1 and 2; four consecutive rows (the end of a
    block and the start of the next) need frac((f - 1) R) + 4 R < 1 at their first one, and ring 3, which has such a run at
    every block edge from row 31 on, takes a second R for what the first leaves."""
    return greedy_groups(fail_rows(NB))


def sub(rng, c):
    return ar.ALPHA[(int(np.searchsorted(ar.ALPHA, c)) + 1 + rng.randint(3)) % 4]


def diag_costs(x, y, n):
    """cost(i, i), i = 0 .. n, of the plain unbanded unit-cost matrix of x[:n] against y[:n]"""
    prev, out = list(range(n + 1)), [0]
    for i in range(1, n + 1):
        cur = [i] + [0] * n
        for j in range(1, n + 1):
            cur[j] = min(prev[j - 1] + (x[i - 1] != y[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        out.append(cur[i])
        prev = cur
    return out


CATCH_UP = 72                 # rows within which the tightrope has caught up with the bound and runs at its natural spacing


def hug_pair(rng, m, R, tight_to, f=0):
    """x and a copy with substitutions only: behind HEAD clean rows one at every row where the count is below floor(i R) -- on
    every second row at the most, so the catching up is no run of substitutions that two indels could replace -- up to row
    tight_to: the diagonal's cost is floor(i R) from where it has caught up.  f: one more at row f (which can_fail_first
    says is no row of the tightrope), the first row to fail.  Clean behind.  Drawn again until the plain matrix of the first
    CATCH_UP rows has exactly the planted substitutions on its diagonal; behind them the substitutions stand alone, 1 / R
    rows apart, and the oracle has the last word in the test."""
    for _ in range(200):
        x = ar.rand_seq(rng, m)
        y = bytearray(x)
        cnt, cnts = 0, [0]
        for i in range(1, min(m, tight_to) + 1):
            if i > HEAD and ((cnt < int(i * R) and not (i >= 2 and y[i - 2] != x[i - 2])) or i == f):
                y[i - 1] = sub(rng, x[i - 1])
                cnt += 1
            cnts.append(cnt)
        n = min(m, tight_to, CATCH_UP)
        if diag_costs(x, y, n) == cnts[:n + 1] and cnts[n] == int(n * R) + (n == f):
            return x, bytes(y)
    raise AssertionError((m, R, tight_to, f))


def touches_bound(oracle, a, b, m, R, RB):
    """after oracle.align(a, b, R): cost(i, i) == floor(i R) at every segment end of the first three superblocks"""
    ends = [i for i in range(64, min(m, 3 * RB) + 1, 32)] + ([m] if m <= 3 * RB else [])
    return bool(ends) and all(oracle.cell(i, i)[0] == int(i * R) for i in ends)
