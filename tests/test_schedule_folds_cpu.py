"""The inputs of tests/test_gpu_schedule_folds.py are what they are named for, from the oracle and the constants of
align_bitvec.h alone.  No GPU."""
import numpy as np
import pytest

import align_rings as ar
import schedule_fold_inputs as sf
from diag_collect_inputs import diag_costs


def diag_costs_behind_prefix(x, y, k, n):
    """{i: cost(i, i)}, i = k .. n, of the plain unit-cost matrix of x[:n] against y[:n] where x[:k] == y[:k]: row k of that
    matrix is |k - j| (a prefix against a prefix of itself), and the rows behind it follow from it.  Kept to the columns
    within n - k + 1 of the diagonal: cost(i, i) <= i - k, so no path to a diagonal cell leaves them."""
    h = n - k + 1
    xs, ys = np.frombuffer(x, np.uint8), np.frombuffer(y, np.uint8)
    off = np.arange(-h, h + 1)
    prev = np.abs(off).astype(np.int64)                        # row k: columns k - h .. k + h
    out = {k: 0}
    big = 1 << 30
    for i in range(k + 1, n + 1):                              # row i: columns i - h .. i + h; prev is shifted by one column
        cols = i + off
        ok = (cols >= 1) & (cols <= n)
        yc = np.where(ok, ys[np.clip(cols - 1, 0, n - 1)], 255)
        diag = prev + (yc != xs[i - 1])                        # (i - 1, j - 1): the same offset
        up = np.append(prev[1:], big) + 1                      # (i - 1, j): offset + 1 in the row above
        cur = np.minimum(diag, up)
        cur = np.where(cols == 0, i, np.where(ok, cur, big))
        cur = np.minimum.accumulate(cur - off) + off           # (i, j - 1) + 1, along the row
        out[i] = int(cur[h])
        prev = cur
    return out


@pytest.mark.parametrize("NB", [1, 2])
def test_edge_pairs_pass_in_their_whole_band(oracle, NB):
    RB = 32 * NB
    B = sf.edge_pairs(NB)
    assert {x["m"] for x in B.meta} == set(sf.edge_ms(NB)) == {RB - 1, RB, RB + 1, 2 * RB, 2 * RB + 1, 64 * RB, 64 * RB + 1, 65 * RB + 1}
    seen = set()
    for meta, x in zip(B.meta, ar.expected(oracle, B, sf.FOLD_R)):
        m, n, w, nr, S = sf.geometry(NB, x["len_a"], x["len_b"])
        assert x["rc"] >= 0 and m == meta["m"] and (x["len_a"] > x["len_b"]) == (meta["a_rows"] and meta["extra"] > 0), (meta, x)
        assert ar.nb1(x["max_dst"]) <= NB and w == x["max_dst"]              # the ring's narrow window is the pair's whole band
        assert nr - m == meta["extra"] and meta["extra"] in (0, 1, w)
        seen.add((m, "0" if nr == m else "1" if nr == m + 1 else "w", meta["a_rows"]))
    assert len(seen) == 8 * 3 * 2
    assert max(x["m"] for x in B.meta) > 64 * RB                             # lane 0's second superblock


@pytest.mark.parametrize("NB", [1, 2, 3])
def test_bursts_fail_first_at_their_row_and_only_near_it(oracle, NB):
    RB = 32 * NB
    rows = sf.burst_rows(NB)
    assert {RB, RB + 1, RB + 2, 2 * RB, 2 * RB + 1, 64 * RB, 64 * RB + 1, 64 * RB + 20} <= set(rows)
    seen = set()
    for R, B in sf.burst_groups(NB).items():
        for q, (meta, x) in enumerate(zip(B.meta, ar.expected(oracle, B, R))):
            f = meta["f"]
            assert x["rc"] == -1 and x["fail_row"] == f and min(x["len_a"], x["len_b"]) == meta["m"], (meta, x)
            assert ar.bv_pass1_w(x["max_dst"], NB) == x["max_dst"]          # certified by the narrow sweep: nothing is re-run
            a, b = B.elems(q)
            n = min(meta["m"], f + 40)
            if f <= 200:                                                    # the plain matrix in Python: the short ones
                d = diag_costs(a, b, n)
                late = [i for i in range(11, n + 1) if d[i] > i * R]
                k = f - int((f - 1) * R) - 1                                # (and the two ways of computing it agree)
                assert diag_costs_behind_prefix(a, b, k, n) == {i: d[i] for i in range(k, n + 1)}
            else:                                                           # the others from the end of the common prefix on
                k = f - int((f - 1) * R) - 1
                assert a[:k] == b[:k]
                d = diag_costs_behind_prefix(a, b, k, n)
                late = [i for i in range(k + 1, n + 1) if d[i] > i * R]
            assert late and late[0] == f and late[-1] <= f + 6, (meta, late)     # a diagonal collected a few rows off passes
            seen.add((f, meta["m"] == f))
    assert seen == {(f, last) for f in rows for last in (True, False)}


@pytest.mark.parametrize("NB", [1, 2])
def test_ring_fill_pairs_have_their_superblocks(oracle, NB):
    B = sf.ring_fill_pairs(NB)
    got = []
    for meta, x in zip(B.meta, ar.expected(oracle, B, sf.FOLD_R)):
        m, n, w, nr, S = sf.geometry(NB, x["len_a"], x["len_b"])
        assert x["rc"] >= 0 and S == meta["S"] and nr == n and w == x["max_dst"], (meta, x)
        got.append((S, nr % (32 * NB)))
    assert {s for s, _ in got} == set(sf.S_EDGES) and {r for s, r in got if s > 1} == {0, 1}
    assert ar.nb1(max(x["max_dst"] for x in ar.expected(oracle, B, sf.FOLD_R))) <= NB


def test_walk_set_parks_in_ring_2_and_resumes_in_ring_3(oracle):
    import walk_ring_inputs as wi
    C = sf.walk_set()
    assert 250 <= len(C["texts"]) <= 400 and all(2000 <= len(t) <= sf.WALK_L for t in C["texts"])
    W = wi.model(oracle, C)
    n_pairs = sum(sf.WALK_LONG.values()) + sf.WALK_SHORT
    L = wi.listed(W)
    assert len(L) == n_pairs
    costs = sf.walk_costs()
    by_t = {}
    for t, v in L.items():                     # one candidate per target is its planted copy; a few tail keys hit by accident:
        for c in v:                            # candidates of a few dozen rows, decided in any window, no overlap
            if (c["jd"], c["p"]) == (0, 0):
                by_t[t] = c
            else:
                assert not c["ok"] and min(c["x"]["len_a"], c["x"]["len_b"]) < 128, c
    assert len(by_t) == n_pairs and sum(len(v) for v in L.values()) <= n_pairs + 8
    for name, ps in C["long"].items():
        for ix, iy in ps:
            c = by_t[ix]
            x = c["x"]
            assert c["q"] == iy and c["ok"] and x["cost"] == costs[name] and x["max_dst"] == wi.call_md(C), (name, x)
            assert wi.gives_up(x["diag"], sf.WALK_L, ar.bv_pass1_w(x["max_dst"], 2), sf.WALK_L, margin=0.97) == []   # never given up: not near it
            assert wi.outcome(c, 2, False, sf.WALK_R) == ("ok" if name == "w1" else "park") and wi.outcome(c, 3, True, sf.WALK_R) == "ok"
    for ix, iy in C["short"]:
        c = by_t[ix]
        assert c["q"] == iy and c["ok"] and ar.bv_pass1_w(c["x"]["max_dst"], 2) == c["x"]["max_dst"]
    want = wi.stages(W)
    parked = sf.WALK_LONG["w1+1"] + sf.WALK_LONG["band"]
    assert want["launches"] == [(2, "first", n_pairs), (3, "redo_band", parked)] and want["parked"] == parked
    assert len(want["rows"]) == len(W["rows"]) == n_pairs
