"""The inputs of tests/test_gpu_align_rings.py are what they are named for: proven here from the oracle and from the
constants parsed out of align_bitvec.h alone, so that no GPU test can pass vacuously.  No GPU."""
import numpy as np
import pytest

import align_rings as ar

# (nb1, nb2) -> largest max_dst range, as the plan table of DESIGN.md 4.2 states it
TABLE = [(1, 1386, 1, 1), (1387, 2463, 1, 2), (2464, 2730, 2, 2), (2731, 4074, 2, 3), (4075, 4853, 2, 4), (4854, 5418, 3, 4),
         (5419, 7242, 3, 6), (7243, 8106, 4, 6), (8107, 9631, 4, 8), (9632, 10794, 6, 8)]
# first-pass window of a pair at the LOW end of its row (the ring's room; towards the top of a row 9/16 max_dst takes over)
WINDOWS = {(1, 2): (1384, 693), (2, 3): (2728, 1365), (2, 4): (2728, 1365), (3, 4): (4072, 2037), (3, 6): (4072, 2037),
           (4, 6): (5416, 2709), (4, 8): (5416, 2709), (6, 8): (8104, 4053)}
EDGE_R = 0.30


def test_plan_table_follows_from_the_constants():
    assert ar.RINGS == [1, 2, 3, 4, 6, 8] and ar.MAX_NB == 8
    assert ar.plan_rows() == TABLE
    for lo, hi, n1, n2 in TABLE:
        for md in (lo, hi):
            assert (ar.nb1(md), ar.nb2(md)) == (n1, n2), md
        if lo > 1:
            assert (ar.nb1(lo - 1), ar.nb2(lo - 1)) != (n1, n2)
    for row, (w, wl) in WINDOWS.items():
        lo, _ = ar.row_of(*row)
        assert (ar.bv_pass1_w(lo, row[0]), ar.bv_pass1_wl(lo, row[0])) == (w, wl), row
    # "whole band" in rows (1,1) and (2,2) holds up to the ring's room, two short of the row's end: max_dst 1385 / 1386 (2729 /
    # 2730) get w = 1384 (2728) in the narrow launch and a re-run in the same ring when their cost is above it
    assert ar.bv_pass1_w(1384, 1) == 1384 == ar.bv_pass1_w(1386, 1) and ar.bv_pass1_w(2728, 2) == 2728 == ar.bv_pass1_w(2730, 2)
    assert ar.bitvec_supports(10794) and not ar.bitvec_supports(10795)
    assert (ar.nb1(10795), ar.nb2(10795)) == (0, 0)
    # text_clip: the shorter side times R, truncated, plus one
    assert ar.max_dst_of(100, 5000, 0.3) == 31 and ar.max_dst_of(5000, 100, 0.3) == 31 and ar.max_dst_of(10, 10, 0.49) == 5


@pytest.mark.parametrize("row", [(lo, hi, a, b) for lo, hi, a, b in TABLE if (a, b) != (1, 1)])
def test_pilots_land_in_their_rows_and_fail_at_once(oracle, row):
    lo, hi, n1, n2 = row
    for md in (lo, hi):
        a, b = ar.pilot(md, EDGE_R)
        x = oracle.align(a, b, EDGE_R)
        assert x["max_dst"] == md and (ar.nb1(x["max_dst"]), ar.nb2(x["max_dst"])) == (n1, n2)
        assert x["rc"] == -1 and 11 <= x["fail_row"] <= 32, x


@pytest.mark.parametrize("NB", ar.RINGS[:-1])
def test_edge_set_of_every_ring(oracle, NB):
    B = ar.edge_pairs(NB, EDGE_R)
    exp = ar.expected(oracle, B, EDGE_R)
    assert 100 <= len(B.pairs) <= 220
    true = [x["rc"] >= 0 for x, m in zip(exp, B.meta) if m["kind"] == "true"]
    assert 3 * sum(true) >= len(true) and len(true) >= 60
    assert sum(x["rc"] < 0 for x, m in zip(exp, B.meta) if m["kind"] == "unrel") >= 30
    grid = [m for m in B.meta if "delta" in m]
    assert {m["m"] for m in grid} == set(ar.edge_ms(NB)) >= {32 * NB - 1, 32 * NB, 32 * NB + 1, 64 * NB, 64 * NB + 1, 10, 11}
    for m in ar.edge_ms(NB):
        md = 1 + int(m * EDGE_R)
        assert {g["delta"] for g in grid if g["m"] == m} == {0, 1, md - 1, md, md + 40}
        assert {g["kind"] for g in grid if g["m"] == m} == {"true", "unrel"}
    # every direction combination, both sides as the longer one, every origin residue on both sides and in both directions
    flags = [p[6] for p, m in zip(B.pairs, B.meta) if "delta" in m]
    assert set(flags) == {0, 1, 2, 3} and {m["a_longer"] for m in grid} == {True, False}
    for side, pos, bit in (("amod", 1, 1), ("bmod", 4, 2)):
        for back in (0, bit):
            assert {p[pos] % 32 for p, m in zip(B.pairs, B.meta) if "delta" in m and (p[6] & bit) == back} == {0, 1, 31}, (side, back)
    # the placements: sequence 0 read backward from below base 31, a sequence behind an empty one, the last sequence to its end
    assert sum(1 for p in B.pairs if p[0] == 0 and p[6] & 1 and p[1] < 31) >= 3
    assert sum(1 for p in B.pairs if p[3] == 0 and p[6] & 2 and p[4] < 31) >= 3
    empty = B.seqs.index(b"")
    assert any(p[0] == empty + 1 and p[1] == 0 for p in B.pairs) and any(p[0] == empty + 1 and p[6] & 1 for p in B.pairs)
    last = len(B.seqs) - 1
    assert any(p[3] == last and p[4] + p[5] == len(B.seqs[last]) and not p[6] & 2 for p in B.pairs)
    assert any(p[0] == last and p[6] & 1 for p in B.pairs)
    # the pilot leaves sequence 0 and the last sequence where they are
    P = B.with_pilot(ar.pilot(2464, EDGE_R))
    assert P.seqs[0] == B.seqs[0] and P.seqs[-1] == B.seqs[-1] and len(P.pairs) == len(B.pairs) + 1
    assert all(P.elems(q + 1) == B.elems(q) for q in range(len(B.pairs)))


@pytest.mark.parametrize("NB", ar.RINGS[:-1])
def test_wrap_pairs_have_the_rows_they_are_named_for(oracle, NB):
    B = ar.wrap_pairs(NB)
    exp = ar.expected(oracle, B, 0.30)
    RB = 32 * NB
    assert [max(x["len_a"], x["len_b"]) for x in exp] == [64 * RB - 1, 64 * RB, 64 * RB + 1, 64 * RB + 33]
    assert all(x["rc"] >= 0 for x in exp) and exp[3]["len_a"] > exp[3]["len_b"] and exp[0]["len_a"] < exp[0]["len_b"]
    for x in exp:                       # the narrow launch sweeps the whole band of these pairs in ring NB: every row is swept
        assert ar.bv_pass1_w(x["max_dst"], NB) == x["max_dst"] and min(x["len_a"], x["len_b"]) + x["max_dst"] >= 64 * RB + 33


EXC_MD = 2400


def excursion_case():
    w, wl = ar.bv_pass1_w(EXC_MD, 1), ar.bv_pass1_wl(EXC_MD, 1)
    return ar.excursion_pairs(EXC_MD, w, wl), w, wl


def must_redo(exp, meta, w, wl):
    """pairs no sweep over [i - w, i + wl] can certify: an accepted cost above min(w, 2 wl + 1), or a failure at a row fr
    with fr R >= 2 wl + 2"""
    return [q for q, (x, m) in enumerate(zip(exp, meta))
            if (x["rc"] >= 0 and x["cost"] > min(w, 2 * wl + 1)) or (x["rc"] < 0 and x["fail_row"] * ar.EXC_R >= 2 * wl + 2)]


def test_excursion_pairs_leave_the_window_as_named(oracle):
    B, w, wl = excursion_case()
    assert (w, wl) == WINDOWS[(1, 2)] and (ar.nb1(EXC_MD), ar.nb2(EXC_MD)) == (1, 2)
    exp = ar.expected(oracle, B, ar.EXC_R)
    seen = set()
    for x, m in zip(exp, B.meta):
        assert x["max_dst"] == EXC_MD, m
        if m["kind"] == "late":
            assert x["rc"] == -1 and x["fail_row"] * ar.EXC_R >= 2 * wl + 2, (m, x["fail_row"])
            continue
        assert x["rc"] >= 0, m
        out_wl, out_w = ar.script_excursion(x["ops"], m["a_rows"])
        d = m["d"]
        if m["side"] == "wl":
            assert d <= out_wl <= d + 8 and out_w <= 8, (m, out_wl, out_w)
            beyond = out_wl > wl
        else:
            assert d <= out_w <= d + 8 and out_wl <= 8, (m, out_wl, out_w)
            beyond = out_w > w
        assert beyond == (d > (wl if m["side"] == "wl" else w)), m
        if beyond:                       # header comment of align_bitvec.h: leaving costs >= 2 wl + 2 / >= w + 1
            assert x["cost"] >= (2 * wl + 2 if m["side"] == "wl" else w + 1), (m, x["cost"])
        seen.add((m["side"], d, m["a_rows"]))
    # every d on the side where the reference can accept it, in both orders of the pair
    for a_rows in (False, True):
        assert {d for s, d, r in seen if s == "w" and r == a_rows} == set(ar.excursion_ds(w, wl))
        assert {d for s, d, r in seen if s == "wl" and r == a_rows} == {wl - 1, wl, wl + 1, wl + 40}
    redo = must_redo(exp, B.meta, w, wl)
    assert sum(B.meta[q]["kind"] == "late" for q in redo) == len(B.pairs) // 2
    # the accepted ones beyond the window (d = wl + 1, wl + 40 on the wl side, d = w + 1 on the w side, both orders) are among them
    out = [q for q, m in enumerate(B.meta) if m["kind"] == "accept" and m["d"] > (wl if m["side"] == "wl" else w)]
    assert len(out) == 6 and set(out) <= set(redo)
    # ... and the ones exactly at the edge stay certifiable: cost == w after an excursion of exactly w / of wl - 1 and back
    assert sum(x["rc"] >= 0 and x["cost"] == w for x in exp) >= 3


@pytest.mark.parametrize("row", sorted(ar.WIDE))
def test_wide_pairs_cost_more_than_their_first_window(oracle, row):
    B, R = ar.wide_pairs(row)
    exp = ar.expected(oracle, B, R)
    assert len(exp) >= 2
    lo, hi = ar.row_of(*row)
    for x in exp:
        assert lo <= x["max_dst"] <= hi
        assert (min(x["len_a"], x["len_b"]) + 1) * (2 * x["max_dst"] + 1) <= ar.ORACLE_CELL_BUDGET
        assert x["rc"] >= 0 and x["cost"] > ar.bv_pass1_w(x["max_dst"], row[0]), (row, x["cost"])
    if row[1] == 8:                      # lane 0's second superblock in the widest ring
        assert all(max(x["len_a"], x["len_b"]) >= 64 * 256 + 1 for x in exp)
    assert {r[1] for r in ar.WIDE} == {3, 4, 6, 8}
