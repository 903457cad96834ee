"""The inputs of tests/test_gpu_lane_shift.py are what they are named for, from the oracle and the constants of align_bitvec.h
alone.  No GPU."""
import pytest

import align_rings as ar
import lane_shift_inputs as ls


@pytest.mark.parametrize("NB", [1, 2])
def test_wrap_pairs_have_their_rows_and_their_deltas(oracle, NB):
    """every pair passes the diagonal's checks in its own first window (no re-run), its longer side has the rows it is named
    for, and the five deltas stand where they are named: 0, 1, one below the wide side, on it, 40 past it; both orders"""
    RB = 32 * NB
    B = ls.wrap_batch(NB)
    assert {x["rows"] for x in B.meta} == {64 * RB - 1, 64 * RB, 64 * RB + 1, 65 * RB + 1, 128 * RB + 1}
    assert {x["a_longer"] for x in B.meta} == {False, True}
    for meta, x in zip(B.meta, ar.expected(oracle, B, ls.WRAP_R)):
        m, n = min(x["len_a"], x["len_b"]), max(x["len_a"], x["len_b"])
        md = ar.max_dst_of(m, meta["rows"], ls.WRAP_R)
        assert (m, n) == (meta["m"], min(meta["rows"], m + md)), (meta, x)           # (the reference clips the longer side)
        assert (x["len_a"] > x["len_b"] or m == n) == (meta["a_longer"] or m == n), (meta, x)
        n = meta["rows"]
        w, wl = ar.bv_pass1_w(md, NB), ar.bv_pass1_wl(md, NB)
        assert w == md and wl + w <= ar.bv_max_span(NB)       # the first window is the whole band: nothing is swept twice
        assert x["fail_row"] == 0, (meta, x)
        want = {"0": 0, "1": 1, "w-1": w - 1, "w": w, "w+40": w + 40}[meta["delta"]]
        assert n - m == want or (meta["delta"] != "0" and meta["delta"] != "1" and 0 <= n - m - want <= 1), (meta, n - m, w)
        # rows swept: min(n, m + w); the superblocks past the 64th are what the last lane takes at a close
        S = (min(n, m + w) + RB - 1) // RB
        assert S >= 63
    assert any(min(x["rows"], x["m"] + ar.bv_pass1_w(ar.max_dst_of(x["m"], x["rows"], ls.WRAP_R), NB)) > 128 * RB for x in B.meta)


@pytest.mark.parametrize("NB", [1, 2])
def test_seg_pairs_fail_first_in_the_segment_beside_the_close(oracle, NB):
    RB = 32 * NB
    B = ls.seg_batch(NB)
    assert {(x["close"], x["dd"]) for x in B.meta} == {(c, d) for c in ls.SEG_CLOSES for d in ls.SEG_DD}
    for meta, x in zip(B.meta, ar.expected(oracle, B, ls.SEG_R)):
        m, n = min(x["len_a"], x["len_b"]), max(x["len_a"], x["len_b"])
        assert m == meta["m"] and n == m + 12
        assert x["rc"] == -1 and x["fail_row"] == meta["f"], (meta, x)
        md = ar.max_dst_of(m, n, ls.SEG_R)
        w, wl = ar.bv_pass1_w(md, NB), ar.bv_pass1_wl(md, NB)
        i, c = meta["seg_end"], meta["close"]
        assert i % 32 == 0 and i - 31 <= meta["f"] <= i and i < m
        assert c * RB + RB + wl < m                            # the close is no end-of-text close
        assert ls.t_seg(i, RB) - ls.t_close(c, m, wl, RB) == meta["dd"]
        # superblock c + 1 .. of the segment are in lanes 1 .. before the close and 0 .. behind it; the narrow sweep's verdict stands
        assert (i - 1) // RB > c and (i - 1) // RB - c < 64
        assert meta["f"] * ls.SEG_R < 2 * wl + 2


@pytest.mark.parametrize("NB", [1, 2])
def test_alias_pairs_put_the_minimum_in_every_kind_of_superblock(oracle, NB):
    RB = 32 * NB
    B = ls.alias_batch(NB)
    m0 = ls.alias_m(NB)
    md = ar.max_dst_of(m0, m0 + 1, ls.ALIAS_R)
    assert ar.bv_pass1_w(md, NB) == md and (m0 - 1) // RB >= 64           # many closes before the first fin word
    seen = set()
    for meta, x in zip(B.meta, ar.expected(oracle, B, ls.ALIAS_R)):
        if x["rc"] < 0:
            continue
        m, n = min(x["len_a"], x["len_b"]), max(x["len_a"], x["len_b"])
        assert m == m0
        S, s_m = (min(n, m + md) + RB - 1) // RB, (m - 1) // RB
        sb = (max(x["matlen_a"], x["matlen_b"]) - 1) // RB
        assert s_m <= sb < S
        if S - 1 > s_m:
            seen.add("first, closed early" if sb == s_m else "last, open at the end" if sb == S - 1 else "between, closed early")
        else:
            seen.add("only one")
    assert seen == {"first, closed early", "between, closed early", "last, open at the end", "only one"}, seen


@pytest.mark.parametrize("NB", [1, 2])
def test_driver_reads_are_found_once_and_align_as_planted(oracle, NB):
    g, texts, meta = ls.driver_case(NB)
    gb = g.tobytes()
    n_true = n_fail = 0
    for t, mt in zip(texts, meta):
        if mt["kind"] == "filler":
            continue
        assert gb.count(t[:16]) == 1 and gb.find(t[:16]) == mt["pos"]
        x = oracle.align(t, gb[mt["pos"]:mt["pos"] + 2 * len(t) + 8], ls.DRIVER_R)
        if mt["kind"] == "fail":
            assert x["rc"] == -1 and x["fail_row"] > 24, (mt, x)        # behind the head the two share
            n_fail += 1
        else:
            assert x["rc"] >= 0 and x["len_a"] == mt["m"], (mt, x)
            n_true += 1
    assert n_true == len(ls.driver_ms(NB)) and n_fail == 4
