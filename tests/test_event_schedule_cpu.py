"""The inputs of tests/test_gpu_event_schedule.py are what they are named for, from the oracle and the constants of
align_bitvec.h alone.  No GPU."""
import pytest

import align_rings as ar
import event_schedule_inputs as ev


@pytest.mark.parametrize("NB", [1, 2])
def test_hugging_pairs_run_along_the_window_edge(oracle, NB):
    w, wl = ev.hug_window(NB)
    assert (w, wl) == {1: (1384, 693), 2: (2728, 1365)}[NB]
    RB, m = 32 * NB, ev.HUG_M[NB]
    assert m > 64 * RB                                             # past the first ring wrap
    dels, ins = ev.hug_gaps(NB)
    assert dels == [w - RB - 1, w - RB, w - RB + 1, w - 1, w] and ins == [wl - 1, wl]
    ok, redo = ev.hug_pairs(NB)
    assert [x["kind"] for x in ok.meta] == ["del"] * 5 + ["ins"] and [x["g"] for x in redo.meta] == [wl]
    for B in (ok, redo):
        for q, (meta, x) in enumerate(zip(B.meta, ar.expected(oracle, B, ev.HUG_R))):
            g = meta["g"]
            a, b = B.elems(q)
            assert oracle.align(a, b, ev.HUG_R)["cost"] == x["cost"]
            diag = oracle.cell(m, m)[0]                            # D(m,m): what k_align_pairs and k_locate also report
            assert ar.nb1(x["max_dst"]) == NB and min(x["len_a"], x["len_b"]) == m
            ahead, behind = ar.script_excursion(x["ops"], meta["a_rows"])      # columns - rows: max, -min
            if meta["kind"] == "del":
                # the reference accepts it at cost g, the path g rows ahead of the columns to the free end: certified (g <= w)
                assert x["rc"] >= 0 and x["cost"] == g <= min(w, 2 * wl + 1) and g <= x["max_dst"] - 1, (meta, x)
                assert behind == g and ahead == 0 and max(x["matlen_a"], x["matlen_b"]) == m + g
                assert max(x["len_a"], x["len_b"]) == m + g <= m + w
                assert min(w, 2 * wl + 1) < diag <= x["max_dst"] - 1       # ... which the narrow window cannot vouch for
            else:
                assert x["rc"] >= 0 and x["cost"] == 2 * g <= x["max_dst"] - 1, (meta, x)
                assert ahead == g and behind == 0 and diag == 2 * g
                assert (B is ok) == (2 * g <= min(w, 2 * wl + 1))


@pytest.mark.parametrize("NB", [1, 2])
def test_coinciding_pairs_pass_and_fail_where_named(oracle, NB):
    RB = 32 * NB
    B = ev.coin_pairs(NB)
    ms = ev.coin_ms(NB)
    assert {11, 12, 31, 33, RB - 1, RB, RB + 1} <= set(ms)
    assert any((m + ar.max_dst_of(m, m + 1, ev.COIN_R)) % RB == 0 for m in ms)
    exp = ar.expected(oracle, B, ev.COIN_R)
    seen = set()
    for meta, x in zip(B.meta, exp):
        if meta["kind"] == "true":
            assert x["rc"] >= 0 and min(x["len_a"], x["len_b"]) == meta["m"], (meta, x)
            assert ar.bv_pass1_w(x["max_dst"], NB) == x["max_dst"]            # its whole band: certified by the narrow sweep
        else:
            assert x["rc"] == -1 and x["fail_row"] == meta["f"], (meta, x)
            seen.add(meta["f"])
    assert seen == set(ev.FAIL_ROWS) | {64 * RB + 20}
    assert len(B.pairs) <= 80
