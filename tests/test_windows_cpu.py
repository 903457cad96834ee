"""Per-window alignment counts and the trim rule without a GPU: tests/windows_ref.py pinned by hand, the host twins
(pba_windows_from_script, pba_windows_bound, pba_trim_rows_apply) against it on the oracle's own scripts, the script-derived
windows against the run-derived ones, and the planted 6 % input with the oracle's rows: plain clip misses the chimeras, clip
over the trimmed rows finds them.  No GPU."""
import numpy as np

import align_rings as ar
import cigar_ref as cr
import windows_ref as wr
from clip_ref import PLANTED, clip_ref
from conftest import MASK_PAT
from correct_helpers import oracle_rows
from pacbioassembly_amd import engine as eng

FLAGS = (0, cr.REVERSED, cr.B_IS_QUERY, cr.REVERSED | cr.B_IS_QUERY)
WS = (1, 2, 7, 63, 64, 65, 100, 10000)


def W_(eq=0, x=0, ins=0, dele=0):
    return dict(n_eq=eq, n_x=x, n_ins=ins, n_del=dele)


def test_windows_by_hand():
    # a = ACGTAC from position 3, W = 4: x = 3 4 5 6 7 8, g = 0 1 1 1 1 2, w = 0 1 1 1 1 2
    ops, a, b = [1, 1, 3, 2, 1, 1, 1], b"ACGTAC", b"ACTTAG"
    # MATCH e0 A=A -> w0 | MATCH e1 C=C -> w1 | DELETE e2 -> w1 (I) | INSERT after 3 a-elements: e2 -> w1 (D) | MATCH e3 T=T -> w1
    # | MATCH e4 A=A -> w1 | MATCH e5 C/G -> w2 (X)
    want = [W_(eq=1), W_(eq=3, ins=1, dele=1), W_(x=1)]
    assert wr.from_script(ops, a, b, 3, False, 4) == want
    assert wr.from_script(ops, a, b, 3, False, 4, cr.REVERSED) == want[::-1]
    assert wr.from_script(ops, a, b, 3, False, 4, cr.B_IS_QUERY) == [W_(eq=1), W_(eq=3, ins=1, dele=1), W_(x=1)]
    # under B_IS_QUERY the two names are exchanged: one of each here, so a script with two DELETEs tells them apart
    assert wr.from_script([1, 3, 3], b"AAA", b"A", 0, False, 8) == [W_(eq=1, ins=2)]
    assert wr.from_script([1, 3, 3], b"AAA", b"A", 0, False, 8, cr.B_IS_QUERY) == [W_(eq=1, dele=2)]
    # backward from position 9, W = 4: x = 9 8 7 6 5 4, g = 2 2 1 1 1 1, w = 0 0 1 1 1 1
    assert wr.from_script(ops, a, b, 9, True, 4) == [W_(eq=2), W_(eq=2, x=1, ins=1, dele=1)]
    # a leading INSERT belongs to window 0; W = 1 gives one window per a-element, an INSERT with the element before it
    assert wr.from_script([2, 1, 2, 1], b"AC", b"TAGC", 5, False, 1) == [W_(eq=1, dele=2), W_(eq=1)]
    assert wr.from_script([], b"", b"", 7, False, 3) == [W_()]
    # the bound: the windows the clipped len_a touches.  a_len 100, b_len 20, R 0.3: md = 1 + 6, len_a = 27; from position 6 at
    # W = 7 the elements lie at 6 .. 32: g = 0 .. 4, five windows; backward from 32 the same five
    assert wr.bound(6, 100, 20, 0.3, 7) == 5 and wr.bound(32, 100, 20, 0.3, 7, True) == 5 and wr.bound(7, 100, 20, 0.3, 7) == 4
    assert wr.bound(0, 0, 0, 0.3, 7) == 1


def test_trim_rule_by_hand():
    # W = 10, max_err 0.25: thr[10] = 2, thr[4] = 1, thr[3] = 0
    assert wr.thr_table(0.25, 10) == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2]
    g, bad = W_(eq=9, x=1), W_(eq=7, x=3)                    # 10 a-elements each: err 1 <= 2, err 3 > 2
    edge = W_(eq=8, x=2)                                      # err == thr
    s = wr.trim([g, g, bad, g, g, g], 10, 0.25, 0)            # runs [0, 2) of 20 and [3, 6) of 30: the longer one
    assert (s["state"], s["w_beg"], s["w_end"], s["a0"], s["b0"], s["na"], s["nb"], s["cost"], s["n_runs"], s["n_good"]) == \
        (wr.CUT, 3, 6, 30, 30, 30, 30, 3, 2, 5)
    s = wr.trim([g, g, bad, g, g], 10, 0.25, 0)               # equal runs: the first
    assert (s["w_beg"], s["w_end"], s["a0"]) == (0, 2, 0)
    assert wr.trim([edge, edge], 10, 0.25, 0)["state"] == wr.WHOLE and wr.trim([bad, bad], 10, 0.25, 0)["state"] == wr.DROPPED
    assert wr.trim([g, g, bad], 10, 0.25, 20)["state"] == wr.CUT and wr.trim([g, g, bad], 10, 0.25, 21)["state"] == wr.DROPPED
    assert wr.trim([g, g, bad], 10, 0.25, 21)["n_runs"] == 1  # the run is still reported
    assert wr.trim([W_(ins=4, x=0)], 10, 1.0, 0)["state"] == wr.DROPPED      # a run without a b-element
    assert wr.trim([], 10, 0.25, 0) == dict(dict.fromkeys(wr.SPAN_FIELDS, 0), state=wr.DROPPED)
    # a window with an insertion and a deletion: na = 9 + 1 + 1, over W -- so 8 + 1 + 1 = 10: nb = 8 + 1 + 2, err = 1 + 1 + 2
    s = wr.trim([W_(eq=8, x=1, ins=1, dele=2)], 10, 0.5, 0)
    assert (s["na"], s["nb"], s["cost"]) == (10, 11, 4)
    # the row mapping.  Target windows [bad, g, g] in the target's forward order, 10 a- and b-elements each
    row = dict(dir=1, strand=1, j=5, t_beg=100, t_end=130, q_beg=5, q_end=35)
    t = wr.row_trim(row, 50, [bad, g, g], 10, 0.25, 0)
    assert (t["t_beg"], t["t_end"], t["q_beg"], t["q_end"]) == (110, 130, 15, 35)
    t = wr.row_trim(dict(row, strand=-1, q_beg=15, q_end=45), 50, [bad, g, g], 10, 0.25, 0)     # walked [15, 35) of rc(q): [50 - 35, 50 - 15)
    assert (t["q_beg"], t["q_end"]) == (15, 35)
    # dir -1: element order is the reverse; the kept run [1, 3) in the target's order is elements' [0, 2): a0 = b0 = 0.  The
    # walked query text ends at slen - j = 45 and the kept 20 elements are its last: [25, 45)
    t = wr.row_trim(dict(row, dir=-1, q_beg=15, q_end=45), 50, [bad, g, g], 10, 0.25, 0)
    assert (t["t_beg"], t["t_end"], t["q_beg"], t["q_end"]) == (110, 130, 25, 45)
    t = wr.row_trim(dict(row, dir=-1, q_beg=15, q_end=45), 50, [g, g, bad], 10, 0.25, 0)        # a0 = b0 = 10 in element order
    assert (t["t_beg"], t["t_end"], t["q_beg"], t["q_end"]) == (100, 120, 15, 35)


def pairs_under_test():
    """[(tag, a elements, b elements, a backward)] of cigar_ref's planted pairs and flags batch"""
    out = [(tag, a, b, False) for tag, a, b, _ in cr.planted_pairs()]
    for k, (a, fa, b, fb) in enumerate(cr.flags_batch()):
        out.append((f"flags{k}", a[::-1] if fa else a, b[::-1] if fb else b, fa))
    return out


def test_host_twin_equals_reference_and_runs(lib, oracle):
    """pba_windows_from_script against from_script, from_script against from_runs, the bound and the invariants: every planted
    pair, W in WS, a_pos at residues 0, 1, W - 1 of the grid, the four flag combinations"""
    R = cr.PLANT_R
    n_ok = n_multi = 0
    for tag, a, b, back in pairs_under_test():
        x = oracle.align(a, b, R, want_ops=True)
        for W in WS:
            for res in sorted({0, 1 % W, W - 1}):
                a_pos = (len(a) // W + 1) * W + res               # (a backward accessor reaches down len(a) - 1 positions)
                bd = eng.windows_bound(a_pos, len(a), len(b), R, W, back)
                assert bd == wr.bound(a_pos, len(a), len(b), R, W, back), (tag, W, res)
                if x["rc"] < 0:
                    continue
                for fl in FLAGS:
                    want = wr.from_script(x["ops"], a, b, a_pos, back, W, fl)
                    got = eng.windows_from_script(x["ops"], a, b, a_pos, back, W, fl)
                    assert [wr.tup(w) for w in want] == [tuple(int(v) for v in g) for g in got], (tag, W, res, fl)
                    runs, _ = cr.runs(x["ops"], a, b, fl)
                    assert wr.from_runs(runs, a_pos, back, W, fl) == want, (tag, W, res, fl)
                    wr.check_invariants(want, x, W, fl)
                    assert len(want) <= bd, (tag, W, res, len(want), bd)
                    n_multi += len(want) >= 3
                n_ok += 1
    assert n_ok >= 50 * len(WS) * 2 and n_multi >= 1000
    # caps and refusals of the host twin
    ops = np.array([1, 1, 3, 2, 1, 1, 1], np.uint8)
    win = np.zeros(2, eng.ALN_COUNTS_DTYPE)
    assert lib.pba_windows_from_script(ops.ctypes.data, 7, b"ACGTAC", b"ACTTAG", 3, 0, 4, 0, win.ctypes.data, 2) == 3
    assert [tuple(int(v) for v in w) for w in win] == [(1, 0, 0, 0), (3, 0, 1, 1)]
    assert lib.pba_windows_from_script(ops.ctypes.data, 7, b"ACGTAC", b"ACTTAG", 3, 0, 0, 0, win.ctypes.data, 2) == -1      # W < 1
    assert lib.pba_windows_from_script(ops.ctypes.data, 7, b"ACGTAC", b"ACTTAG", 3, 0, 4, 4, win.ctypes.data, 2) == -1      # a flag
    assert lib.pba_windows_from_script(ops.ctypes.data, 7, b"ACGTAC", b"ACTTAG", 3, 1, 4, 0, win.ctypes.data, 2) == -1      # below 0
    bad = np.array([1, 4], np.uint8)
    assert lib.pba_windows_from_script(bad.ctypes.data, 2, b"AC", b"AC", 0, 0, 4, 0, win.ctypes.data, 2) == -1
    assert eng.windows_bound(0, 10, 10, 0.3, 0) == 0 and eng.windows_bound(3, 10, 10, 0.3, 4, True) == 0 and eng.windows_bound(0, 10, 10, 1.0, 4) == 0
    assert eng.TRIM_ROW_DTYPE.itemsize == 44 == eng.TRIM_SPAN_DTYPE.itemsize


def test_fuzz_scripts(lib, oracle):
    """random pairs at 0 .. 30 % error, either side the longer one, forward and backward, a_pos anywhere"""
    rng = np.random.RandomState(8811)
    n_ok = 0
    for k in range(120):
        m = int(rng.randint(1, 500))
        x = ar.rand_seq(rng, m)
        y = ar.mutate(rng, x, (0.0, 0.03, 0.1, 0.2)[k % 4], head=min(40, m // 2)) + ar.rand_seq(rng, int(rng.randint(0, 60)))
        a, b = (y, x) if k % 2 else (x, y)
        back, W = bool(k % 3 == 0), int(rng.choice([1, 3, 16, 50, 100, 128]))
        a_pos = int(rng.randint(len(a), 3 * len(a) + 5))
        res = oracle.align(a, b, 0.3, want_ops=True)
        if res["rc"] < 0:
            continue
        n_ok += 1
        for fl in FLAGS:
            want = wr.from_script(res["ops"], a, b, a_pos, back, W, fl)
            got = eng.windows_from_script(res["ops"], a, b, a_pos, back, W, fl)
            assert [wr.tup(w) for w in want] == [tuple(int(v) for v in g) for g in got], (k, fl)
            assert wr.from_runs(cr.runs(res["ops"], a, b, fl)[0], a_pos, back, W, fl) == want
            wr.check_invariants(want, res, W, fl)
            assert len(want) <= eng.windows_bound(a_pos, len(a), len(b), 0.3, W, back)
    assert n_ok >= 80


def test_trim_rows_apply(lib):
    rows = np.zeros(4, eng.STRAND_OVERLAP_DTYPE)
    rows["target"], rows["query"], rows["strand"] = (0, 1, 2, 3), (4, 5, 6, 7), (1, -1, 1, -1)
    rows["t_beg"], rows["t_end"], rows["q_beg"], rows["q_end"] = (0, 10, 20, 30), (100, 110, 120, 130), (1, 2, 3, 4), (91, 92, 93, 94)
    rows["j"], rows["cost"] = (7, 8, 9, 10), (11, 12, 13, 14)
    trims = np.zeros(4, eng.TRIM_ROW_DTYPE)
    trims["state"] = (wr.WHOLE, wr.DROPPED, wr.CUT, wr.CUT)
    trims["t_beg"], trims["t_end"], trims["q_beg"], trims["q_end"] = (0, 0, 40, 50), (100, 0, 100, 90), (1, 0, 23, 34), (91, 0, 63, 44)
    got = eng.trim_rows_apply(rows, trims)
    want = wr.apply_trims(rows, [dict(zip(trims.dtype.names, t)) for t in trims.tolist()])
    assert got.tolist() == want.tolist() and len(got) == 3
    assert got["target"].tolist() == [0, 2, 3] and got["t_beg"].tolist() == [0, 40, 50] and got["j"].tolist() == [7, 9, 10]
    assert len(eng.trim_rows_apply(rows[:0], trims[:0])) == 0


def test_planted_six_percent(lib, oracle):
    """The planted input of tests/test_gpu_windows.py::test_end_to_end_planted with the rows, the scripts and both rules from
    the CPU oracle and the plain Python references.  Conditions (windows_ref.planted_conditions): under plain clip at least 6 of
    the 11 chimeras stay WHOLE (observed: 10); under the trimmed rows none is WHOLE, at most 2 keep both J - margin and
    J + margin (observed: 0), and at least as many clean reads stay whole as under plain clip, minus 4 (observed difference:
    0).  Everything else is printed."""
    P, T = PLANTED, wr.TRIM
    texts, chim = wr.planted_reads_6()
    rows = oracle_rows(oracle, texts, eng.mask_from_pattern(MASK_PAT), P["R"], nthreads=16)
    trims = []
    for r in rows:
        wins, _ = wr.row_windows(oracle, r, texts, P["R"], T["W"], cr.REVERSED if int(r["dir"]) == -1 else 0)
        trims.append(wr.row_trim(r, len(texts[int(r["query"])]), wins, T["W"], T["max_err"], T["min_span"]))
    print(len(rows), "rows;", sum(t["state"] == wr.CUT for t in trims), "cut,", sum(t["state"] == wr.DROPPED for t in trims), "dropped")
    lens = [len(t) for t in texts]
    plain = clip_ref(lens, rows, P["margin"], P["min_cov"])
    trimmed = clip_ref(lens, wr.apply_trims(rows, trims), P["margin"], P["min_cov"])
    wr.planted_conditions(plain["table"], trimmed["table"], chim, P["margin"])
