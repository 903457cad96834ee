"""tests/sites_ref.py pinned by hand, without a GPU: the site rule at every threshold's equality and one below, its tie orders,
both kinds on one box, two weights; the per-row allele records on scripts written out op by op; and the conditions the planted
diploid input must meet on the CPU oracle's own boxes (conditions, not measurements: tests/test_gpu_sites.py relies on them)."""
import numpy as np
import pytest

import sites_ref as sr
from sites_ref import DEL, SEL, SUP

A, C, G, T = 0, 1, 2, 3


def box(sel, sup=(0, 0, 0, 0), tot=None, dels=0):
    """one box as arrays: tot defaults to 1 + the votes the counters and `dels` DELETEs account for under weight 1"""
    sel, sup = np.array([sel], np.uint16), np.array([sup], np.uint16)
    tot = np.array([int(sel.sum()) + dels if tot is None else tot], np.int32)     # weight 1: N = tot
    return sel, sup, tot


def one(sel, sup=(0, 0, 0, 0), th=(1, 1, 0), own=b"A", weight=1, tot=None, dels=0):
    return [tuple(int(v) for v in s) for s in sr.sites_of(*box(sel, sup, tot, dels), own, weight, th)]


def test_each_threshold_at_equality_and_one_below():
    # N = 10, minor C = 3: depth, count and share each at equality
    assert one((7, 3, 0, 0), th=(10, 3, 300)) == [(0, 0, SEL, A, A, C, 10, 7, 3)]
    assert one((7, 3, 0, 0), th=(11, 3, 300)) == []                      # one row short of min_depth
    assert one((7, 3, 0, 0), th=(10, 4, 300)) == []                      # one allele short of min_alt
    assert one((7, 3, 0, 0), th=(10, 3, 301)) == []                      # 3000 < 3010
    assert one((7, 3, 0, 0), th=(10, 3, 0)) == [(0, 0, SEL, A, A, C, 10, 7, 3)]
    assert one((10, 0, 0, 0), th=(1, 1, 0)) == []                        # min_alt >= 1: a box without a second allele is none
    # a minor that ties the major holds half of N: a site at 500 permille, none at 501
    assert one((5, 5, 0, 0), th=(1, 1, 500)) == [(0, 0, SEL, A, A, C, 10, 5, 5)]
    assert one((5, 5, 0, 0), th=(1, 1, 501)) == []


def test_tie_orders():
    assert one((4, 4, 4, 4))[0][4:6] == (A, C)                           # all equal: the first two in order
    assert one((1, 4, 4, 0), tot=10)[0][4:6] == (C, G)                   # weight 1, N = 10, DEL = 1
    assert one((2, 0, 0, 2), dels=2)[0][4:6] == (A, T)                   # T before DEL on a tie for minor
    assert one((2, 0, 0, 1), dels=2)[0][4:6] == (A, DEL)                 # A before DEL on a tie for major
    # major = DEL: six rows deleted the base, three matched it
    assert one((3, 0, 0, 0), dels=6) == [(0, 0, SEL, A, DEL, A, 9, 6, 3)]
    assert one((0, 3, 3, 0), dels=6, own=b"C")[0][3:9] == (C, DEL, C, 12, 6, 3)


def test_own_neither_major_nor_minor():
    # the target's own base G carries only its weight; the rows split between A and T
    assert one((5, 0, 1, 4), own=b"G") == [(0, 0, SEL, G, A, T, 10, 5, 4)]


def test_both_kinds_on_one_box_sel_first():
    got = one((6, 4, 0, 0), sup=(0, 0, 5, 1), th=(10, 4, 400))
    assert got == [(0, 0, SEL, A, A, C, 10, 6, 4), (0, 0, SUP, A, A, G, 10, 0, 5)]
    assert one((6, 4, 0, 0), sup=(0, 0, 3, 3), th=(10, 4, 400)) == [(0, 0, SEL, A, A, C, 10, 6, 4)]
    assert one((10, 0, 0, 0), sup=(0, 0, 0, 4), th=(10, 4, 400)) == [(0, 0, SUP, A, A, T, 10, 0, 4)]
    assert one((10, 0, 0, 0), sup=(2, 2, 0, 0), th=(1, 2, 0))[0][5] == A  # the first maximal sup base


def test_weight_1_and_3():
    # the same votes (5 x A on an own A, 3 x C) under weight 1 and weight 3: the own base's counter and N carry the weight
    sel1, sel3 = (6, 3, 0, 0), (8, 3, 0, 0)
    assert one(sel1, tot=9, weight=1) == [(0, 0, SEL, A, A, C, 9, 6, 3)]
    assert one(sel3, tot=9, weight=3) == [(0, 0, SEL, A, A, C, 11, 8, 3)]
    assert one(sel1, tot=9, weight=1, th=(1, 1, 300)) and not one(sel3, tot=9, weight=3, th=(1, 1, 300))   # 3 / 9 but 3 / 11
    # several boxes: positions, and the target id handed through
    sel = np.array([[9, 0, 0, 0], [3, 0, 4, 0], [1, 0, 0, 0]], np.uint16)
    sup = np.zeros((3, 4), np.uint16)
    got = sr.sites_of(sel, sup, np.array([9, 7, 1], np.int32), b"AAA", 1, (1, 1, 0), target=5)
    assert [(int(s["target"]), int(s["pos"]), int(s["major"]), int(s["minor"])) for s in got] == [(5, 1, G, A)]


# ----------------------------------------------------------------------------- scripts
def test_site_on_match_delete_and_between_inserts():
    #            a: x0 x1 x2 -- -- x3 x4        (a_pos = 10: positions 10 .. 14)
    ops = [1, 1, 3, 2, 2, 1, 1]
    b = b"ACGTTA"                                   # b0 b1 | b2 b3 inserted | b4 b5
    # the site on the DELETE (a-element 2), INSERTs right behind it: the inserted bases leave nothing
    assert sr.alleles_from_script(ops, b, 10, False, [12]) == [(0, DEL)]
    # INSERTs on either side of a site: a-elements 2 (before the run) and 3 (after it)
    assert sr.alleles_from_script(ops, b, 10, False, [11, 13]) == [(0, C), (1, T)]
    assert sr.alleles_from_script(ops, b, 10, False, [10, 14]) == [(0, A), (1, A)]
    assert sr.alleles_from_script(ops, b, 10, False, [9, 15]) == []          # one before and one past the covered span
    assert sr.alleles_from_script([], b"", 10, False, [10]) == []
    assert sr.alleles_from_script([2, 2], b"AC", 10, False, [10]) == []     # a path of INSERTs alone consumes no a-element


def test_backward_accessor_ascending_site_order():
    ops = [1, 1, 3, 2, 2, 1, 1]
    b = b"ACGTTA"
    # a_pos = 14, backward: a-element e at 14 - e; the records come in ascending site order all the same
    assert sr.alleles_from_script(ops, b, 14, True, [10, 12, 14]) == [(0, A), (1, DEL), (2, A)]
    assert sr.alleles_from_script(ops, b, 14, True, [11, 13]) == [(0, T), (1, C)]
    assert sr.alleles_from_script(ops, b, 14, True, [9, 15]) == []


def test_row_totals_and_histogram():
    sites = np.zeros(3, sr.SITE)
    sites["own"], sites["major"], sites["minor"] = [A, G, C], [A, A, DEL], [C, T, C]
    recs = [(0, A), (1, G), (2, DEL), (2, C)]
    assert sr.row_totals(recs[:3], sites) == dict(n_sites=3, n_own=2, n_major=2, n_minor=0, n_other=1)
    assert sr.row_totals([(2, C)], sites) == dict(n_sites=1, n_own=1, n_major=0, n_minor=1, n_other=0)
    h = sr.histogram(3, recs)
    assert h.tolist() == [[1, 0, 0, 0, 0], [0, 0, 1, 0, 0], [0, 1, 0, 0, 1]]
    c = sr.box_counts(np.array([[3, 0, 4, 0]], np.uint16), np.array([9], np.int32), 2)
    assert c.tolist() == [[3, 0, 4, 0, 3]]
    assert sr.tsv_line(sr.sites_of(*box((3, 0, 0, 0), dels=6), b"A", 1, (1, 1, 0))[0], "ctg") == "ctg\t1\tSEL\tA\t-\tA\t9\t6\t3"


def test_engine_tsv_lines_are_the_reference_lines():
    from pacbioassembly_amd import engine as eng
    recs = np.zeros(3, sr.SITE)
    recs["target"], recs["pos"], recs["kind"] = [0, 0, 2], [9, 9, 0], [SEL, SUP, SEL]
    recs["own"], recs["major"], recs["minor"] = [A, A, T], [A, A, DEL], [G, C, T]
    recs["n"], recs["n_major"], recs["n_minor"] = [12, 12, 9], [8, 0, 5], [4, 3, 4]
    lines = list(eng.sites_tsv_lines(recs.astype(eng.SITE_DTYPE)))
    assert lines == [sr.tsv_line(r) for r in recs] and lines[1] == "0\t10\tSUP\tA\tA\tC\t12\t0\t3"
    names = ["ctg_a", "x", "ctg_c"]
    assert list(eng.sites_tsv_lines(recs.astype(eng.SITE_DTYPE), names))[2] == sr.tsv_line(recs[2], "ctg_c") == "ctg_c\t1\tSEL\tT\t-\tT\t9\t5\t4"


# ----------------------------------------------------------------------------- the planted diploid
@pytest.fixture(scope="module")
def diploid_oracle(oracle):
    """the planted input voted by the CPU oracle: (case, map rows, the oracle's boxes, {row: align result})"""
    from conftest import MASK_PAT
    from map_ref import map_reads_ref
    from pacbioassembly_amd import engine as eng
    from polish_helpers import oracle_boxes, oracle_vote
    D = sr.DIPLOID
    case = sr.planted_diploid()
    h0, _, reads, _, _ = case
    rows, _, _ = map_reads_ref(oracle, [h0], reads, eng.mask_from_pattern(MASK_PAT), D["R"])
    cons, res, voted = oracle_vote(oracle, [h0], reads, rows, 0, D["weight"], D["R"], D["overlap_min"])
    return case, rows, oracle_boxes(cons, len(h0)), res, voted


def test_planted_diploid_conditions(diploid_oracle):
    """every planted site is found under the chosen thresholds, at most 1 % of the reported sites are unplanted, and the reads
    of each haplotype carry their haplotype's allele at the planted sites"""
    from polish_helpers import row_texts
    D = sr.DIPLOID
    (h0, h1, reads, hap_of, planted), rows, (sel, sup, tot), res, voted = diploid_oracle
    assert len(planted) >= 150 and {k for k, _, _ in planted.values()} == {"sub", "del"} and len(h1) < len(h0)
    assert voted >= 0.95 * len(reads) and {int(s) for s in rows["strand"][rows["found"] != 0]} == {1, -1}
    n = len(h0)
    sites = sr.sites_of(sel[:n], sup[:n], tot[:n], h0, D["weight"], D["thresholds"])
    sr.planted_conditions(sites, planted)
    pos = sorted(planted)
    agree = total = 0
    for k, o in res.items():
        if o["rc"] < 0 or o["matlen_a"] < D["overlap_min"]:
            continue
        pr, _, b = row_texts(rows[k], [h0], reads, D["R"])
        for s, a in sr.alleles_from_script(o["ops"], b, int(pr["a_pos"]), False, pos):
            total += 1
            agree += a == planted[pos[s]][1 + hap_of[k]]
    print("records at planted sites", total, "carrying their haplotype's allele", agree)
    assert total >= 10 * len(planted) and agree >= 0.9 * total


# ----------------------------------------------------------------------------- the hand-built inputs of the GPU tests
def test_scan_case_conditions(oracle):
    """the hand-built pile-up states hold what tests/test_gpu_sites.py plants them for, on the oracle's own boxes"""
    import sites_inputs as si
    from polish_helpers import oracle_boxes
    targets, reads, rows, want_sel, want_sup = si.scan_case()
    assert all(100 <= len(r) <= 301 for r in reads)
    off = np.concatenate([[0], np.cumsum([len(t) for t in targets])])
    assert [int(off[t]) % 64 for t in (1, 3, 4)] == [63, 0, 1]           # arena offsets 63 / 64 / 65 mod 64
    both = 0
    for t, T in enumerate(targets):
        if not T:
            continue
        cons, voted = si.oracle_place_vote(oracle, targets, reads, rows, t)
        assert voted == int((rows["contig"] == t).sum())
        sel, sup, tot = (x[:len(T)] for x in oracle_boxes(cons, len(T)))
        strict = sr.sites_of(sel, sup, tot, T, 1, si.STRICT, t)
        assert [int(s["pos"]) for s in strict if s["kind"] == SEL] == want_sel[t], t
        assert [int(s["pos"]) for s in strict if s["kind"] == SUP] == want_sup[t], t
        both += sum(1 for s in strict if s["kind"] == SUP and int(s["pos"]) in want_sel[t])
        if t == si.SCAN_DEL[0]:
            assert [int(s["minor"]) for s in strict if int(s["pos"]) == si.SCAN_DEL[1]] == [DEL]
        if t == si.SCAN_RUN[0]:
            loose = [int(s["pos"]) for s in sr.sites_of(sel, sup, tot, T, 1, si.LOOSE, t) if s["kind"] == SEL]
            assert loose == list(range(si.SCAN_RUN[1], si.SCAN_RUN[2])) and len(loose) == 200
    assert both == 1 and want_sel[0][0] == 0 and want_sel[0][-1] == len(targets[0]) - 1 and not want_sel[4]
    T, reads, rows = si.long_case()
    cons, voted = si.oracle_place_vote(oracle, [T], reads, rows, 0)
    sel, sup, tot = (x[:len(T)] for x in oracle_boxes(cons, len(T)))
    assert voted == len(reads) and [int(s["pos"]) for s in sr.sites_of(sel, sup, tot, T, 1, si.STRICT)] == list(si.LONG_SITES)


def test_sink_case_conditions(oracle):
    """the rows of the sink tests put their sites where the tests want them, on the oracle's own scripts"""
    import cigar_ref as cr
    import sites_inputs as si
    texts, rows, tags = si.sink_case()
    seen = {}
    for row, tag in zip(rows, tags):
        pr, a, b, a_pos, back = si.row_pair(row, texts)
        x = oracle.align(a, b, si.R, want_ops=True)
        assert x["rc"] >= 0, tag
        ops, ma = x["ops"], x["matlen_a"]
        la = cr.clip(int(pr["a_len"]), int(pr["b_len"]), si.R)[0]
        pos = si.choose_sites(tag, ops, a_pos, back, ma, la, len(texts[int(row["target"])]))
        recs = sr.alleles_from_script(ops, b, a_pos, back, pos)
        e = si.consumed(ops)
        seen[tag] = (pos, recs, ops, e, ma, a_pos, back)
        assert back == (int(row["dir"]) == -1)
    pos, recs, ops, e, ma, a_pos, back = seen["edges"]
    assert pos == [a_pos, a_pos + ma - 1, a_pos + ma] and [k for k, _ in recs] == [0, 1]      # one past the span: no record
    pos, recs, ops, e, ma, a_pos, back = seen["ops63"]
    assert len(ops) >= 300 and len(recs) == len(pos) >= 2
    pos, recs, *_ = seen["two"]
    assert len(recs) == len(pos) == 2
    pos, recs, ops, *_ = seen["copy"]
    assert len(pos) == len(recs) == 64 and pos[-1] - pos[0] == 63 and (np.asarray(ops) == 1).all()
    pos, recs, ops, *_ = seen["del"]
    assert sum(1 for _, a in recs) == len(pos) and sum(1 for _, a in recs if a == DEL) == 4 == int((np.asarray(ops) == 3).sum())
    for tag in ("back", "back-minus"):
        pos, recs, ops, e, ma, a_pos, back = seen[tag]
        assert back and a_pos - ma >= 0 and pos[0] == a_pos - ma and [k for k, _ in recs] == list(range(1, len(pos)))
    assert seen["nosite"][0] == [] and len(seen["tiny"][2]) <= 12 and len(seen["tiny"][1]) == 2
    recs = si.site_list(texts, {int(r["target"]): seen[t][0] for r, t in zip(rows, tags)})
    assert (recs["kind"] == SUP).sum() >= len(tags) - 1 and (recs["major"] == recs["own"]).all() and (recs["minor"] != recs["own"]).all()
