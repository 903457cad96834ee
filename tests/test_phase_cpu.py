"""The phase rule restated in numpy (tests/phase_ref.py) pinned by hand-computed answers, and the planted input of
tests/test_gpu_phase.py run end to end through the CPU oracle's composition -- rows, boxes, sites_of, alleles_from_script,
phase_ref, a vote by the kept rows only, evolve -- without a GPU.  Every comparison is exact."""
import itertools

import numpy as np
import pytest

import phase_ref as pr
import sites_ref as sr

A, C, G, T, DEL = 0, 1, 2, 3, 4
SEL, SUP = sr.SEL, sr.SUP


def sites_of(*specs):
    """SITE records from (own, major, minor) or (own, major, minor, kind), one target, positions 10 apart"""
    s = np.zeros(len(specs), sr.SITE)
    for k, sp in enumerate(specs):
        own, major, minor = sp[:3]
        s[k] = (0, 10 * k, sp[3] if len(sp) > 3 else SEL, own, major, minor, 12, 8, 4)
    return s


def run(sites, records, n_iter, min_margin, self_weight):
    rows, out, st = pr.phase_ref(sites, records, n_iter, min_margin, self_weight)
    return ([tuple(int(r[f]) for f in pr.ROW.names) for r in rows], [tuple(int(s[f]) for f in pr.SITE.names) for s in out], st)


def test_rows_of_no_and_one_record():
    S = sites_of((A, A, C))
    rows, sites, st = run(S, [[], [(0, A)]], 0, 1, 1)
    assert rows == [(0, 0, 0, 0), (1, 1, 1, 1)] and sites == [(0, 1, 1, 1, 0)]         # score = self_weight * o0 for n_iter 0
    assert st == dict(n_rows=2, n_same=1, n_other=0, n_unphased=1, n_sites=1, n_records=1, n_flipped_last=0)
    rows, sites, st = run(S, [[], [(0, A)]], 1, 1, 1)
    assert rows == [(0, 0, 0, 0), (1, 1, 1, 1)] and sites == [(0, 1, 2, 1, 0)]         # f = 1 * 1 + (+1)(+1)
    rows, sites, st = run(S, [[(0, C)]], 1, 2, 1)                                       # one record never reaches a margin of 2
    assert rows == [(0, -1, 1, 1)] and sites == [(0, 1, 1, 0, 0)] and st["n_unphased"] == 1


def test_margin_at_equality_and_one_below_and_zero():
    S = sites_of((A, A, C), (A, A, C), (A, A, C))
    recs = [[(0, A), (1, A), (2, A)],            # g = +3: at the margin
            [(0, A), (1, A), (2, T)],            # g = +2, one `other` allele: one below
            [(0, C), (1, C), (2, C)],            # g = -3
            [(0, C), (1, C)],                    # g = -2
            [(0, A), (1, C)]]                    # g = 0
    rows, sites, st = run(S, recs, 0, 3, 1)      # n_iter 0: the labels follow from the records' own counts
    assert rows == [(1, 3, 3, 3), (0, 2, 2, 3), (-1, -3, 3, 3), (0, -2, 2, 2), (0, 0, 2, 2)]
    # rows 0 and 2 are the labelled ones, and both agree: a row of the other copy that carries the minor allele is consistent
    assert sites == [(0, 1, 1, 2, 0), (1, 1, 1, 2, 0), (2, 1, 1, 2, 0)]
    assert (st["n_same"], st["n_other"], st["n_unphased"], st["n_records"], st["n_flipped_last"]) == (1, 1, 3, 13, 0)
    assert [r[0] for r in run(S, recs, 0, 2, 1)[0]] == [1, 1, -1, -1, 0]


def test_self_weight_cancelled_by_one_opposing_row():
    """f = 0: the site loses its orientation, stops being informative and counts nobody"""
    S = sites_of((A, A, C), (A, A, C), (A, A, C))
    rows, sites, st = run(S, [[(0, C), (1, A), (2, A)]], 1, 1, 1)
    # o0 = (1, 1, 1): g = -1 + 1 + 1 = 1, h = +1; f = (1 - 1, 1 + 1, 1 + 1); final g = 0 + 1 + 1
    assert sites == [(0, 0, 0, 0, 0), (1, 1, 2, 1, 0), (2, 1, 2, 1, 0)]
    assert rows == [(1, 2, 2, 3)] and st["n_flipped_last"] == 1
    assert run(S, [[(0, C), (1, A), (2, A)]], 1, 1, 2)[1][0] == (0, 1, 1, 0, 1)         # self_weight 2 holds it: the row disagrees


def test_own_neither_major_nor_minor():
    S = sites_of((G, A, C), (A, A, C))
    recs = [[(0, A), (1, A)]]
    assert run(S, recs, 0, 1, 1) == ([(1, 1, 1, 2)], [(0, 0, 0, 0, 0), (1, 1, 1, 1, 0)],
                                    dict(n_rows=1, n_same=1, n_other=0, n_unphased=0, n_sites=2, n_records=2, n_flipped_last=0))
    rows, sites, st = run(S, recs, 1, 1, 1)      # the row orients the unseeded site: f = 0 + 1
    assert rows == [(1, 2, 2, 2)] and sites == [(0, 1, 1, 1, 0), (1, 1, 2, 1, 0)] and st["n_flipped_last"] == 1


def test_other_allele_and_del_minor_and_sup_between():
    """a DEL minor is an allele like any; an allele that is neither votes nothing; a SUP record between two SEL ones makes the
    record index differ from the SEL rank"""
    S = sites_of((A, A, DEL), (A, A, G, SUP), (C, DEL, C))
    assert [pr.value(S[0], a) for a in (A, C, G, T, DEL)] == [1, 0, 0, 0, -1]
    assert [pr.value(S[2], a) for a in (A, C, G, T, DEL)] == [0, -1, 0, 0, 1]
    recs = [[(0, DEL), (2, C)],                  # o0 = (+1, -1): g = -1 + 1 = 0
            [(0, A), (2, C)],                    # g = +1 + 1
            [(0, T), (2, DEL)]]                  # g = 0 - 1
    rows, sites, st = run(S, recs, 0, 1, 1)
    assert rows == [(0, 0, 2, 2), (1, 2, 2, 2), (-1, -1, 1, 2)]
    assert sites == [(0, 1, 1, 1, 0), (2, -1, -1, 2, 0)] and st["n_sites"] == 2


def test_two_iterations_to_settle():
    """w = 0: the first iteration leaves site 2 at f = 0, the second decides it from the one row that is labelled by then; the
    labels after one and after two iterations differ, and nothing flips in a third"""
    S = sites_of((A, A, C), (A, A, C), (A, A, C))
    recs = [[(0, A), (1, A), (2, C)], [(0, T), (1, T), (2, A)]]
    one, two, three = (run(S, recs, k, 1, 0) for k in (1, 2, 3))
    assert one[0] == [(1, 2, 2, 3), (0, 0, 0, 3)] and one[1] == [(0, 1, 1, 1, 0), (1, 1, 1, 1, 0), (2, 0, 0, 0, 0)]
    assert two[0] == [(1, 3, 3, 3), (-1, -1, 1, 3)] and two[1] == [(0, 1, 1, 1, 0), (1, 1, 1, 1, 0), (2, -1, -1, 2, 0)]
    assert (one[2]["n_flipped_last"], two[2]["n_flipped_last"], three[2]["n_flipped_last"]) == (1, 1, 0)
    assert three[0] == two[0] and three[1] == two[1][:2] + [(2, -1, -2, 2, 0)]           # both rows pull site 2 by now


def test_no_two_row_two_site_input_oscillates():
    """The alternating update (rows from sites, sites from rows) is a bidirectional associative memory and settles: over EVERY
    two-row, two-site input (each value +1, -1 or absent, each seed +1, -1 or 0, self_weight 0..2, min_margin 1..2) three and
    four iterations give the same labels and orientations, and the fourth flips nothing"""
    allele = {1: A, -1: C, 0: T}
    own = {1: A, -1: C, 0: G}
    n = 0
    for o0 in itertools.product((1, -1, 0), repeat=2):
        S = sites_of(*[(own[o], A, C) for o in o0])
        for M in itertools.product((1, -1, 0), repeat=4):
            recs = [[(s, allele[M[2 * r + s]]) for s in range(2)] for r in range(2)]
            for w, mm in itertools.product((0, 1, 2), (1, 2)):
                r3, r4 = pr.phase_ref(S, recs, 3, mm, w), pr.phase_ref(S, recs, 4, mm, w)
                assert (r3[0] == r4[0]).all() and (r3[1] == r4[1]).all() and r4[2]["n_flipped_last"] == 0, (o0, M, w, mm)
                n += 1
    assert n == 9 * 81 * 6


def test_apply():
    labels = [1, 0, -1, 1, 0]
    assert pr.apply(labels, True) == [0, 1, 3, 4] and pr.apply(labels, False) == [0, 3] and pr.apply([], True) == []


def test_engine_apply_is_the_reference_apply():
    from pacbioassembly_amd import engine as eng
    rows = np.zeros(5, eng.STRAND_OVERLAP_DTYPE)
    rows["target"], rows["query"], rows["cost"] = 7, np.arange(5) + 10, np.arange(5)
    ph = np.zeros(5, eng.PHASE_ROW_DTYPE)
    ph["label"] = [1, 0, -1, 1, 0]
    for keep in (True, False):
        got = eng.phase_rows_apply(rows, ph, keep)
        assert got.tobytes() == rows[pr.apply(ph["label"], keep)].tobytes()
    assert eng.phase_rows_apply(rows[:0], ph[:0]).size == 0
    with pytest.raises(eng.PbaError):
        eng.phase_rows_apply(rows, ph[:4])


# ----------------------------------------------------------------------------- the planted input
# What the reference rule yields on phase_ref.PLANTED under phase_ref.PARAMS; the input is deterministic, so
# these are asserted with no margin.
PLANTED_ROWS, PLANTED_DECIDED, PLANTED_RIGHT = 10467, 9122, 8815


def test_planted_input_end_to_end(oracle):
    """160 reads of two haplotypes, all-vs-all on both strands, every read a target: the decided rows fall on the side hap_of
    gives, and phased correction leaves strictly fewer (read, planted site) pairs on the other haplotype's allele than plain"""
    from conftest import MASK_PAT
    from correct_helpers import oracle_rows
    from pacbioassembly_amd import engine as eng
    D = pr.PLANTED
    h0, h1, reads, hap_of, planted = sr.planted_diploid(D)
    assert len(planted) >= 90 and {k for k, _, _ in planted.values()} == {"sub", "del"}
    mask = eng.mask_from_pattern(MASK_PAT)
    rows = oracle_rows(oracle, reads, mask, D["R"], 32, D["overlap_min"])
    assert {int(s) for s in rows["strand"]} == {1, -1}
    per = [[] for _ in reads]
    for r in rows:
        per[int(r["target"])].append(r)
    out = [pr.correct_phased_ref(oracle, reads, t, per[t], D["weight"], D["R"], D["thresholds"], pr.PARAMS) for t in range(len(reads))]
    decided = right = 0
    for t, o in enumerate(out):
        assert len(o["kept"]) == int((o["labels"] >= 0).sum())
        for k, r in enumerate(per[t]):
            lab = int(o["labels"][k])
            decided += lab != 0
            right += lab != 0 and (lab > 0) == (hap_of[int(r["query"])] == hap_of[t])
    print("rows", rows.size, "decided", decided, "on hap_of's side", right, f"({100.0 * right / decided:.2f} %)", "undecided", rows.size - decided,
          f"({100.0 * (rows.size - decided) / rows.size:.2f} %)")
    plain = pr.wrong_pairs(oracle, h0, [o["plain"] for o in out], hap_of, planted, mask, D["R"])
    phased = pr.wrong_pairs(oracle, h0, [o["text"] for o in out], hap_of, planted, mask, D["R"])
    print("(read, planted site) pairs on the other haplotype's allele: plain", plain, "phased", phased)
    assert plain[1] >= 20 * len(planted) and phased[1] >= 20 * len(planted)
    assert phased[0] < plain[0]
    assert (int(rows.size), decided, right) == (PLANTED_ROWS, PLANTED_DECIDED, PLANTED_RIGHT)
