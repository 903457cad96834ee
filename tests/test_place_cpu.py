"""tests/place_ref.py -- the placement rule of DESIGN §5.7 in plain Python, the expectation pba_layout_place is held to on the
device (tests/test_gpu_place.py) -- pinned without a GPU: on error-free tilings, where a correct placement makes contig and
read agree element for element, and on cases computed by hand.  pba_place_row_pair (host arithmetic of libpba.so) is checked
against the same arithmetic in Python, and the seed of the noisy GPU case is chosen here from the CPU oracle alone."""
import collections
import ctypes as C

import numpy as np
import pytest

from conftest import MASK_PAT
from correct_helpers import oracle_rows
from layout_ref import CONTAINED, PLACED, layout_ref, make_rows
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PAIR_DTYPE, PLACE_ROW_DTYPE, PbaError
from place_ref import (EDGE_LEN, EDGE_PLACES, HAND_LAY_ROWS, HAND_LENS, HAND_PLACE, HAND_TABLE, NOISY_SEED, OVERLAP_MIN, PLACE_COUNTERS,
                       PLACE_FIELDS, R, accessors_agree, edge_case, hand_placements, hand_texts, make_place_rows, noisy_conditions,
                       noisy_reads, oracle_vote_placed, pair_texts, place_pair, place_ref, place_tilings)


def test_every_placement_on_the_tilings_is_exact(lib):
    """40 seeds of three error-free tilings each (2 .. 39 reads of 40 .. 199 bases, steps 1 .. 59, min_ov 1 .. 29, dir drawn
    per row): for every placement the contig from pos and the read text from j agree element for element over the shorter
    accessor, in the direction the placement says; no accessor is empty.  All eight classes (target orient x row strand x
    row dir) occur among the winning rows, and PLACED as well as CONTAINED queries are placed."""
    classes, by_state, n_reads, n_found = collections.Counter(), collections.Counter(), 0, 0
    for seed in range(40):
        texts, rows = place_tilings(seed)
        lens = [len(x) for x in texts]
        lay = layout_ref(lens, rows, 64, 2, texts)
        places, st = place_ref(lens, lay["table"], rows)
        assert st["n_target_not_placed"] + st["n_outside"] + st["n_eligible"] == st["n_rows"] == len(rows)
        assert st["n_found"] == sum(p[1] for p in places) == st["n_found_placed"] + st["n_found_contained"] + st["n_found_unplaced"]
        n_reads += len(texts)
        for p in places:
            if not p[1]:
                assert p == (p[0], 0, 0, -1, 0, 0, 0, 0)
                continue
            n_found += 1
            row = rows[p[2]]
            assert int(row["query"]) == p[0]
            a, b = accessors_agree(p, lay["texts"][p[3]], texts[p[0]])
            assert len(a) > 0 and a == b, (seed, p)
            classes[(lay["table"][int(row["target"])][4], int(row["strand"]), int(row["dir"]))] += 1
            by_state[lay["table"][p[0]][1]] += 1
    print("reads", n_reads, "placements", n_found, "by state", dict(by_state), "classes", dict(classes))
    assert set(classes) == {(o, s, d) for o in (0, 1) for s in (1, -1) for d in (1, -1)}
    assert by_state[PLACED] > 100 and by_state[CONTAINED] > 100


def test_hand_layout_is_the_table_written_out(lib):
    got = layout_ref(HAND_LENS, make_rows(HAND_LAY_ROWS), 64, 2)
    assert got["table"] == HAND_TABLE and got["contigs"] == [(0, 3, 190)]


@pytest.mark.parametrize("case", HAND_PLACE, ids=[c["name"] for c in HAND_PLACE])
def test_reference_on_hand_cases(lib, case):
    """Ties, the cost clamps, anchors one base outside and on both edges of the supplied part for both orientations, targets
    that are not PLACED, queries of every state and a query without an eligible row: expected placements and counters are
    written out in place_ref.HAND_PLACE with their arithmetic."""
    places, st = place_ref(HAND_LENS, HAND_TABLE, make_place_rows(case["rows"]))
    assert places == hand_placements(case)
    assert st == case["stats"]


def test_hand_placements_down_to_the_bases(lib):
    """The rows of the hand cases are not overlaps of any texts; here reads 3 .. 5 are made so that they are: the contig is
    r0 + rc(r1)[60:] + r2[50:], and each query is copied from the contig around its anchor."""
    from layout_ref import rc
    t = hand_texts()
    contig = t[0] + rc(t[1])[60:] + t[2][50:]
    # read 4 is contig [90, 190) as it stands.  The contig holds rc(r1)[60, 100) at [100, 140), so r1[0, 40) = rc(contig[100, 140))
    # = rc(r4[10, 50)) = rc(r4)[50, 90): a strand -1 row of target 1 and query 4
    r4 = contig[90:190]
    row = (1, 4, -1, 0, 0, 40, 100 - 90, 100 - 50, 1)             # walked rc(r4) [50, 90); forward on r4: [10, 50)
    assert t[1][0:40] == rc(r4)[50:90]
    places, _ = place_ref(HAND_LENS, HAND_TABLE, make_place_rows([row]))
    # anchor t_beg 0 -> rc(t) index 99 -> pos 100 + 99 - 60 = 139; yb = 50 -> j' = 99 - 50 = 49 in r4 as given, backward
    assert places[4] == (4, 1, 0, 0, 139, -1, 1, 49)
    a, b = accessors_agree(places[4], contig, r4)
    assert a == b and len(a) == 50


def row_of(p):
    r = np.zeros(1, PLACE_ROW_DTYPE)[0]
    for f, v in zip(PLACE_FIELDS, p):
        r[f] = v
    return r


def test_place_row_pair_through_the_library(lib):
    """pba_place_row_pair against place_ref.place_pair on every hand placement, every edge placement and a sweep of
    positions around the clip; then its refusals."""
    cases = [(p, 190, HAND_LENS[p[0]]) for c in HAND_PLACE for p in hand_placements(c) if p[1]]
    _, reads, places = edge_case()
    cases += [(p, EDGE_LEN, len(reads[p[0]])) for p in places]
    for pos in (0, 1, 63, 64, 1000, 1299, 1300, 1301, 1999):
        for d in (1, -1):
            for j in (0, 1, 500, 998, 999):
                cases.append(((7, 1, 3, 2, pos, d, -1, j), 2000, 1000))
    for p, cl, rl in cases:
        got = eng.place_row_pair(row_of(p), cl, rl, R)
        assert tuple(int(got[k]) for k in PAIR_DTYPE.names) == place_pair(p, cl, rl, R), p
    # spelled out: forward from (pos 100, j 10) of a 1 000-base read on a 5 000-base contig: b 990, a = 990 + 1 + 297
    got = eng.place_row_pair(row_of((3, 1, 0, 2, 100, 1, 1, 10)), 5000, 1000, 0.30)
    assert tuple(int(got[k]) for k in PAIR_DTYPE.names) == (2, 100, 1288, 3, 10, 990, 0)
    # backward from (pos 100, j 989): b 990, the contig has 101 bases left
    got = eng.place_row_pair(row_of((3, 1, 0, 2, 100, -1, -1, 989)), 5000, 1000, 0.30)
    assert tuple(int(got[k]) for k in PAIR_DTYPE.names) == (2, 100, 101, 3, 989, 990, 3)

    def status(p, cl=2000, rl=1000, R=0.30):
        with pytest.raises(PbaError) as e:
            eng.place_row_pair(row_of(p), cl, rl, R)
        return e.value.status

    good = (7, 1, 3, 2, 100, 1, 1, 10)
    eng.place_row_pair(row_of(good), 2000, 1000, 0.30)
    assert status((7, 0, 0, -1, 0, 0, 0, 0)) == -1                                            # not found
    assert status(good[:5] + (0,) + good[6:]) == -1 and status(good[:5] + (2,) + good[6:]) == -1      # dir
    assert status(good[:6] + (0, 10)) == -1 and status(good[:6] + (-2, 10)) == -1             # strand
    assert status(good[:4] + (2000,) + good[5:]) == -1 and status(good[:4] + (-1,) + good[5:]) == -1  # pos outside
    assert status(good[:7] + (1000,)) == -1 and status(good[:7] + (-1,)) == -1                # j outside
    assert status(good[:3] + (-1,) + good[4:]) == -1 and status((-1,) + good[1:]) == -1       # contig, read
    assert status(good, R=0.0) == -1 and status(good, R=1.0) == -1
    eng.place_row_pair(row_of(good[:4] + (1999,) + good[5:]), 2000, 1000, 0.30)               # the last legal positions
    eng.place_row_pair(row_of(good[:7] + (999,)), 2000, 1000, 0.30)
    assert status((7, 1, 3, 2, 0, 1, 1, 0), cl=200000, rl=65001) == -4                        # b beyond the engine's limit
    assert status((7, 1, 3, 2, 199999, -1, 1, 65000), cl=200000, rl=65001) == -4
    eng.place_row_pair(row_of((7, 1, 3, 2, 0, 1, 1, 1)), 60000, 65001, 0.30)                  # b of 65 000, a the contig's 60 000
    assert status((7, 1, 3, 2, 0, 1, 1, 1), cl=200000, rl=65001) == -4                        # a = 65 000 + 19 501 after the clip
    r, out = np.zeros(1, PLACE_ROW_DTYPE), np.zeros(1, PAIR_DTYPE)
    r[0] = row_of(good)
    assert lib.pba_place_row_pair(None, 2000, 1000, 0.3, C.c_void_p(out.ctypes.data)) == -1
    assert lib.pba_place_row_pair(C.c_void_p(r.ctypes.data), 2000, 1000, 0.3, None) == -1
    assert lib.pba_place_row_pair(C.c_void_p(r.ctypes.data), 2000, 1000, 0.3, C.c_void_p(out.ctypes.data)) == 0


def test_a_forward_placement_makes_the_pair_of_its_map_row(lib):
    """pba_map_row_pair and pba_place_row_pair with dir = +1 on the same anchor: equal in every field of the pair, flags 0,
    at the first, second and last base of the contig, the first and last of the read, both strands, a contig shorter and
    longer than the read and the 200 000 / 40 000 clip case of test_polish_cpu.py; and the same status for the same bad input."""
    def both(pos, j, cl, rl, R, strand=1, found=1):
        """("ok", pair) or ("refused", status) from each of the two functions"""
        anchor = dict(read=5, found=found, contig=2, pos=pos, strand=strand, j=j)
        got = []
        for fn, row in ((eng.map_row_pair, anchor), (eng.place_row_pair, dict(anchor, row=9, dir=1))):
            try:
                pair = fn(row, cl, rl, R)
                got.append(("ok", tuple(int(pair[k]) for k in PAIR_DTYPE.names)))
            except PbaError as e:
                got.append(("refused", e.status))
        return got

    n = 0
    for cl, rl in ((1, 1), (2000, 1000), (1000, 2000), (200000, 40000)):
        for R in (0.05, 0.30):
            for strand in (1, -1):
                for pos in sorted({p for p in (0, 1, cl - 1) if p < cl}):
                    for j in sorted({0, rl - 1}):
                        m, p = both(pos, j, cl, rl, R, strand)
                        assert m[0] == "ok" and m == p and m[1][-1] == 0, (cl, rl, R, strand, pos, j, m, p)
                        assert m[1][:2] == (2, pos) and m[1][3:6] == (5, j, rl - j), m
                        n += 1
    assert n == 2 * 2 * (1 + 3 * 2 * 3)
    # the clip itself: 40 000 read bases from the contig's first base take 40 000 + 1 + 12 000 of its 200 000
    assert both(0, 0, 200000, 40000, 0.30)[0] == ("ok", (2, 0, 52001, 5, 0, 40000, 0))
    for bad, want in ((dict(pos=2000, j=10), -1), (dict(pos=100, j=1000), -1), (dict(pos=100, j=10, R=0.0), -1),
                      (dict(pos=100, j=10, R=1.0), -1), (dict(pos=100, j=10, found=0), -1),
                      (dict(pos=0, j=0, cl=200000, rl=65001), -4)):
        args = dict(dict(cl=2000, rl=1000, R=0.30), **bad)
        assert both(**args) == [("refused", want)] * 2, bad


def test_edge_case_is_exact_and_meets_its_conditions(lib, oracle):
    """The hand-made placements of the 70 001-base contig (place_ref.EDGE_PLACES): every one is exact, and the oracle votes
    all but the two that leave the contig 41 bases."""
    T, reads, places = edge_case()
    for p in places:
        a, b = accessors_agree(p, T, reads[p[0]])
        assert len(a) > 0 and a == b, p
    _, res, voted = oracle_vote_placed(oracle, [T], reads, places, 0)
    failing = [k for k, o in res.items() if not (o["rc"] >= 0 and o["matlen_a"] >= OVERLAP_MIN)]
    assert failing == [14, 15] and voted == len(places) - 2
    assert sum(p[4] > 65535 for p in places) >= 4 and {p[4] for p in places} >= {4095, 4096, 8191}


def test_noisy_case_meets_its_conditions(lib, oracle):
    """The seed of tests/test_gpu_place.py's noisy input (200 reads of 600 - 1 500 bases at 12 % error, both strands), judged
    from the CPU oracle alone: its rows (correct_helpers.oracle_rows: what pba_overlap_strands is specified to return), the
    layout and placement references and the oracle's aligner.  At least 5 voting placements in each (dir', strand') class,
    a voting CONTAINED read, a found placement that fails the gate."""
    texts = noisy_reads(NOISY_SEED)
    rows = oracle_rows(oracle, texts, eng.mask_from_pattern(MASK_PAT))
    cond, lay, places, st = noisy_conditions(oracle, texts, rows)
    print("seed", NOISY_SEED, "rows", len(rows), cond, st)
    assert all(600 <= len(x) <= 1500 for x in texts)
    assert all(v >= 5 for v in cond["voted"].values()), cond
    assert cond["voted_contained"] >= 1 and cond["found_not_voted"] >= 1, cond
