"""Placement of reads on their laid-out contigs and the consensus voted from it, on the device (pba_layout_place,
pba_pileup_vote_placed, pba_layout_consensus).  Placements and counters must be IDENTICAL to tests/place_ref.py,
the rule restated sequentially (tests/test_place_cpu.py pins that reference by hand and on tilings where a correct placement
is exact); boxes, results and texts are held to the CPU oracle composed the same way, box for box and byte for byte.  Needs a
real MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

from conftest import MASK_PAT
from layout_ref import ACGT, CONTAINED, PLACED, ROW_FIELDS, combine, layout_ref, make_rows, tiling
from pacbioassembly_amd import Pileup
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PLACE_ROW_DTYPE, PbaError
from place_ref import (EDGE_LEN, HAND_LAY_ROWS, HAND_LENS, HAND_PLACE, HAND_TABLE, NOISY_SEED, OVERLAP_MIN, PLACE_COUNTERS, PLACE_FIELDS,
                       R, check_result, edge_case, fuzz_rows, hand_placements, hand_texts, make_place_rows, noisy_reads,
                       oracle_boxes, oracle_consensus, oracle_evolve, oracle_vote_placed, place_ref, place_tilings)
from polish_helpers import PileupAs

pytestmark = pytest.mark.gpu


def texts_of(S):
    return [S.get_text(i) for i in range(S.count)]


def as_tuples(rows, fields):
    return [tuple(int(r[f]) for f in fields) for r in rows]


def check_place(lay, S, lens, rows, table=None):
    """Placements and counters of the device == the reference over the device's own table.  Returns (placements, counters)."""
    table = as_tuples(lay.rows(), ROW_FIELDS) if table is None else table
    want, st = place_ref(lens, table, rows)
    got = lay.place(S, rows)
    assert got.dtype == PLACE_ROW_DTYPE and as_tuples(got, PLACE_FIELDS) == want
    assert {k: int(lay.place_stats[k]) for k in PLACE_COUNTERS} == st
    assert lay.place_stats["place_ms"] > 0
    return got, st


@pytest.fixture(scope="module")
def hand(ctx):
    texts = hand_texts()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    lay = ctx.layout(S, make_rows(HAND_LAY_ROWS), 64, 2)
    assert as_tuples(lay.rows(), ROW_FIELDS) == HAND_TABLE
    return S, lay


@pytest.mark.parametrize("case", HAND_PLACE, ids=[c["name"] for c in HAND_PLACE])
def test_hand_cases(ctx, hand, case):
    """Rows written by hand (tests/place_ref.py: HAND_PLACE, with the arithmetic next to each)."""
    S, lay = hand
    got, st = check_place(lay, S, HAND_LENS, make_place_rows(case["rows"]))
    assert as_tuples(got, PLACE_FIELDS) == hand_placements(case) and st == case["stats"]


def test_tilings(ctx):
    """The 40 tilings of tests/test_place_cpu.py (all eight classes of target orient x strand x dir, PLACED and CONTAINED
    queries): 2 691 reads, 2 370 placements."""
    found = 0
    for seed in range(40):
        texts, rows = place_tilings(seed)
        S = ctx.seqs_from_list(texts, strict_acgt=True)
        lay = ctx.layout(S, rows, 64, 2)
        _, st = check_place(lay, S, [len(x) for x in texts], rows)
        found += st["n_found"]
        lay.close()
    assert found == 2370


@pytest.fixture(scope="module")
def fuzz(ctx):
    """2 000 reads of 50 - 300 bases under a layout of 20 000 random rows; its table once."""
    rng = np.random.default_rng(331)
    lens = [int(n) for n in rng.integers(50, 301, 2000)]
    texts = [rng.choice(ACGT, n).tobytes() for n in lens]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    lay = ctx.layout(S, fuzz_rows(rng, lens, 20000), 64, 2)
    return dict(rng=rng, lens=lens, S=S, lay=lay, table=as_tuples(lay.rows(), ROW_FIELDS))


def test_fuzz_random_rows(ctx, fuzz):
    """20 000 random valid rows of both directions, not the layout's own, costs beyond both clamps among them; then 20 000
    whose targets are all PLACED, so that every query has several eligible rows: any disagreement between the atomicMax and
    the sequential pick shows here."""
    rows = fuzz_rows(fuzz["rng"], fuzz["lens"], 20000)
    _, st = check_place(fuzz["lay"], fuzz["S"], fuzz["lens"], rows, fuzz["table"])
    assert st["n_target_not_placed"] > 1000 and st["n_outside"] > 1000 and st["n_eligible"] > 1000
    assert min(st["n_found_placed"], st["n_found_contained"], st["n_found_unplaced"]) > 20
    placed = [r for r, row in enumerate(fuzz["table"]) if row[1] == PLACED]
    rows = fuzz_rows(fuzz["rng"], fuzz["lens"], 20000, targets=placed)
    _, st = check_place(fuzz["lay"], fuzz["S"], fuzz["lens"], rows, fuzz["table"])
    assert st["n_target_not_placed"] == 0 and st["n_eligible"] > 3 * st["n_found"] > 3000


@pytest.mark.parametrize("n_rows", [0, 1, 63, 64, 65, 255, 256, 257])
def test_row_counts_at_wavefront_and_block_edges(ctx, fuzz, n_rows):
    """The counters take one atomic per wavefront: row counts around one wavefront and one workgroup."""
    rows = fuzz_rows(np.random.default_rng(332), fuzz["lens"], 257)[:n_rows]
    _, st = check_place(fuzz["lay"], fuzz["S"], fuzz["lens"], rows, fuzz["table"])
    assert st["n_rows"] == n_rows


def test_empty_set(ctx):
    S = ctx.seqs_from_list([], strict_acgt=True)
    lay = ctx.layout(S, make_rows([]), 64, 1)
    got = lay.place(S, make_rows([]))
    assert got.size == 0 and {k: int(lay.place_stats[k]) for k in PLACE_COUNTERS} == dict.fromkeys(PLACE_COUNTERS, 0)
    out, rows_out, st = ctx.layout_consensus(lay, S, make_rows([]), R)
    assert out.count == 0 and rows_out.size == 0 and st["n_chunks"] == 0 and st["n_voted"] == 0


# ----------------------------------------------------------------------------- the vote
@pytest.fixture(scope="module")
def noisy(ctx, oracle):
    """200 reads of 600 - 1 500 bases at 12 % error on both strands (tests/test_place_cpu.py chose the seed), the rows of the
    engine's own overlapper, their layout, the stitched contigs, the placements, and the oracle's vote per contig."""
    texts = noisy_reads(NOISY_SEED)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, eng.mask_from_pattern(MASK_PAT), R, 32, 64, reads_rc=Src)
    lay = ctx.layout(S, rows, 64, 2)
    contigs = lay.stitch(S)
    ctexts = texts_of(contigs)
    places, _ = check_place(lay, S, [len(x) for x in texts], rows)
    want = [oracle_vote_placed(oracle, ctexts, texts, as_tuples(places, PLACE_FIELDS), c) for c in range(len(ctexts))]
    return dict(texts=texts, S=S, Src=Src, rows=rows, lay=lay, table=lay.rows(), contigs=contigs, ctexts=ctexts, places=places, want=want)


def test_votes_vs_oracle_noisy(ctx, noisy):
    places, ctexts = noisy["places"], noisy["ctexts"]
    pile = Pileup(ctx, noisy["contigs"])
    res, n_voted = pile.vote_placed(noisy["S"], places, R, OVERLAP_MIN, reads_rc=noisy["Src"])
    voted = {(d, s): 0 for d in (1, -1) for s in (1, -1)}
    contained = not_voted = seen = 0
    for c, (cons, want_res, _) in enumerate(noisy["want"]):
        for k, o in want_res.items():
            check_result(res[k], o, (c, k))
            seen += 1
            if o["rc"] >= 0 and o["matlen_a"] >= OVERLAP_MIN:
                voted[(int(places[k]["dir"]), int(places[k]["strand"]))] += 1
                contained += int(noisy["table"][k]["state"]) == CONTAINED
            else:
                not_voted += 1
        for x, y, name in zip(pile.dump(c), oracle_boxes(cons, len(ctexts[c])), ("sel", "sup", "tot")):
            assert x.shape == y.shape and (x == y).all(), (c, name)
    print("voted per (dir, strand):", voted, "contained:", contained, "found but not voted:", not_voted)
    assert seen == int(places["found"].sum())
    assert min(voted.values()) >= 5 and contained >= 1 and not_voted >= 1       # the input exercises what it is meant to
    for k in np.flatnonzero(places["found"] == 0):
        assert int(res[k]["rc"]) == -1 and not any(int(res[k][f]) for f in res.dtype.names if f != "rc"), k
    assert n_voted == sum(voted.values()) == sum(w[2] for w in noisy["want"])
    _, crows = pile.evolve()
    assert [int(x) for x in crows["n_rows"]] == [w[2] for w in noisy["want"]]


def test_votes_vs_oracle_hand_placements_on_a_long_contig(ctx, oracle):
    """Placement rows written by hand on a contig of 70 001 bases (the tiled pile-up kernels), every read an exact copy around
    its anchor (tests/place_ref.py: EDGE_PLACES): forward and backward from positions beyond 65 535, from the tile edges
    4 095, 4 096 and 8 191, backward off base 0 and forward off the last base, and two that leave the contig 41 bases."""
    T, reads, places = edge_case()
    S = ctx.seqs_from_list([T], strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    Rc = ctx.seqs_revcomp(Rd)
    rows = np.zeros(len(places), PLACE_ROW_DTYPE)
    for k, p in enumerate(places):
        rows[k] = p
    cons, want_res, want_voted = oracle_vote_placed(oracle, [T], reads, places, 0)
    assert want_voted == len(places) - 2
    pile = Pileup(ctx, S)
    res, n_voted = pile.vote_placed(Rd, rows, R, OVERLAP_MIN, reads_rc=Rc)
    assert n_voted == want_voted
    for k, o in want_res.items():
        check_result(res[k], o, k)
    for x, w, name in zip(pile.dump(0), oracle_boxes(cons, EDGE_LEN), ("sel", "sup", "tot")):
        assert x.shape == w.shape and (x == w).all(), name
    out, crows = pile.evolve()
    assert out.get_text(0) == oracle_evolve(cons, EDGE_LEN) and int(crows[0]["n_rows"]) == want_voted


@pytest.fixture(scope="module")
def noisy_consensus(oracle, noisy):
    return oracle_consensus(oracle, noisy["ctexts"], noisy["texts"], as_tuples(noisy["places"], PLACE_FIELDS))


@pytest.mark.parametrize("max_boxes", [0, 1])
def test_consensus_vs_composed_loop(ctx, noisy, noisy_consensus, max_boxes):
    """pba_layout_consensus == stitch, Pileup, vote_placed, evolve composed here == the oracle's evolve, byte for byte; with
    max_boxes = 1 every range holds exactly one contig."""
    want_texts, want_voted = noisy_consensus
    pile = Pileup(ctx, noisy["contigs"])
    pile.vote_placed(noisy["S"], noisy["places"], R, OVERLAP_MIN, reads_rc=noisy["Src"])
    composed, _ = pile.evolve()
    assert texts_of(composed) == want_texts
    out, rows_out, st = ctx.layout_consensus(noisy["lay"], noisy["S"], noisy["rows"], R, OVERLAP_MIN, 1, max_boxes)
    got = texts_of(out)
    assert got == want_texts and sum(t != c for t, c in zip(got, noisy["ctexts"])) * 2 >= len(got)
    nc = len(want_texts)
    assert as_tuples(rows_out, ("contig", "n_rows", "len_in", "len_out")) == \
           [(c, want_voted[c], len(noisy["ctexts"][c]), len(want_texts[c])) for c in range(nc)]
    assert {k: int(st[k]) for k in PLACE_COUNTERS} == {k: int(noisy["lay"].place_stats[k]) for k in PLACE_COUNTERS}
    assert st["n_voted"] == sum(want_voted) and st["n_contigs"] == nc and st["n_chunks"] == (nc if max_boxes else 1)
    assert st["n_bases_in"] == sum(len(t) for t in noisy["ctexts"]) and st["n_bases_out"] == sum(len(t) for t in want_texts)
    assert min(st[k] for k in ("stitch_ms", "place_ms", "vote_ms", "evolve_ms")) > 0
    assert texts_of(noisy["contigs"]) == noisy["ctexts"]                        # (the stitched set of the fixture is its own)


def test_consensus_of_an_error_free_tiling_is_the_stitched_set(ctx):
    rng = np.random.default_rng(341)
    tilings = [tiling(rng, [300] * n, rng.integers(60, 200, n - 1), min_ov=64) for n in (2, 9, 30)]
    texts, rows, _ = combine(rng, tilings)
    rows["dir"] = rng.choice((1, -1), rows.size)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    lay = ctx.layout(S, rows, 64, 2)
    want = layout_ref([len(x) for x in texts], rows, 64, 2, texts)["texts"]
    for max_boxes in (0, 1):
        out, rows_out, st = ctx.layout_consensus(lay, S, rows, R, OVERLAP_MIN, 1, max_boxes)
        assert texts_of(out) == want and len(want) == 3
        assert st["n_voted"] > 20 and int(rows_out["n_rows"].sum()) == st["n_voted"]


def test_refusals(ctx, hand, noisy):
    """Every refusal gives its status and leaves what it was called on usable."""
    S, lay = hand

    def status(call):
        with pytest.raises(PbaError) as e:
            call()
        return e.value.status

    good = HAND_PLACE[0]["rows"]
    for bad_dir in (0, 2, -2):
        assert status(lambda: lay.place(S, make_place_rows(good + [good[0][:8] + (bad_dir,)]))) == -1
    assert status(lambda: lay.place(S, make_place_rows([(0, 0, 1, 0, 0, 10, 0, 10, 1)]))) == -1           # target == query
    assert status(lambda: lay.place(S, make_place_rows([(0, 6, 1, 0, 0, 10, 0, 10, 1)]))) == -1           # outside the set
    assert status(lambda: lay.place(S, make_place_rows([(0, 3, 1, 0, 0, 10, 0, 51, 1)]))) == -1           # interval beyond its read
    t = hand_texts()
    for other in (t[:-1], t[:-1] + [t[-1][:-1]], t + [b"ACGT"]):                                        # another count, other lengths
        assert status(lambda: lay.place(ctx.seqs_from_list(other, strict_acgt=True), make_place_rows(good))) == -1
    out, rows = np.zeros(6, PLACE_ROW_DTYPE), make_place_rows(good)
    assert ctx.lib.pba_layout_place(ctx.h, lay.h, S.h, C.c_void_p(rows.ctypes.data), rows.size, C.c_void_p(out.ctypes.data), 5, None) == -1
    check_place(lay, S, HAND_LENS, make_place_rows(good))

    contigs, Rd, Rc, places = noisy["contigs"], noisy["S"], noisy["Src"], noisy["places"]
    found = places[places["found"] == 1]
    minus = found[found["strand"] == -1]
    nc = contigs.count
    pile = Pileup(ctx, contigs, t_lo=1, t_hi=nc)
    before = pile.dump(1)
    inside = found[found["contig"] >= 1]
    outside = inside[:8].copy()
    outside["contig"][5] = 0                                                      # good rows first, then one outside [1, nc)
    assert status(lambda: pile.vote_placed(Rd, outside, R, OVERLAP_MIN, reads_rc=Rc)) == -1
    assert status(lambda: pile.vote_placed(Rd, minus[minus["contig"] >= 1][:3], R, OVERLAP_MIN)) == -1   # strand -1 without reads_rc
    bad = inside[:3].copy()
    bad["dir"][1] = 0
    assert status(lambda: pile.vote_placed(Rd, bad, R, OVERLAP_MIN, reads_rc=Rc)) == -1
    other = ctx.seqs_from_list([c + b"A" for c in noisy["ctexts"]], strict_acgt=True)
    assert status(lambda: Pileup.vote_placed(PileupAs(pile, other), Rd, inside[:3], R, OVERLAP_MIN, reads_rc=Rc)) == -1   # not the pile-up's set
    loose = ctx.seqs_from_list([r[:50] + b"N" + r[51:] for r in noisy["texts"]], strict_acgt=False)
    assert status(lambda: pile.vote_placed(loose, inside[:3], R, OVERLAP_MIN, reads_rc=Rc)) == -6         # bytes outside ACGT
    for x, y in zip(before, pile.dump(1)):
        assert (x == y).all()                                                     # host-side refusals leave the boxes alone
    assert status(lambda: ctx.layout_consensus(noisy["lay"], loose, noisy["rows"], R)) == -6
    assert status(lambda: ctx.layout_consensus(noisy["lay"], Rd, noisy["rows"], R, weight=0)) == -1
    pile.evolve()
    assert status(lambda: pile.vote_placed(Rd, inside[:3], R, OVERLAP_MIN, reads_rc=Rc)) == -1            # spent
