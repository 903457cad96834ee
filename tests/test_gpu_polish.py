"""Contig polishing on the device (pba_pileup_vote_mapped, the tiled pile-up kernels, pba_polish_contigs): the reads
pba_map_reads places on a contig vote on it with the roles of the mapper's alignment swapped, evolve gives the next contig.
Held to the CPU oracle composed the same way (tests/polish_helpers.py), box for box and byte for byte.  Needs a real MI355X
(-m gpu)."""
import numpy as np
import pytest

from conftest import MASK_PAT
from map_ref import rand_text
from pacbioassembly_amd import Pileup
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PLACE_ROW_DTYPE, PbaError
from polish_helpers import (EDGE_DEL, EDGE_INS, OVERLAP_MIN, POLISH_LENS, R, TILE, PileupAs, check_result, edge_case, oracle_boxes,
                            oracle_evolve, oracle_polish_round, oracle_vote, polish_case, yields)

pytestmark = pytest.mark.gpu
LONG = POLISH_LENS.index(70001)


def texts_of(S):
    return [S.get_text(i) for i in range(S.count)]


def map_rows(ctx, T, Rd, strands=3, reads_rc=None):
    ix = ctx.index_build_set(T, eng.mask_from_pattern(MASK_PAT))
    rows, _ = ctx.map_reads(ix, T, Rd, R, strands=strands, reads_rc=reads_rc)
    ix.close()
    return rows


@pytest.fixture(scope="module")
def case(ctx):
    """The input of the vote and driver tests on the device, with its map_reads rows (pinned by tests/test_gpu_map.py)."""
    contigs, reads = polish_case(701)
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    Rc = ctx.seqs_revcomp(Rd)
    return dict(contigs=contigs, reads=reads, T=T, Rd=Rd, Rc=Rc, rows=map_rows(ctx, T, Rd, reads_rc=Rc))


@pytest.fixture(scope="module")
def round1(oracle, case):
    """The oracle's vote of the case's rows, per contig: (consensus object before evolve, {row: result}, rows voted)."""
    return [oracle_vote(oracle, case["contigs"], case["reads"], case["rows"], c) if n else None for c, n in enumerate(POLISH_LENS)]


def test_votes_vs_oracle(ctx, case, round1):
    rows, contigs = case["rows"], case["contigs"]
    pile = Pileup(ctx, case["T"])
    res, n_voted = pile.vote_mapped(case["Rd"], rows, R, OVERLAP_MIN, reads_rc=case["Rc"])
    voted = {1: 0, -1: 0}
    not_voted = far = seen = 0
    for c, want in enumerate(round1):
        if want is None:
            continue
        for k, o in want[1].items():
            check_result(res[k], o, (c, k))
            seen += 1
            if o["rc"] >= 0 and o["matlen_a"] >= OVERLAP_MIN:
                voted[int(rows[k]["strand"])] += 1
                far += int(rows[k]["pos"]) > 65535
            else:
                not_voted += 1
        got = pile.dump(c)
        for x, y, name in zip(got, oracle_boxes(want[0], len(contigs[c])), ("sel", "sup", "tot")):
            assert x.shape == y.shape and (x == y).all(), (c, name)
    print("voted per strand:", voted, "found but not voted:", not_voted, "voted beyond 65 535:", far)
    assert seen == int(rows["found"].sum())
    assert voted[1] > 0 and voted[-1] > 0 and not_voted > 0 and far > 0          # the input exercises what it is meant to
    for k in np.flatnonzero(rows["found"] == 0):
        assert int(res[k]["rc"]) == -1 and not any(int(res[k][f]) for f in res.dtype.names if f != "rc"), k
    assert n_voted == voted[1] + voted[-1] == sum(w[2] for w in round1 if w)
    _, crows = pile.evolve()
    assert [int(x) for x in crows["n_rows"]] == [w[2] if w else 0 for w in round1]


def test_placements_vote_as_the_mapped_rows_they_restate(ctx, case):
    """The case's rows as placement rows (same read, found, contig, pos, strand and j; dir = +1; row = k) through vote_placed,
    against the rows themselves through vote_mapped on a second pile-up: results row by row (unfound rows included), rows
    voted, every contig's boxes, the evolved texts and the per-contig rows are identical."""
    rows = case["rows"]
    places = np.zeros(rows.size, PLACE_ROW_DTYPE)
    for f in ("read", "found", "contig", "pos", "strand", "j"):
        places[f] = rows[f]
    places["dir"] = 1
    places["row"] = np.arange(rows.size)
    mapped, placed = Pileup(ctx, case["T"]), Pileup(ctx, case["T"])
    res_m, voted_m = mapped.vote_mapped(case["Rd"], rows, R, OVERLAP_MIN, reads_rc=case["Rc"])
    res_p, voted_p = placed.vote_placed(case["Rd"], places, R, OVERLAP_MIN, reads_rc=case["Rc"])
    assert (rows["found"] == 0).any() and 0 < voted_m < int(rows["found"].sum())
    assert res_m.dtype == res_p.dtype and res_m.tobytes() == res_p.tobytes() and voted_m == voted_p
    for c in range(len(POLISH_LENS)):
        for x, y, name in zip(mapped.dump(c), placed.dump(c), ("sel", "sup", "tot")):
            assert x.shape == y.shape and (x == y).all(), (c, name)
    (out_m, crows_m), (out_p, crows_p) = mapped.evolve(), placed.evolve()
    assert texts_of(out_m) == texts_of(out_p) and crows_m.tobytes() == crows_p.tobytes() and crows_m["n_rows"].sum() == voted_m


@pytest.mark.parametrize("long_len", [65536, 65537, 70001, 200000])
def test_evolve_without_votes_returns_the_texts(ctx, long_len):
    """Up to 65 536 boxes in the longest segment the per-target kernels run, above that the tiled ones (one workgroup per
    4 096 boxes): short, empty and tile-sized segments next to the long one."""
    rng = np.random.default_rng(long_len)
    texts = [rand_text(rng, n) for n in (4097, long_len, 0, 1, 4095, 4096)]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    out, crows = Pileup(ctx, S, weight=2).evolve()
    assert texts_of(out) == texts
    assert [int(x) for x in crows["len_out"]] == [len(t) for t in texts] and not crows["n_rows"].any()


def test_tiled_evolve_with_votes_at_tile_edges(ctx, oracle):
    """Six exact reads over each site: an inserted base right after contig positions 4 095 and 8 191 (the last box of a tile
    yields two characters: the second lands in the next tile's text range), contig bases 12 287 + 12 288 and 16 384 missing
    (the last and the first box of a tile yield nothing).  The sites lie a tile apart: six reads of one site that also
    covered another would vote MATCH on its box and keep it (7 of 13 votes)."""
    T, reads = edge_case(711)
    S = ctx.seqs_from_list([T], strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    rows = map_rows(ctx, S, Rd, strands=1)
    assert rows["found"].all()
    cons, want_res, want_voted = oracle_vote(oracle, [T], reads, rows, 0)
    assert want_voted == len(reads)
    sel, sup, tot = oracle_boxes(cons, len(T))
    y = yields(sel, sup, tot)
    two, none = np.flatnonzero(y == 2), np.flatnonzero(y == 0)
    assert two.tolist() == list(EDGE_INS) and (two % TILE == TILE - 1).all()
    assert set(none.tolist()) >= {b for d in EDGE_DEL for b in d}             # (and a box where one read's alignment ends in a DELETE)
    assert (none % TILE == 0).any() and (none % TILE == TILE - 1).any()
    pile = Pileup(ctx, S)
    res, n_voted = pile.vote_mapped(Rd, rows, R, OVERLAP_MIN)
    assert n_voted == want_voted
    for k, o in want_res.items():
        check_result(res[k], o, k)
    for x, w, name in zip(pile.dump(0), (sel, sup, tot), ("sel", "sup", "tot")):
        assert (x == w).all(), name
    out, crows = pile.evolve()
    want = oracle_evolve(cons, len(T))
    assert len(want) == int(y.sum()) != len(T)
    assert out.get_text(0) == want and int(crows[0]["len_out"]) == len(want) and int(crows[0]["n_rows"]) == len(reads)


@pytest.fixture(scope="module")
def two_rounds(ctx, oracle, case):
    """The driver's loop composed from map_reads rows and the oracle's vote and evolve: per strands value, (texts after two
    rounds, rows voted per contig in the last round, input lengths of the last round, [(n_mapped, n_voted) per round])."""
    def run(strands):
        cur, log = case["contigs"], []
        for _ in range(2):
            T = case["T"] if cur is case["contigs"] else ctx.seqs_from_list(cur, strict_acgt=True)
            rows = map_rows(ctx, T, case["Rd"], strands=strands, reads_rc=case["Rc"])
            before = cur
            cur, voted = oracle_polish_round(oracle, cur, case["reads"], rows)
            log.append((int(rows["found"].sum()), sum(voted)))
        return cur, voted, [len(t) for t in before], log
    return {3: run(3), 1: run(1)}


@pytest.mark.parametrize("strands,max_boxes", [(3, 0), (3, 5000), (1, 0)])
def test_driver_vs_composed_loop(ctx, case, two_rounds, strands, max_boxes):
    want_texts, want_voted, want_in, want_log = two_rounds[strands]
    out, rows_out, log = ctx.polish_contigs(case["T"], case["Rd"], eng.mask_from_pattern(MASK_PAT), R, strands=strands,
                                            overlap_min=OVERLAP_MIN, weight=1, rounds=2, max_boxes=max_boxes)
    assert texts_of(case["T"]) == case["contigs"]                               # the caller's set is as it was
    got = texts_of(out)
    assert out.count == len(POLISH_LENS) and got[0] == b"" and got[1] == case["contigs"][1]   # ids stay; no rows: unchanged
    assert got == want_texts
    assert [tuple(int(r[k]) for k in ("contig", "n_rows", "len_in", "len_out")) for r in rows_out] == \
           [(c, want_voted[c], want_in[c], len(want_texts[c])) for c in range(len(POLISH_LENS))]
    assert [(int(g["round"]), int(g["n_mapped"]), int(g["n_voted"])) for g in log] == [(k + 1,) + want_log[k] for k in range(2)]
    assert (log["n_chunks"] >= 3).all() if max_boxes else (log["n_chunks"] == 1).all()
    assert int(log[1]["n_bases_out"]) == sum(len(t) for t in want_texts)
    if strands == 1:
        assert want_log[0][0] < two_rounds[3][3][0][0]                          # the + rows only


def test_refusals(ctx, case):
    T, Rd, Rc, rows = case["T"], case["Rd"], case["Rc"], case["rows"]
    mask = eng.mask_from_pattern(MASK_PAT)

    def status(call):
        with pytest.raises(PbaError) as e:
            call()
        return e.value.status

    found = rows[rows["found"] == 1]
    minus = found[found["strand"] == -1]
    pile = Pileup(ctx, T, t_lo=2, t_hi=len(POLISH_LENS))
    before = pile.dump(LONG)
    outside = found[:8].copy()
    outside["contig"][5] = 1                                                      # good rows first, then one outside [2, 6)
    assert status(lambda: pile.vote_mapped(Rd, outside, R, OVERLAP_MIN, reads_rc=Rc)) == -1
    assert status(lambda: pile.vote_mapped(Rd, minus[:3], R, OVERLAP_MIN)) == -1                       # strand -1 without reads_rc
    other = ctx.seqs_from_list([c + b"A" for c in case["contigs"]], strict_acgt=True)
    assert status(lambda: Pileup.vote_mapped(PileupAs(pile, other), Rd, found[:3], R, OVERLAP_MIN, reads_rc=Rc)) == -1   # not the pile-up's set
    loose = ctx.seqs_from_list([r[:50] + b"N" + r[51:] for r in case["reads"]], strict_acgt=False)
    assert status(lambda: pile.vote_mapped(loose, found[:3], R, OVERLAP_MIN, reads_rc=Rc)) == -6      # bytes outside ACGT
    after = pile.dump(LONG)
    for x, y in zip(before, after):
        assert (x == y).all()                                                     # host-side refusals leave the boxes alone
    assert status(lambda: ctx.polish_contigs(T, loose, mask, R, rounds=1)) == -6
    assert status(lambda: ctx.polish_contigs(T, Rd, mask, R, rounds=0)) == -1
    pile.evolve()
    assert status(lambda: pile.vote_mapped(Rd, found[:3], R, OVERLAP_MIN, reads_rc=Rc)) == -1          # spent
