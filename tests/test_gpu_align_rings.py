"""The banded bit-vector aligner in every ring size (NB = 1, 2, 3, 4, 6, 8 blocks per lane), as the narrow first launch and
as the reference-band re-run, at the edges of its blocks, superblocks and windows, against the oracle -- exact, results and
edit scripts.  The ring of a launch comes from the largest max_dst of the call (make_plan), so one pilot pair that fails at
once forces it for a few hundred short pairs; tests/align_rings.py builds the inputs, tests/test_align_rings_cpu.py proves
from the oracle alone that each is in the regime it is named for.  Every test asserts the rings it ran in through
last_profile().  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import align_rings as ar
from conftest import MASK_PAT
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import (PAIR_DTYPE, PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL, PBA_KERNEL_AUTO, PBA_KERNEL_BITVEC,
                                       PBA_KERNEL_ROWSWEEP, PbaError)
from test_align_rings_cpu import EDGE_R, excursion_case, must_redo
from test_gpu_parity import check_result

pytestmark = pytest.mark.gpu

EDGE_ROWS = [(1, 1), (2, 2), (2, 3), (3, 4), (3, 6), (4, 6), (6, 8)]


def forced(row, edges, R=EDGE_R):
    """the batch of a plan row: its pilot (none for (1, 1): short pairs are there by themselves) and the edge pairs"""
    return edges if row == (1, 1) else edges.with_pilot(ar.pilot(ar.row_of(*row)[0], R))


def check_batch(ctx, oracle, B, R, kernel, scripts=False):
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs, PAIR_DTYPE)
    if scripts:
        out, ops = ctx.align_batch_trace(S, S, pairs, R, kernel=kernel)
    else:
        out, ops = ctx.align_batch(S, S, pairs, R, kernel=kernel), None
    prof = ctx.last_profile()
    for q, (got, exp) in enumerate(zip(out, ar.expected(oracle, B, R))):
        check_result(got, exp, (B.meta[q]["tag"], kernel))
        if scripts:
            assert ops[q].tolist() == exp["ops"].tolist(), (B.meta[q]["tag"], kernel)
    return prof


@pytest.mark.parametrize("row", EDGE_ROWS)
def test_forced_ring_edges(ctx, oracle, row):
    """k_align_pairs<nb1> on the edge set built for that ring; the row sweep on the same batch cross-checks the set."""
    B = forced(row, ar.edge_pairs(row[0], EDGE_R))
    prof = check_batch(ctx, oracle, B, EDGE_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == row[0] and prof["n_first"] == len(B.pairs)
    assert check_batch(ctx, oracle, B, EDGE_R, PBA_KERNEL_ROWSWEEP)["nb_first"] == 0


@pytest.mark.parametrize("row", EDGE_ROWS)
def test_forced_ring_scripts(ctx, oracle, row, monkeypatch):
    """k_trace_pairs<nb1> in its checkpoint form on the same batches; in its streamed form for two rows, on the pilot and
    32 edge pairs (the streamed scratch is sized per wavefront for the pilot)."""
    edges = ar.edge_pairs(row[0], EDGE_R)
    B = forced(row, edges)
    assert check_batch(ctx, oracle, B, EDGE_R, PBA_KERNEL_BITVEC, scripts=True)["nb_first"] == row[0]
    if row in ((3, 4), (6, 8)):
        n = len(edges.pairs)
        keep = list(range(0, n - 16, max(1, (n - 16) // 16)))[:16] + list(range(n - 16, n))     # a spread of the grid, the placements
        monkeypatch.setenv("PBA_TRACE_STREAM", "1")
        assert check_batch(ctx, oracle, forced(row, edges.subset(keep)), EDGE_R, PBA_KERNEL_BITVEC, scripts=True)["nb_first"] == row[0]


@pytest.mark.parametrize("NB", ar.RINGS)
def test_ring_wrap(ctx, oracle, NB):
    """Rows past 64 superblocks: lane 0 takes its second one.  Ring 1 by the pairs' own size, rings 2 .. 6 behind a pilot,
    ring 8 (only ever a re-run) through the wide pairs of row (4, 8), which have 64 * 256 + 1 rows and more."""
    if NB == 8:
        B, R = ar.wide_pairs((4, 8))
        prof = check_batch(ctx, oracle, B, R, PBA_KERNEL_BITVEC, scripts=True)
        assert prof["nb_redo"] == 8 and prof["n_redo"] == len(B.pairs)
        return
    row = next((a, b) for _, _, a, b in ar.plan_rows() if a == NB)
    B = forced(row, ar.wrap_pairs(NB))
    for scripts in (False, True):
        assert check_batch(ctx, oracle, B, 0.30, PBA_KERNEL_BITVEC, scripts=scripts)["nb_first"] == NB


def test_certificate_excursions(ctx, oracle):
    """Pairs whose cheapest path leaves the narrow window by one base more or less than it holds, on either side, and pairs
    that fail too late for a narrow sweep to say so: what bv_goal_certified / bv_fail_certified cannot vouch for is re-run at
    the reference band, everything equals the oracle."""
    B, w, wl = excursion_case()
    need = len(must_redo(ar.expected(oracle, B, ar.EXC_R), B.meta, w, wl))
    assert need >= len(B.pairs) // 2 + 6
    for scripts in (False, True):
        prof = check_batch(ctx, oracle, B, ar.EXC_R, PBA_KERNEL_BITVEC, scripts=scripts)
        assert prof["nb_first"] == 1 and prof["nb_redo"] == 2 and prof["n_redo"] >= need, (scripts, prof["n_redo"], need)


@pytest.mark.parametrize("row", sorted(ar.WIDE))
def test_reference_band_rings(ctx, oracle, row):
    """k_align_pairs<nb2> / k_trace_pairs<nb2> at the reference band for nb2 = 3, 4, 6, 8: pairs the reference accepts at a
    cost above the first window of their row."""
    B, R = ar.wide_pairs(row)
    prof = check_batch(ctx, oracle, B, R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == row[0] and prof["nb_redo"] == row[1] and prof["n_redo"] >= len(B.pairs)
    prof = check_batch(ctx, oracle, B.subset([0]), R, PBA_KERNEL_BITVEC, scripts=True)
    assert prof["nb_redo"] == row[1] and prof["n_redo"] == 1


def test_plan_edge_10794(ctx, oracle):
    """The last band the bit-vector array takes and the first it does not."""
    edges = ar.edge_pairs(6, EDGE_R)
    B = edges.with_pilot(ar.pilot(10794, EDGE_R))
    prof = check_batch(ctx, oracle, B, EDGE_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == ar.nb1(10794) == 6
    assert prof["n_redo"] == 0 or prof["nb_redo"] == ar.nb2(10794)      # (nothing in this batch needs the re-run)
    B = edges.with_pilot(ar.pilot(10795, EDGE_R))
    with pytest.raises(PbaError) as e:
        check_batch(ctx, oracle, B, EDGE_R, PBA_KERNEL_BITVEC)
    assert e.value.status == -4
    assert check_batch(ctx, oracle, B, EDGE_R, PBA_KERNEL_AUTO)["nb_first"] == 0


def driver_case(fill_len):
    g = eng.synth_genome(611, 60000)
    reads, offs, _ = eng.synth_reads(612, g, 40, 1500)
    rng = np.random.RandomState(613)
    texts = [reads[int(offs[r]):int(offs[r + 1])].tobytes()[:int(rng.randint(1000, 1501))] for r in range(40)]
    texts.append(ar.rand_seq(rng, fill_len))               # the filler: sizes the plan, its probes hit nothing
    return g, texts


@pytest.mark.parametrize("row", [(3, 6), (6, 8)])
def test_drivers_in_forced_rings(ctx, oracle, row):
    """k_locate<nb1> and k_spaced_round<nb1>: the drivers plan from the longest read, so one long unrelated read puts 40
    reads of 1 - 1.5 kb through rings 3 and 6."""
    R = 0.30
    fill = len(ar.pilot(ar.row_of(*row)[0], R)[0])
    g, texts = driver_case(fill)
    assert (ar.nb1(1 + int(fill * R)), ar.nb2(1 + int(fill * R))) == row
    reads = np.frombuffer(b"".join(texts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
    mask = eng.mask_from_pattern(MASK_PAT)
    T = ctx.seqs_from_list([g.tobytes()], strict_acgt=True)
    Rd = ctx.seqs_from_text(reads, offs, strict_acgt=True)
    ix = ctx.index_build(T, 0, mask, PBA_INDEX_ALL)
    rows, st = ctx.locate(ix, T, 0, Rd, R, 50, 500, kernel=PBA_KERNEL_BITVEC)
    assert ctx.last_profile()["nb_first"] == row[0]
    want, wst = oracle.locator(g, mask, R, reads, offs, 50, 500, nthreads=8)
    for c in ("nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs"):
        assert (rows[c] == want[c]).all(), c
    assert st == wst and wst["n_located"] >= 25 and int(want["found"][-1]) == 0
    gb = g.tobytes()
    for r in np.flatnonzero(want["found"] == 1):           # locator.cpp:86: the cell at the end of the diagonal
        j, pos = int(want["j"][r]), int(want["pos"][r])
        x = oracle.align(texts[r][j:], gb[pos:pos + 2 * len(texts[r]) + 8], R)
        m = min(x["len_a"], x["len_b"])
        assert x["rc"] >= 0 and int(rows["diag_cost"][r]) == oracle.cell(m, m)[0], r
    # the locked round of spaced_seed.cpp over the same reads as records
    file = b"".join(eng.text2bin(t) for t in texts)
    rec_offs = np.concatenate([[0], np.cumsum([4 + (len(t) + 3) // 4 for t in texts])[:-1]]).astype(np.uint64)
    Rs = ctx.seqs_from_records(file, 0, 1 << 30)
    assert Rs.count == len(texts) and Rs.max_len == fill
    ixh = ctx.index_build(T, 0, mask, PBA_INDEX_HEAD_TAIL)
    for buggy in (True, False):
        got = ctx.spaced_round(ixh, T, 0, Rs, R, 32, 64, buggy_seed_at=buggy, kernel=PBA_KERNEL_BITVEC)
        assert ctx.last_profile()["nb_first"] == row[0]
        wss = oracle.spaced_round(gb, mask, R, file, rec_offs, 32, 64, buggy=buggy, nthreads=8)
        for c in ("found", "n_trials", "n_pairs"):
            assert (got[c] == wss[c]).all(), (c, buggy)
        sel = wss["found"] == 1
        for c in ("j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b"):
            assert (got[c][sel] == wss[c][sel]).all(), (c, buggy)
        assert int(wss["found"][-1]) == 0


@pytest.mark.parametrize("row", [(3, 4), (6, 8)])
def test_votes_in_forced_rings(ctx, row):
    """k_vote_pairs<nb1> == the scripts of k_trace_pairs<nb1> applied with pba_cons_elect (the comparison of
    test_cons_vote_pairs_equals_scripts_then_elect) in rings 3 and 6: the reference is long enough for a pilot -- all of it
    against an unrelated read of the pilot's length -- to size the plan."""
    from cons_scenarios import round_tries, scenario_inputs
    fill = len(ar.pilot(ar.row_of(*row)[0], 0.3)[0])
    sc = ("vote", 151, 152, 40000, 1000, fill + 200, 240, 1300, 2, (0.05, 0.05, 0.05), True)
    text, weight, reads = scenario_inputs(sc)
    reads = list(reads) + [ar.rand_seq(np.random.RandomState(153), fill)]
    A = ctx.seqs_from_list([b"ACGT" * 10, text], strict_acgt=True)       # the reference is sequence 1 of its set
    B = ctx.seqs_from_list(reads, strict_acgt=True)
    pairs = [(1, 0, len(text), len(reads) - 1, 0, fill, 0)]             # the pilot
    for rnd in (0, 1):
        for hit, r, seg, fwd in round_tries(text, reads[:-1], rnd):
            if fwd:
                pairs.append((1, hit, len(text) - hit, r, len(reads[r]) - len(seg), len(seg), 0))
            else:
                pairs.append((1, hit, hit + 1, r, len(seg) - 1, len(seg), 3))
    pairs = np.array(pairs, PAIR_DTYPE)
    assert pairs.size >= 30 and (pairs["flags"] == 3).sum() >= 8
    one, many = eng.Consensus(ctx, text, weight), eng.Consensus(ctx, text, weight)
    out, scripts = ctx.align_batch_trace(A, B, pairs, 0.3, kernel=PBA_KERNEL_BITVEC)
    assert ctx.last_profile()["nb_first"] == row[0] and int(out["rc"][0]) == -1
    n_voted = 0
    for pr, res, ops in zip(pairs, out, scripts):
        if int(res["rc"]) < 0 or int(res["matlen_a"]) < 64:
            continue
        fwd = int(pr["flags"]) == 0
        rd = reads[int(pr["b_seq"])]
        seg = rd[int(pr["b_pos"]):] if fwd else rd[:int(pr["b_pos"]) + 1]
        one.elect([int(pr["a_pos"])], [fwd], [ops], [eng.script_vals(ops, seg, fwd)])
        n_voted += 1
    out2 = many.vote_pairs(A, 1, B, pairs, 0.3, 64)
    assert ctx.last_profile()["nb_first"] == row[0]
    assert n_voted >= 20
    for c in ("rc", "cost", "matlen_a", "matlen_b"):
        assert (out[c] == out2[c]).all(), c
    for x, y in zip(one.dump()[:3], many.dump()[:3]):
        assert (x == y).all()
    assert one.evolve() == many.evolve()


# The all-vs-all walk (pba_overlap_all) picks its rings itself, through nb_mid and the sampled decision: its first launch,
# middle ring and reference band in every plan row are in tests/test_gpu_walk_rings.py (inputs: tests/walk_ring_inputs.py).
