"""The shifted form of the score-only bit-vector sweep in rings 1 and 2 (align_bitvec.h: bitvec_pass with SHIFT,
csrc/lane_shift.h): lane k holds superblock s_cl + k, lane 0 is always the top of the band, the hand-off of the carry masks
is a scalar shift without a mask, and every close moves Pv / Mv / acc one lane up and the table and ring addresses one column
on.  What can go wrong is a lane that takes the border a step early or late behind a close, a last lane that starts its next
superblock on the registers of another, a segment's word read from the lane its superblock was in before the move, fin
words written by lane number where they are read by column, and a sweep that starts on what the previous one left
shifted.  So: longer sides of 64 RB - 1 .. 128 RB + 1 rows with the shorter side 0, 1, w - 1, w, w + 40 shorter; a first failing
row in the segment judged one step before, at and one step behind the close of superblock 0, 63 and 64; the free end's
minimum in the first, a middle and the last superblock below row m after sixty closes; a re-run at the reference band; 32
pairs 640 times through every wavefront.  Through k_align_pairs, and a subset through k_locate (one probe per read: the
band-cell counter is a function of each alignment) and the spaced round.  Every input is proved from the oracle in
test_lane_shift_inputs_cpu.py; csrc/lane_shift.h itself is played against the ring of lanes in test_lane_shift_cpu.py.
Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import align_rings as ar
import lane_shift_inputs as ls
import test_gpu_align_rings as rings
from conftest import MASK_PAT
from diag_collect_inputs import ROW
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PAIR_DTYPE, PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL, PBA_KERNEL_BITVEC
from test_align_rings_cpu import excursion_case, must_redo
from test_gpu_parity import check_result
from test_gpu_text_ring import RS

pytestmark = pytest.mark.gpu


def forced(NB, B, R):
    return B if NB == 1 else B.with_pilot(ar.pilot(ar.row_of(*ROW[NB])[0], R))


@pytest.mark.parametrize("NB", [1, 2])
def test_rows_past_the_first_and_second_revolution(ctx, oracle, NB):
    F = forced(NB, ls.wrap_batch(NB), ls.WRAP_R)
    prof = rings.check_batch(ctx, oracle, F, ls.WRAP_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == NB and prof["n_first"] == len(F.pairs) and prof["n_redo"] == 0


@pytest.mark.parametrize("NB", [1, 2])
def test_first_failing_row_beside_a_close(ctx, oracle, NB):
    F = forced(NB, ls.seg_batch(NB), ls.SEG_R)
    want = ar.expected(oracle, F, ls.SEG_R)
    assert sum(1 for meta, x in zip(F.meta, want) if meta["kind"] == "fail" and x["fail_row"] == meta["f"]) == 9
    prof = rings.check_batch(ctx, oracle, F, ls.SEG_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == NB and prof["n_redo"] == 0


@pytest.mark.parametrize("NB", [1, 2])
def test_fin_words_found_by_column_after_many_moves(ctx, oracle, NB):
    F = forced(NB, ls.alias_batch(NB), ls.ALIAS_R)
    prof = rings.check_batch(ctx, oracle, F, ls.ALIAS_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == NB and prof["n_redo"] == 0


def test_rerun_at_the_reference_band(ctx, oracle):
    """pairs the narrow sweep of ring 1 cannot certify: swept again in ring 2 at the reference band, both in the shifted form"""
    B, w, wl = excursion_case()
    redo = must_redo(ar.expected(oracle, B, ar.EXC_R), B.meta, w, wl)
    keep = sorted(redo)[-6:] + [q for q in range(len(B.pairs)) if q not in redo][-2:]
    prof = rings.check_batch(ctx, oracle, B.subset(keep), ar.EXC_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == 1 and prof["nb_redo"] == 2 and prof["n_redo"] >= 6


@pytest.mark.parametrize("NB", [1, 2])
def test_sweeps_start_on_what_the_last_one_left_moved(ctx, oracle, NB):
    """more pairs than the chip has wavefronts: every wavefront sweeps several, long ones (a dozen closes) and short ones in
    turn, and finds the previous pair's lanes, masks, columns and fin words where its moves left them"""
    R = RS[NB]
    B = ls.stale_batch(NB, R)
    want = ar.expected(oracle, B, R)
    for meta, x in zip(B.meta, want):
        assert (x["rc"] >= 0 or x["fail_row"] == 0) == (meta["kind"] == "true"), (meta, x)
    assert sum(x["rc"] >= 0 for x in want) >= 16
    reps = 640
    F = forced(NB, B, R)
    n0 = len(F.pairs) - len(B.pairs)                          # the pilot, once
    S = ctx.seqs_from_list(F.seqs, strict_acgt=True)
    pairs = np.array(F.pairs[:n0] + F.pairs[n0:] * reps, PAIR_DTYPE)
    assert pairs.size > 2 * 256 * 32
    out = ctx.align_batch(S, S, pairs, R, kernel=PBA_KERNEL_BITVEC)
    assert ctx.last_profile()["nb_first"] == NB
    for q in range(len(B.pairs)):
        check_result(out[n0 + q], want[q], B.meta[q]["tag"])
    first = out[n0:n0 + len(B.pairs)]
    for r in range(1, reps):
        assert (out[n0 + r * len(B.pairs):n0 + (r + 1) * len(B.pairs)] == first).all(), r


# ----------------------------------------------------------------------------- the drivers
@pytest.mark.parametrize("NB", [1, 2])
def test_locate_in_the_shifted_form(ctx, oracle, NB):
    """k_locate<NB>, one probe per read: rows, pair counts and the band cells against the oracle."""
    R = ls.DRIVER_R
    g, texts, meta = ls.driver_case(NB)
    reads = np.frombuffer(b"".join(texts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
    mask = eng.mask_from_pattern(MASK_PAT)
    T = ctx.seqs_from_list([g.tobytes()], strict_acgt=True)
    Rd = ctx.seqs_from_text(reads, offs, strict_acgt=True)
    ix = ctx.index_build(T, 0, mask, PBA_INDEX_ALL)
    rows, st = ctx.locate(ix, T, 0, Rd, R, 1, 33, kernel=PBA_KERNEL_BITVEC)
    assert ctx.last_profile()["nb_first"] == NB
    want, wst = oracle.locator(g, mask, R, reads, offs, 1, 33, nthreads=8)
    for c in ("nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs"):
        assert (rows[c] == want[c]).all(), c
    assert st == wst and "n_cells" in st and wst["n_located"] == len(ls.driver_ms(NB)), (st, wst)


@pytest.mark.parametrize("NB", [1, 2])
def test_spaced_round_in_the_shifted_form(ctx, oracle, NB):
    """k_spaced_round<NB> over the same reads as records, in both seed placements."""
    R = ls.DRIVER_R
    g, texts, meta = ls.driver_case(NB)
    gb = g.tobytes()
    assert len(gb) < 40000                                   # a head-and-tail index sees all of it
    file = b"".join(eng.text2bin(t) for t in texts)
    rec_offs = np.concatenate([[0], np.cumsum([4 + (len(t) + 3) // 4 for t in texts])[:-1]]).astype(np.uint64)
    mask = eng.mask_from_pattern(MASK_PAT)
    T = ctx.seqs_from_list([gb], strict_acgt=True)
    Rs = ctx.seqs_from_records(file, 0, 1 << 30)
    assert Rs.count == len(texts)
    ixh = ctx.index_build(T, 0, mask, PBA_INDEX_HEAD_TAIL)
    for buggy in (True, False):
        got = ctx.spaced_round(ixh, T, 0, Rs, R, 32, 64, buggy_seed_at=buggy, kernel=PBA_KERNEL_BITVEC)
        assert ctx.last_profile()["nb_first"] == NB
        wss = oracle.spaced_round(gb, mask, R, file, rec_offs, 32, 64, buggy=buggy, nthreads=8)
        for c in ("found", "n_trials", "n_pairs"):
            assert (got[c] == wss[c]).all(), (c, buggy)
        sel = wss["found"] == 1
        for c in ("j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b"):
            assert (got[c][sel] == wss[c][sel]).all(), (c, buggy)
        assert int(sel.sum()) >= 4 and int(wss["n_pairs"].sum()) >= int(sel.sum()) + 2, (buggy, int(sel.sum()))
