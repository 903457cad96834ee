"""The two events the bit-vector sweep's schedule no longer has (align_bitvec.h: bitvec_pass) -- the hand-off's end, now the
close event's own (`live`: a lane's carries are masked where it hands them out), and the diagonal's entry, now armed by the
segment end in front of it (the 64-bit `one`) -- against the oracle, exactly, at the shapes where either can go wrong:

  1  m around the superblock edges: the diagonal leaves a superblock exactly at m, one row before, one row after; at the first
     edge, the second, and behind the ring's wrap (lane 0's second superblock), rings 1 and 2
  2  a first failing row just before and just after a superblock edge and in the first segment behind the fold, rings 1, 2, 3.
     The batch entry points report no row: each pair fails in the few rows from its planted one on and nowhere else
     (test_schedule_folds_cpu.py, for every burst, the ring's wrap included), so a diagonal collected a row or a block off
     passes it, and nothing is re-run
  3  S = 1, 2, 63, 64, 65, 128, 129 superblocks: where `live` starts and where it is re-armed
  4  superblocks that close on the last column in the step a neighbour's hand-off ends: nr - m = 0, 1 and w, the longer
     sequence as a and as b (the pairs of 1)
  5  the traced forms on the pairs of 1 - 4: pba_align_batch_trace in its checkpoint and its streamed form (edit scripts,
     or the verdict alone where a pair fails) and pba_align_batch_cigar (runs and counts) -- bitvec_rerun restores from
     checkpoints written under the new mask
  6  one all-vs-all of 292 reads of 2 - 3 kb (schedule_fold_inputs.walk_set): 146 work items in k_ovl_walk<2>, of which 20
     park -- a cost one above the narrow window, and one near the band's limit -- between items that are decided narrowly,
     and are resumed in k_ovl_walk<3>: rows and every counter against overlap_ref.walk_composition, the launches against
     walk_ring_inputs.stages

tests/schedule_fold_inputs.py builds the inputs.  Every case asserts its ring and that the narrow pass certified by itself through
last_profile(): a re-run at the reference band would hide a wrong narrow sweep.  Needs a real MI355X (-m gpu)."""
import pytest

import schedule_fold_inputs as sf
import test_gpu_align_rings as rings
import test_gpu_cigar as cigar
import test_gpu_walk_rings as walk
import walk_ring_inputs as wi
from pacbioassembly_amd.engine import PBA_KERNEL_BITVEC

pytestmark = pytest.mark.gpu


def certified(prof, NB, B):
    assert prof["nb_first"] == NB and prof["n_first"] == len(B.pairs) and prof["n_redo"] == 0, prof


@pytest.mark.parametrize("NB", [1, 2])
def test_m_at_the_superblock_edges(ctx, oracle, NB):
    """1, 4: k_align_pairs<NB>, which also reports D(m, m)"""
    B = sf.forced(NB, sf.edge_pairs(NB), sf.FOLD_R)
    certified(rings.check_batch(ctx, oracle, B, sf.FOLD_R, PBA_KERNEL_BITVEC), NB, B)


FORMS = ["score", "checkpoint", "stream"]      # k_align_pairs; k_trace_pairs<NB, true>; k_trace_pairs<NB, false>


def run_form(ctx, oracle, monkeypatch, B, R, form):
    if form == "stream":
        monkeypatch.setenv("PBA_TRACE_STREAM", "1")
    return rings.check_batch(ctx, oracle, B, R, PBA_KERNEL_BITVEC, scripts=form != "score")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("NB", [1, 2, 3])
def test_first_failing_row_around_a_fold(ctx, oracle, monkeypatch, NB, form):
    """2, 5: the verdicts of the score-only kernel and of the scripts' kernel in both its forms"""
    for R, G in sf.burst_groups(NB).items():
        B = sf.forced(NB, G, R)
        certified(run_form(ctx, oracle, monkeypatch, B, R, form), NB, B)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("NB", [1, 2])
def test_superblocks_around_the_ring_size(ctx, oracle, monkeypatch, NB, form):
    """3, 5: score only and with scripts in both forms"""
    B = sf.forced(NB, sf.ring_fill_pairs(NB), sf.FOLD_R)
    certified(run_form(ctx, oracle, monkeypatch, B, sf.FOLD_R, form), NB, B)


@pytest.mark.parametrize("form", ["checkpoint", "stream"])
@pytest.mark.parametrize("NB", [1, 2])
def test_scripts_over_the_edges(ctx, oracle, NB, form, monkeypatch):
    """5: k_trace_pairs<NB> in both forms on the pairs of 1 and 4"""
    B = sf.forced(NB, sf.edge_pairs(NB), sf.FOLD_R)
    certified(run_form(ctx, oracle, monkeypatch, B, sf.FOLD_R, form), NB, B)


@pytest.mark.parametrize("NB", [1, 2])
def test_cigars_over_the_edges(ctx, oracle, NB):
    """5: k_cigar_pairs<NB> on the pairs of 1 and 4, and of 3"""
    for B in (sf.edge_pairs(NB), sf.ring_fill_pairs(NB)):
        B = sf.forced(NB, B, sf.FOLD_R)
        certified(cigar.check_batch(ctx, oracle, B, sf.FOLD_R), NB, B)


def test_walk_parks_and_resumes(ctx, oracle, monkeypatch):
    """6: test_gpu_walk_rings.run holds rows and counters to the composition (test_gpu_overlap_edges.check) and the ctx
    profile to the launches derived on the CPU"""
    C = sf.walk_set()
    W = wi.model(oracle, C)
    want = walk.run(ctx, monkeypatch, W)
    parked = sf.WALK_LONG["w1+1"] + sf.WALK_LONG["band"]
    assert want["launches"] == [(2, "first", len(wi.items_of(W))), (3, "redo_band", parked)]
    assert want["parked"] == parked > 0 and want["nb_redo"] == 3 > want["nb_first"] == 2
    assert len(W["rows"]) == sum(sf.WALK_LONG.values()) + sf.WALK_SHORT
