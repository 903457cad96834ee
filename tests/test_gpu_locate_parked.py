"""k_locate<NB, SET> where the walk goes on behind a sweep of the wavefront (pba_drivers.hip; rings 1 and 2), on the inputs of
locate_parked_inputs.py: the success behind one, two and three survivors of its own 64-slot group (hits the prefilter passes
and the wavefront's sweep refuses in rows 33 .. 64), at slot 63, at slot 64 and in a third chunk, in the second lane block of
trials = 130 with failed survivors in the first, a read never located whose sweeps all fail late, and a read handed to the
re-run behind survivors.  After each failed sweep the walk has to find again: the survivors left, the failed hits counted so
far and from where, the chunk, the lane block, the list's length, the hit mask, the read and the counters -- whatever the
sweep pushed out of the scalar registers (a form that parks them in LDS across the sweep was built against these tests and
dropped for want of a gain: DESIGN.md 4.3, round 14).
Every case is one read per call (ring 2: with an unrelated pilot read behind it that sizes the plan), in both forms -- one
contig (pba_locate) and a set of two whose second is the contig (pba_map_reads, one strand: the survivor's contig travels
with the walk too) -- and every row column, n_pairs per read, n_cells and n_probe_hits are Oracle.locator's.  Again over
scribbled work buffers, and once on a caller-owned stream.  What each input is, is proved in
test_locate_parked_inputs_cpu.py.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import locate_parked_inputs as lp
import locate_walk_inputs as lw
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_INDEX_ALL, PBA_KERNEL_BITVEC

pytestmark = pytest.mark.gpu

CASES = lp.cases()
DECOY = np.random.RandomState(9599).randint(0, 4, 333)
DECOY = np.frombuffer(b"ACGT", np.uint8)[DECOY].tobytes()          # contig 0 of the set form: the case's genome is contig 1


def run_case(ctx, oracle, c, NB, SET, n_redo=0):
    pilot = NB == 2
    want, wst = lp.expected(oracle, c, pilot)
    texts = c["reads"] + ([lp.pilot_read()] if pilot else [])
    mask = eng.mask_from_pattern(c["pat"])
    Rd = ctx.seqs_from_list(texts, strict_acgt=True)
    if SET:
        T = ctx.seqs_from_list([DECOY, c["g"]], strict_acgt=True)
        rows, mst = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, c["R"], c["trials"], c["min_len"], kernel=PBA_KERNEL_BITVEC, strands=1)
        st = mst["strand"][0]
        assert (rows["contig"] == np.where(want["found"] == 1, 1, -1)).all(), (c["name"], rows["contig"])
    else:
        T = ctx.seqs_from_list([c["g"]], strict_acgt=True)
        rows, st = ctx.locate(ctx.index_build(T, 0, mask, PBA_INDEX_ALL), T, 0, Rd, c["R"], c["trials"], c["min_len"], kernel=PBA_KERNEL_BITVEC)
    prof = ctx.last_profile()
    assert prof["nb_first"] == NB and prof["n_redo"] == n_redo, (c["name"], prof)
    for col in lw.LOC_COLS:
        assert (rows[col] == want[col]).all(), (c["name"], NB, SET, col, rows[col], want[col])
    for key in lw.STAT_KEYS:
        assert st[key] == wst[key], (c["name"], NB, SET, key, st[key], wst[key])
    return want, wst


@pytest.mark.parametrize("SET", [False, True], ids=["one", "set"])
@pytest.mark.parametrize("NB", [1, 2])
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_walk_resumes_behind_failed_sweeps(ctx, oracle, c, NB, SET):
    want, wst = run_case(ctx, oracle, c, NB, SET)
    assert want["found"][0] == (c["claims"].get("success", True) is not None)
    assert wst["n_pairs"] >= 5 and wst["n_cells"] > 0


@pytest.mark.parametrize("SET", [False, True], ids=["one", "set"])
def test_redo_behind_survivors(ctx, oracle, SET):
    """the narrow pass cannot certify the read's true place: behind two failed sweeps the walk hands the read over with the
    probes counted so far, and the re-run at the reference band (ring 2) gives the oracle's row"""
    c, j = lp.redo_case(oracle)
    want, wst = run_case(ctx, oracle, c, 1, SET, n_redo=1)
    assert ctx.last_profile()["nb_redo"] == 2
    assert want["found"][0] == 1 and want["j"][0] == j


@pytest.mark.parametrize("NB", [1, 2])
def test_over_scribbled_work_buffers(ctx, oracle, NB):
    """every case again, both forms, each call over work buffers a scribble left: nothing of the walk's state is taken from
    what an earlier read, an earlier call or the scribble wrote"""
    for byte in (0xFF, 0x5A):
        for c in CASES:
            for SET in (False, True):
                ctx.scribble(byte)
                run_case(ctx, oracle, c, NB, SET)
    c, _ = lp.redo_case(oracle)
    if NB == 1:
        ctx.scribble(0xFF)
        run_case(ctx, oracle, c, 1, False, n_redo=1)


def test_on_a_caller_owned_stream(ctx, oracle):
    import torch
    s = torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    try:
        for c in CASES:
            for NB in (1, 2):
                run_case(ctx, oracle, c, NB, NB == 2)
    finally:
        ctx.set_stream(None)
