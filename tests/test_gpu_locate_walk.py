"""k_locate<NB, SET>'s lane-parallel candidate walk (pba_drivers.hip, csrc/locate_walk.h) on the inputs of
locate_walk_inputs.py: a read's probes keyed and looked up 64 at a time, their hits one list in the reference's order,
prefiltered 64 slots at a time, first success.  Every case is one read per call -- a slip in the counters has no other read
to cancel in -- and compares every row column and n_pairs, n_located, n_probe_hits, n_cells with Oracle.locator (the set
cases with map_ref); what each input is (list lengths, the slot of the success, the rows the hits in front of it fail at) is
proved in test_locate_walk_cpu.py.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import locate_walk_inputs as lw
import map_ref
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_INDEX_ALL, PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP

pytestmark = pytest.mark.gpu

CASES = lw.cases()
MAP_COLS = ("nseq", "found", "strand", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs", "r_beg", "r_end", "c_beg", "c_end")


def one_read_calls(ctx, oracle, c):
    """every read of a one-contig case in a call of its own, against the oracle's walk of that read"""
    mask = eng.mask_from_pattern(c["pat"])
    T = ctx.seqs_from_list([c["g"]], strict_acgt=True)
    ix = ctx.index_build(T, 0, mask, PBA_INDEX_ALL)
    kernel = PBA_KERNEL_ROWSWEEP if c.get("kernel") == "rowsweep" else PBA_KERNEL_BITVEC
    for r, x in enumerate(c["reads"]):
        want, wst = lw.expected(oracle, c, r)
        rows, st = ctx.locate(ix, T, 0, ctx.seqs_from_list([x], strict_acgt=True), c["R"], c["trials"], c["min_len"], kernel=kernel)
        assert ctx.last_profile()["n_redo"] == 0
        for col in lw.LOC_COLS:
            assert (rows[col] == want[col]).all(), (c["name"], r, col, rows, want)
        assert st == wst, (c["name"], r, st, wst)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_walk_case(ctx, oracle, c):
    """run length, chunk seam, position of the success, probe count, zero keys, the row sweep"""
    one_read_calls(ctx, oracle, c)


def test_short_reads(ctx, oracle):
    """min_len = 20, reads of 45, 40, 40 and 15 bases under trials = 50: lanes past the read's end are idle, the probes of the
    last 15 positions key padded windows (read 2 succeeds at one), pairs below 32 elements skip the prefilter"""
    c = lw.short_case()
    one_read_calls(ctx, oracle, c)
    mask = eng.mask_from_pattern(c["pat"])                                    # ... and all four in one call: nseq runs past the short one
    T = ctx.seqs_from_list([c["g"]], strict_acgt=True)
    reads = np.frombuffer(b"".join(c["reads"]), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(x) for x in c["reads"]])]).astype(np.uint64)
    want, wst = oracle.locator(np.frombuffer(c["g"], np.uint8), mask, c["R"], reads, offs, c["trials"], c["min_len"])
    rows, st = ctx.locate(ctx.index_build(T, 0, mask, PBA_INDEX_ALL), T, 0, ctx.seqs_from_list(c["reads"], strict_acgt=True), c["R"],
                          c["trials"], c["min_len"], kernel=PBA_KERNEL_BITVEC)
    for col in lw.LOC_COLS:
        assert (rows[col] == want[col]).all(), col
    assert st == wst and wst["n_located"] == 3 and wst["n_reads_kept"] == 3


@pytest.mark.parametrize("strands", [1, 3])
def test_set_form(ctx, oracle, strands):
    """k_locate<NB, true>: one key with hits in three contigs, in (contig, position) order across the 64-slot seam; with both
    strands the second read is found by the - walk"""
    contigs, reads = lw.set_case()
    mask = eng.mask_from_pattern(lw.MASK_PAT)
    want, wst, _ = map_ref.map_reads_ref(oracle, contigs, reads, mask, 0.30, 50, 500, strands=strands)
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    ix = ctx.index_build_set(T, mask)
    got, gst = ctx.map_reads(ix, T, ctx.seqs_from_list(reads, strict_acgt=True), 0.30, 50, 500, kernel=PBA_KERNEL_BITVEC, strands=strands)
    for col in MAP_COLS:
        assert (got[col] == want[col]).all(), (col, got, want)
    for k in range(2):
        for key in map_ref.STAT_KEYS:
            assert gst["strand"][k][key] == wst[k][key], (k, key, gst["strand"][k], wst[k])
    for r, x in enumerate(reads):                                             # read by read
        w1, s1, _ = map_ref.map_reads_ref(oracle, contigs, [x], mask, 0.30, 50, 500, strands=strands)
        g1, t1 = ctx.map_reads(ix, T, ctx.seqs_from_list([x], strict_acgt=True), 0.30, 50, 500, kernel=PBA_KERNEL_BITVEC, strands=strands)
        for col in MAP_COLS:
            assert (g1[col] == w1[col]).all(), (r, col)
        assert [[t1["strand"][k][key] for key in map_ref.STAT_KEYS] for k in range(2)] == [[s1[k][key] for key in map_ref.STAT_KEYS] for k in range(2)], r


def test_redo_behind_failing_hits(ctx, oracle):
    """one read whose true place the narrow pass cannot certify, behind 70 hits that fail in the prefilter: the read is handed
    to the redo, and rows and counters after it are the oracle's"""
    g, x, j = lw.redo_case(oracle)
    mask = eng.mask_from_pattern(lw.MASK_PAT)
    want, wst = oracle.locator(np.frombuffer(g, np.uint8), mask, 0.30, np.frombuffer(x, np.uint8), np.array([0, len(x)], np.uint64), 50, 500)
    T = ctx.seqs_from_list([g], strict_acgt=True)
    rows, st = ctx.locate(ctx.index_build(T, 0, mask, PBA_INDEX_ALL), T, 0, ctx.seqs_from_list([x], strict_acgt=True), 0.30, 50, 500,
                          kernel=PBA_KERNEL_BITVEC)
    prof = ctx.last_profile()
    assert prof["nb_first"] == 1 and prof["n_redo"] == 1
    for col in lw.LOC_COLS:
        assert (rows[col] == want[col]).all(), (col, rows, want)
    assert st == wst and wst["n_located"] == 1 and rows["j"][0] == j
