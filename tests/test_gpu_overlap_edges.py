"""The bookkeeping of the all-vs-all scan held to a plain model (overlap_ref.py: enumeration, index_ref's seedmap, the oracle's
verdict per candidate) on the inputs of overlap_edge_inputs.py; test_overlap_edges_cpu.py proves what each input is and that
the model is the oracle's spaced_seed round, target by target.  Every comparison is exact, and both forms of the kernels are
held to the model, never only to each other.

  PBA_OVL_COMPACT, locate     k_ovl_scan and k_ovl_fill (which expands the same macros): buckets of 1 .. 520 entries, rounds of
                              exactly 64 and of 65 slots, a run that starts at slot 64 behind a long run / behind 64 runs of one,
                              three slot groups with survivors at lanes 0, 31, 32, 63 of each, a full round of 512 runs, runs in
                              every wavefront, both halves, a second step and the last live chunk -- n_candidates, n_prefiltered,
                              n_listed and the rows say whether every slot met its own run's record
  ovl_rule: ord_of, pos_of    targets of 20 015 .. 50 000 bases with copies on either side of position 20 000, of tail_lo and of
                              tail_top, and one key at two head and two tail positions: the scan, count / fill, the walk's
                              decode and k_ovl_after
  k_ovl_after                 max_trial 1, 2, 33, 63 (t2 = 66 and 126: the second ballot round) on queries whose later probes do
                              not exist, have a zero key, miss the gate by one, repeat the success's key or one another's
  k_probe_emit                the entries themselves, whole sets and shards, and a buffer that is too short

What this cannot show: the order of a bucket's entries is the table's fill order, so which lane a member of a bucket of N
lands in is not the input's to choose -- lanes are pinned through runs of one only.
Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import overlap_edge_inputs as oi
import overlap_ref as orf
import prefilter_inputs as pi
from conftest import MASK_PAT
from pacbioassembly_amd import _lib
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP
from test_gpu_parity import prekeep  # noqa: F401  (the three ways the scan sizes the survivors' slices)

pytestmark = pytest.mark.gpu

KERNELS = (PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP)
COLS = ("target", "query", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b")


def rows_of(got):
    return [tuple(int(r[c]) for c in COLS) for r in got]


def check(got, st, W, kernel, what):
    """rows and counters against the model's"""
    print(what, kernel, {k: st[k] for k in ("n_candidates", "n_pairs", "n_overlaps", "n_listed", "n_prefiltered", "n_probe_entries", "cap_overflow")})
    assert rows_of(got) == W["rows"], what
    assert st["n_overlaps"] == len(W["rows"]) and st["n_pairs"] == W["pairs"], (what, st)
    assert st["n_candidates"] == W["n_match"] and st["n_probe_entries"] == W["n_probe_entries"], (what, st)
    if kernel == PBA_KERNEL_BITVEC:
        assert (st["n_prefiltered"], st["n_listed"]) == (W["n_pre"], W["n_listed"]), (what, st)


@pytest.mark.parametrize("case", oi.CASES, ids=oi.case_id)
def test_overlap_edges(ctx, oracle, prekeep, case):
    """pba_overlap_all, both kernels, every way of sizing the slices: rows, n_overlaps, n_pairs, n_candidates and
    n_probe_entries equal to the model's; for the bit-vector kernels n_prefiltered and n_listed as well."""
    W = oi.expected(oracle, case)
    assert eng.mask_from_pattern(case[2] if case[0] == "run" else MASK_PAT) == W["mask"]
    S = ctx.seqs_from_list(W["texts"], strict_acgt=True)
    for kernel in KERNELS:
        got, st = ctx.overlap_all(S, W["mask"], W["R"], W["max_trial"], W["overlap_min"], kernel=kernel)
        check(got, st, W, kernel, oi.case_id(case))


@pytest.mark.parametrize("case", oi.VIEW_CASES, ids=oi.case_id)
def test_overlap_edges_in_target_ranges_and_on_the_other_strand(ctx, oracle, prekeep, case):
    """the same through overlap_all_sharded (one table, ranges of seven targets) and through the reverse-complement pass of
    pba_overlap_strands over the set with its query reads flipped"""
    W = oi.expected(oracle, case)
    S = ctx.seqs_from_list(W["texts"], strict_acgt=True)
    V = oi.expected(oracle, case, "rc")
    Sv = ctx.seqs_from_list(V["texts"], strict_acgt=True)
    for kernel in KERNELS:
        got, st = ctx.overlap_all_sharded(S, W["mask"], W["R"], W["max_trial"], W["overlap_min"], targets_per_call=7, kernel=kernel)
        check(got, st, W, kernel, oi.case_id(case) + " sharded")
        got, sts = ctx.overlap_strands(Sv, V["mask"], V["R"], V["max_trial"], V["overlap_min"], strands=2, kernel=kernel)
        assert (got["strand"] == -1).all() and len(V["rows"]) > 0
        check(got, sts[1], V, kernel, oi.case_id(case) + " rc")


def test_census_that_misses(ctx, oracle, monkeypatch):
    """1 040 targets are sized from every 16th; none of those has a candidate, read 1 has 144 survivors: the range overflows
    its equal room and is scanned again -- with no hook set -- and the answer is the model's."""
    for k in ("PBA_OVL_ROOM", "PBA_OVL_CAPFILL_PCT", "PBA_OVL_SAMPLE_MIN", "PBA_OVL_MAX_CANDIDATES", "PBA_OVL_WIDE"):
        monkeypatch.delenv(k, raising=False)
    W = oi.expected(oracle, ("census",))
    S = ctx.seqs_from_list(W["texts"], strict_acgt=True)
    got, st = ctx.overlap_all(S, W["mask"], W["R"], W["max_trial"], W["overlap_min"], kernel=PBA_KERNEL_BITVEC)
    check(got, st, W, PBA_KERNEL_BITVEC, "census")
    assert st["cap_overflow"] == 1 and st["cap_fill"] == 0, st
    got, st = ctx.overlap_all(S, W["mask"], W["R"], W["max_trial"], W["overlap_min"], kernel=PBA_KERNEL_ROWSWEEP)
    check(got, st, W, PBA_KERNEL_ROWSWEEP, "census")


@pytest.mark.parametrize("case", oi.SHORT_CASES, ids=oi.case_id)
def test_probe_table_scan_small_and_tiled(ctx, oracle, case):
    """masks of six and of seven care bases: the probe table's 4 096 bucket counts are scanned by one workgroup (k_scan_small),
    its 16 384 by the tiled form; rows and counters of both kernels are the model's"""
    W = oi.expected(oracle, case)
    assert eng.mask_from_pattern(case[1]) == W["mask"] and len(W["rows"]) >= 20
    S = ctx.seqs_from_list(W["texts"], strict_acgt=True)
    for kernel in KERNELS:
        got, st = ctx.overlap_all(S, W["mask"], W["R"], W["max_trial"], W["overlap_min"], kernel=kernel)
        check(got, st, W, kernel, oi.case_id(case))


PROBE_CASES = [("run", "misc", MASK_PAT), ("run", "misc", pi.HEAVY_PAT), ("after", "main", 1, 10), ("after", "main", 2, 10),
               ("after", "main", 33, 10), ("after", "main", 63, 10), ("ht", 40017)]


@pytest.mark.parametrize("case", PROBE_CASES, ids=oi.case_id)
def test_probe_entries(ctx, oracle, case):
    """pba_overlap_probes: the entries key << 32 | (q t2 + 2 j + backward), sorted, are the model's -- of the whole set, of
    query shards -- and a buffer shorter than the count is refused with nothing written behind it."""
    import torch
    S, R, pat, mt, om = oi.case_params(case)
    mask = orf.mask_of(pat)
    n = len(S.texts)
    want = orf.probe_entries(S.texts, mask, mt)
    assert 0 < want.size <= n * 2 * mt and (mt == 1 or want.size < n * 2 * mt)  # (short reads and zero keys: not every slot is an entry)
    D = ctx.seqs_from_list(S.texts, strict_acgt=True)
    GUARD = 8
    for lo, hi in ((0, n), (0, n // 3), (n // 3, n // 3 + 1), (n // 3 + 1, n), (n, n)):
        w = orf.probe_entries(S.texts, mask, mt, lo, hi)
        buf = torch.full((w.size + GUARD,), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        cnt = ctx.overlap_probes(D, lo, hi, mask, mt, buf.data_ptr(), w.size)
        host = buf.cpu().numpy().view(np.uint64)
        assert cnt == w.size and (np.sort(host[:cnt]) == w).all(), (lo, hi)
        assert (host[cnt:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    cap = want.size - 3
    buf = torch.full((cap + GUARD,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(eng.PbaError) as e:
        ctx.overlap_probes(D, 0, n, mask, mt, buf.data_ptr(), cap)
    assert e.value.status == _lib.PBA_E_INVALID
    host = buf.cpu().numpy().view(np.uint64)
    assert (host[cap:] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()                  # nothing behind the buffer's end
    assert np.isin(host[:cap], want).all() and np.unique(host[:cap]).size == cap   # ... and cap of the entries before it
