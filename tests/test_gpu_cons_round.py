"""The unlocked round (pba_cons_round over k_spaced_round / ss_try) at every growth, deferral and gate edge, and ss_try's own
gates in the locked round (pba_spaced_round), against the serial oracle on the planted inputs of cons_round_inputs.py.

Every unlocked case names in meta['line'] the line of ss_try / pba_cons_round it stands on; what makes it that case is
shown on the oracle alone in test_cons_round_inputs_cpu.py.  The rows are the check: a read taken against a text that an
earlier pool read should have grown first comes back with another matlen, or not found."""
import numpy as np
import pytest

import cons_round_inputs as ci
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP, PbaError
from test_cons_round_inputs_cpu import BY_NAME, COLS, UNLOCKED, IDS, locked_rows, must_rewalk, oracle_round

pytestmark = pytest.mark.gpu

KERNELS = [PBA_KERNEL_ROWSWEEP, PBA_KERNEL_BITVEC]
PBA_E_TOOLONG = -4


def same(got, want, what):
    """element-wise equality that names the first element that differs (the row, the box)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "first at", bad[0].tolist(), "got", got[tuple(bad[0])], "want", want[tuple(bad[0])], "of", len(bad))


def same_rows(got, want, what, cols=COLS):
    for c in cols:
        same(got[c], want[c], (what, c))


def mask_of(oracle):
    return oracle.mask_from_pattern(ci.PATTERN)


def check_round(c, Rd, case, pool, o, tag, kernel, mask, text_len):
    """one round of `c` against the oracle's record o[...+tag]; returns the stats"""
    name = (case.meta["name"], kernel, "round" + (tag or "1"))
    rows, st = c.round(Rd, pool, mask, ci.R, case.max_trial, case.overlap_min, buggy_seed_at=False, kernel=kernel)
    want = o["rows" + tag]
    same_rows(rows, want, name)
    assert c.extent() == o["ext" + tag], name
    sel, sup, tot, _ = c.dump()
    same(tot, o["tot" + tag], (name, "tot")); same(sel, o["sel" + tag], (name, "sel")); same(sup, o["sup" + tag], (name, "sup"))
    assert c.text() == o["text" + tag], name
    m = must_rewalk(case, want, pool, text_len)
    assert st["n_found"] == int(want["found"].sum()), (name, st)
    assert (st["n_grown_fwd"], st["n_grown_bwd"]) == (m["n_grown_fwd"], m["n_grown_bwd"]), (name, st, m)
    assert st["n_deferred"] >= m["n_rewalk"] and st["n_batches"] >= m["depth"], (name, st, m)
    assert c.evolve() == o["evolved" + tag], name
    return st


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("case", UNLOCKED, ids=IDS)
def test_unlocked_round_equals_the_serial_oracle(ctx, oracle, case, kernel):
    """Consensus.round == the oracle's serial round (spaced_seed.cpp:420-446) on the line named by case.meta['line']: all ten
    row columns in pool order, the extent, every vote box, the text before and after evolve -- and again for a second
    round over another pool on the evolved object, which starts from beg = pre.  The stats are held to the sequential
    restatement: as many growths per end, at least the re-walks and batches it requires, and exactly one batch with
    nothing deferred where no read touches an end that grew (batching must not decay into a read per launch)."""
    o = oracle_round(oracle, case)
    file, offs = ci.records(case.reads)
    Rd = ctx.seqs_from_records(file, 0, 1 << 30)
    assert Rd.count == len(case.reads)
    mask = mask_of(oracle)
    c = eng.Consensus(ctx, case.text, case.weight)
    st = check_round(c, Rd, case, case.pool, o, "", kernel, mask, len(case.text))
    meta = case.meta
    if meta.get("one_batch"):
        assert st["n_batches"] == 1 and st["n_deferred"] == 0, (meta["name"], st)
    if "interior" in meta:          # a read is walked once per batch at the most, an interior read once
        assert st["n_deferred"] <= (len(case.pool) - len(meta["interior"])) * (st["n_batches"] - 1), (meta["name"], st)
    check_round(c, Rd, case, meta["pool2"], o, "2", kernel, mask, len(o["evolved"]))


@pytest.mark.parametrize("kernel", KERNELS)
def test_rows_outside_the_pool_come_back_untouched(ctx, oracle, kernel):
    """spaced_round_subset / pba_cons_round write rows[pool[k]] only: a pool in non-ascending order that is a strict subset
    of the set leaves the caller's other rows as they were."""
    case = BY_NAME["subset_pool"]
    o = oracle_round(oracle, case)
    file, offs = ci.records(case.reads)
    Rd = ctx.seqs_from_records(file, 0, 1 << 30)
    c = eng.Consensus(ctx, case.text, case.weight)
    pool = np.ascontiguousarray(case.pool, np.uint32)
    rows = np.zeros(Rd.count, eng.SS_ROW_DTYPE)
    for col in COLS:
        rows[col] = -77
    st = np.zeros(6, np.int32)
    ctx.check(ctx.lib.pba_cons_round(ctx.h, c.h, Rd.h, eng._ptr(pool), pool.size, mask_of(oracle), ci.R,
                                     case.max_trial, case.overlap_min, 0, kernel, 26000, 6000, eng._ptr(rows),
                                     eng._ptr(st)), "cons_round")
    same_rows(rows[pool], o["rows"], ("subset_pool", kernel))
    for r in case.meta["outside"]:
        assert all(int(rows[col][r]) == -77 for col in COLS), (r, rows[r])


@pytest.mark.parametrize("side", ci.SIDES)
def test_growth_past_the_buffer_is_refused(ctx, oracle, side):
    """pba_cons_append / pba_cons_prepend inside pba_cons_round: a growth past 3 * max_len, or before the buffer's start,
    answers PBA_E_TOOLONG.  Nothing is asked of the refused object; a fresh one on the same ctx runs the first case."""
    case = {c.meta["name"]: c for c in ci.toolong_cases()}[f"toolong_{side}"]
    file, offs = ci.records(case.reads)
    Rd = ctx.seqs_from_records(file, 0, 1 << 30)
    c = eng.Consensus(ctx, case.text, case.weight, max_len=case.meta["max_len"])
    with pytest.raises(PbaError) as e:
        c.round(Rd, case.pool, mask_of(oracle), ci.R, case.max_trial, case.overlap_min)
    assert e.value.status == PBA_E_TOOLONG
    first = UNLOCKED[0]
    file, offs = ci.records(first.reads)
    Rd = ctx.seqs_from_records(file, 0, 1 << 30)
    c = eng.Consensus(ctx, first.text, first.weight)
    check_round(c, Rd, first, first.pool, oracle_round(oracle, first), "", eng.PBA_KERNEL_AUTO, mask_of(oracle), len(first.text))


# ------------------------------------------------------------------------------------------------ locked-round gates
def locked_gpu(ctx, oracle, ring):
    reads, names, nc = ci.locked_reads(ring)
    file, offs = ci.records(reads)
    Rf = ctx.seqs_from_list([ci.locked_ref()])
    Rd = ctx.seqs_from_records(file, 0, 1 << 30)
    assert Rd.count == len(reads)
    ix = ctx.index_build(Rf, 0, mask_of(oracle), eng.PBA_INDEX_HEAD_TAIL)
    return Rf, Rd, ix, names, nc


@pytest.mark.parametrize("buggy", (False, True))
@pytest.mark.parametrize("ring", (1, 2))
def test_locked_round_gates(ctx, oracle, ring, buggy):
    """ss_try in the locked round == the oracle on every column, both kernels, both seed placements, in a call that plans
    ring 1 and in one that plans ring 2: hit lists of 1, 64, 65, 66, 129 and 130 candidates (the loop over hits, 64 at a
    time); key 0 (no trial); reads of 15 .. 80 bases (pos + 16 > slen, s_len < overlap_min, either direction); a first
    candidate with matlen_a = overlap_min - 1 before one that passes; forward before backward at the same j."""
    Rf, Rd, ix, names, nc = locked_gpu(ctx, oracle, ring)
    want = locked_rows(oracle, ring, buggy)
    for kernel in KERNELS:
        got = ctx.spaced_round(ix, Rf, 0, Rd, ci.R, ci.LOCK_MAX_TRIAL, ci.LOCK_OVERLAP_MIN, buggy_seed_at=buggy, kernel=kernel)
        for c in COLS:
            bad = np.flatnonzero(got[c][:nc] != want[c][:nc])
            assert bad.size == 0, (kernel, c, [(names[k], int(got[c][k]), int(want[c][k])) for k in bad[:6]])


@pytest.mark.parametrize("max_trial", (0, 1))
def test_locked_round_probe_counts(ctx, oracle, max_trial):
    """k_spaced_round: for (j = 0; j < max_trial; ...) -- no probe at all, and the two probes of j = 0 only."""
    Rf, Rd, ix, names, nc = locked_gpu(ctx, oracle, 1)
    for buggy in (False, True):
        want = locked_rows(oracle, 1, buggy, max_trial)
        for kernel in KERNELS:
            got = ctx.spaced_round(ix, Rf, 0, Rd, ci.R, max_trial, ci.LOCK_OVERLAP_MIN, buggy_seed_at=buggy, kernel=kernel)
            same_rows(got[:nc], want[:nc], (max_trial, buggy, kernel))


# ------------------------------------------------------------------------------------------------ the loop entry points
ASM_CFG = dict(R=ci.R, max_trial=4, overlap_min=64, max_round=6, picks=[1, 0, 1, 1, 0])
ASM_PATTERNS = ("111*11*11*1*1111", "1111*1*11**11*111")


def test_assemble_over_the_both_ends_pool(ctx, oracle):
    """pba_cons_assemble (seed_rounds over pba_cons_round, evolve between rounds) over growers and followers on both ends, an
    interior read and a foreign one, two masks == run_assembly on the oracle: rounds, rows, lengths, final text."""
    from cons_scenarios import run_assembly
    masks = [oracle.mask_from_pattern(p) for p in ASM_PATTERNS]
    reads = ci.both_ends_reads() + [ci.interior(1200), ci.genome(77, 1000)]
    file, offs = ci.records(reads)
    class Serial:                                 # the oracle's object with the intended seed placement
        def __init__(s): s.c = oracle.consensus(ci.text_of(), 1)
        def round(s, mask, R, mt, f, ro, pool): return s.c.round(mask, R, mt, f, ro, pool, buggy=False)
        def evolve(s): s.c.evolve()
        def dump(s): return s.c.dump(40000)
        def text(s): return s.c.text(40000)
    want = run_assembly(Serial(), masks, file, offs, len(reads), ASM_CFG)
    assert len(want["rounds"]) == 3 and len(want["rounds"][0]["found"]) == 5 and want["rounds"][0]["extent"][:2] == [-400, 3400]
    Rd = ctx.seqs_from_records(file, 0, 1 << 30)
    for kernel in KERNELS:
        c = eng.Consensus(ctx, ci.text_of(), 1)
        rows, fr, log = c.assemble(Rd, ASM_CFG["R"], masks, ASM_CFG["picks"], ASM_CFG["max_round"], ASM_CFG["max_trial"],
                                   ASM_CFG["overlap_min"], buggy_seed_at=False, kernel=kernel)
        assert [[l["round"], l["mask"], l["n_tried"], l["n_found"], l["ref_len"]] for l in log] == \
            [[r["round"], r["mask"], r["n_tried"], len(r["found"]), r["ref_len"]] for r in want["rounds"]], kernel
        want_round = {f[0]: r["round"] for r in want["rounds"] for f in r["found"]}
        assert fr.tolist() == [want_round.get(i, 0) for i in range(len(reads))]
        for r in want["rounds"]:
            for f in r["found"]:
                assert [int(rows[c_][f[0]]) for c_ in ("read", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b")] == f, kernel
        assert c.text().decode() == want["final_text"], kernel


def test_spaced_multi_over_the_hit_lists(ctx, oracle):
    """pba_spaced_multi (seed_rounds over spaced_round_subset with a shrinking pool) over the locked-gate reads, three
    masks == multi_rounds over the oracle's locked round."""
    from cons_scenarios import MULTI, multi_rounds
    masks = [oracle.mask_from_pattern(p) for p in ASM_PATTERNS + ("11*1111**1*11*111",)]
    reads, names, nc = ci.locked_reads(1)
    file, offs = ci.records(reads)
    ref = ci.locked_ref()
    fn = lambda mask, pool: oracle.spaced_round(ref, mask, ci.R, file, offs[pool], 2, ci.LOCK_OVERLAP_MIN, buggy=False, nthreads=4)
    w_round, w_log, w_final = multi_rounds(fn, masks, len(reads))
    assert sum(1 for x in w_round if x) >= 12 and len(w_log) >= 4
    Rf = ctx.seqs_from_list([ref])
    Rd = ctx.seqs_from_records(file, 0, 1 << 30)
    for kernel in KERNELS:
        rows, fr, log = ctx.spaced_multi(Rf, 0, Rd, ci.R, masks, MULTI["picks"], MULTI["max_round"], 2, ci.LOCK_OVERLAP_MIN,
                                         buggy_seed_at=False, kernel=kernel)
        assert [[l["round"], l["mask"], l["n_tried"], l["n_found"]] for l in log] == w_log, kernel
        assert fr.tolist() == w_round, kernel
        for r, w in enumerate(w_final):
            assert [int(rows[c][r]) for c in ("found", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b")] == w, (kernel, names[r])
