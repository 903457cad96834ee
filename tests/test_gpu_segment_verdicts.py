"""The verdicts on the diagonal's 32-row segments (align_bitvec.h: segment_done), judged on wave-uniform values: the first
failing row on either side of every boundary the handler knows -- row 11, blocks, superblocks, the ring wrap, the last partial
segment -- lengths that are multiples of 32, of RB and of neither, a segment whose end value fails the shortcut while every
row passes, a failure that only the row-by-row pass finds, and a sweep the all-vs-all walk gives up.  Every input is built on
the CPU and the oracle proves what it is in the test that runs it: a case that drifted fails.  Rows come from align_pairs,
the traced forms and locate; rings 1 and 2.  What each entry point can show: a pba_result has no failing row, so align_pairs
and the traced forms tell a missed or a spurious failure (rc, cost, lengths, scripts) but not row 41 from row 40; the locator's
band-cell counter is a function of the failing row and tells that too, for rows above 32 (the rows up to 32 of a locator pair
belong to the one-lane prefilter).  Rows 11 and 32 are therefore checked for the verdict only.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import align_rings as ar
import test_gpu_align_rings as rings
from conftest import MASK_PAT
from event_schedule_inputs import fail_at
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_INDEX_ALL, PBA_KERNEL_BITVEC

pytestmark = pytest.mark.gpu

# Row f can be the FIRST failing one iff an integer c = cost(f-1, f-1) with c <= (f-1) R and c + 1 > f R exists: at this R
# that holds for every row below (fail_at asserts it per pair)
R = 0.2385
LAST_M, LAST_F = 2100, 2090        # the last, partial segment of a 2 100-row diagonal: rows 2 081 .. 2 100


def fail_cases(NB):
    """(first failing row, length of the shorter side).  RB = 32 NB rows per superblock; 64 * 32 = 2 048 is the ring wrap of
    ring 1 (lane 0's second superblock starts at row 2 049) and a superblock boundary of ring 2."""
    RB = 32 * NB
    return sorted({(11, 11), (11, 40),
                   (32, 32), (32, 45), (33, 33), (33, 64),                    # last row of a block, first row of the next
                   (40, 45), (40, 64),                                        # inside a segment: only the row-by-row pass sees it
                   (RB, RB), (RB, RB + 1), (RB + 1, RB + 1), (RB + 1, 2 * RB),
                   (10 * RB, 10 * RB), (10 * RB, 10 * RB + 7), (10 * RB + 1, 10 * RB + 1), (10 * RB + 1, 11 * RB),
                   (2048, 2048), (2048, 2100), (2049, 2049), (2049, 2100),
                   (LAST_F, LAST_M), (LAST_F, LAST_F)})


TRUE_MS = (64, 96, 100, 1952, 1984, 2001)     # 1 984 = 31 * 64, 1 952 = 61 * 32, 96 = 3 * 32; 100 and 2 001: neither
BUNCH_M, BUNCH_SEG = 160, (65, 96)            # the bunch pair: length, and the segment whose end value is over its first row's bound


def bunch_pair(rng):
    """eight substitutions, one every five rows from row 25, then nine in a row at rows 88 .. 96: cost(96, 96) = 17 is above
    65 R = 15.5, the bound of the segment's first row, and below the bound of every row it was reached in (88 R = 20.99).
    Around the bunch one side has only A / C and the other only G / T there, so no other path is cheaper."""
    x = bytearray(ar.rand_seq(rng, BUNCH_M))
    x[76:108] = np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, 32)].tobytes()
    y = bytearray(x)
    for i in list(range(25, 61, 5)):
        y[i - 1] = ar.ALPHA[(int(np.searchsorted(ar.ALPHA, x[i - 1])) + 1 + rng.randint(3)) % 4]
    y[87:96] = np.frombuffer(b"GT", np.uint8)[rng.randint(0, 2, 9)].tobytes()
    return bytes(x), bytes(y)


def pair_batch(NB) -> ar.Batch:
    rng = np.random.RandomState(9700 + NB)
    B = ar.Batch()
    for k, (f, m) in enumerate(fail_cases(NB)):
        x, y = fail_at(rng, f, m, R)
        y = y + ar.rand_seq(rng, (k % 3) * 20)
        a, b = (y, x) if k % 2 else (x, y)
        B.add_pair(B.place(rng, a, False, ar.MODS[k % 3]), B.place(rng, b, False, ar.MODS[(k + 1) % 3]), False, False,
                   kind="fail", f=f, m=m, tag=f"verdict{NB}:fail{f}:m{m}")
    for k, m in enumerate(TRUE_MS):
        md = ar.max_dst_of(m, m + 1, R)
        for extra in (0, md):
            x = ar.rand_seq(rng, m)
            y = ar.fit(rng, ar.mutate(rng, x, 0.02, head=12), m + extra)
            a, b = (y, x) if (k + extra) % 2 else (x, y)
            B.add_pair(B.place(rng, a, False, ar.MODS[m % 3]), B.place(rng, b, False, ar.MODS[(m + 1) % 3]), False, False,
                       kind="true", m=m, tag=f"verdict{NB}:m{m}+{extra}")
    x, y = bunch_pair(rng)
    B.add_pair(B.place(rng, x, False, 1), B.place(rng, y, False, 31), False, False, kind="bunch", m=BUNCH_M, tag=f"verdict{NB}:bunch")
    return B


def forced(NB, B):
    """ring 1 holds these pairs by themselves; ring 2 behind a pilot of the first max_dst of its plan row"""
    return B if NB == 1 else B.with_pilot(ar.pilot(ar.row_of(2, 2)[0], R))


def prove_pairs(oracle, B):
    """every pair is what it is named for, from the oracle alone"""
    seen = set()
    for q, (meta, x) in enumerate(zip(B.meta, ar.expected(oracle, B, R))):
        if meta["kind"] == "fail":
            assert x["rc"] == -1 and x["fail_row"] == meta["f"] and min(x["len_a"], x["len_b"]) == meta["m"], (meta, x)
            seen.add((meta["f"], meta["m"]))
        elif meta["kind"] == "true":
            assert x["rc"] >= 0 and min(x["len_a"], x["len_b"]) == meta["m"], (meta, x)
        elif meta["kind"] == "bunch":
            a, b = B.elems(q)
            assert oracle.align(a, b, R)["rc"] >= 0                            # every row passes ...
            i0, i1 = BUNCH_SEG
            assert i0 > 32 and oracle.cell(i1, i1)[0] > i0 * R                 # ... though the segment's end value is over its first row's bound
            assert oracle.cell(i0 - 1, i0 - 1)[0] <= (i0 - 1) * R
            seen.add("bunch")
    return seen


@pytest.mark.parametrize("NB", [1, 2])
def test_verdict_rows_align_pairs(ctx, oracle, NB):
    """k_align_pairs<NB>: rc, lengths, max_dst and, where the pair passes, cost and match lengths of every pair against the
    oracle; nothing re-run."""
    B = forced(NB, pair_batch(NB))
    assert prove_pairs(oracle, B) == set(fail_cases(NB)) | {"bunch"}
    assert (LAST_M % 32, LAST_M - LAST_M % 32 < LAST_F <= LAST_M) == (20, True)
    prof = rings.check_batch(ctx, oracle, B, R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == NB and prof["n_first"] == len(B.pairs) and prof["n_redo"] == 0


@pytest.mark.parametrize("form", ["checkpoint", "stream"])
@pytest.mark.parametrize("NB", [1, 2])
def test_verdict_rows_traced(ctx, oracle, NB, form, monkeypatch):
    """k_trace_pairs<NB> in both forms (TRACE == 2 and TRACE == 1 of the sweep): results and edit scripts."""
    B = forced(NB, pair_batch(NB))
    assert prove_pairs(oracle, B) == set(fail_cases(NB)) | {"bunch"}
    if form == "stream":
        monkeypatch.setenv("PBA_TRACE_STREAM", "1")
    prof = rings.check_batch(ctx, oracle, B, R, PBA_KERNEL_BITVEC, scripts=True)
    assert prof["nb_first"] == NB and prof["n_redo"] == 0


def locate_case(NB):
    """A genome that holds, between random spacers, the `b` side of every pair the array gets to judge (first failing row
    above 32: the rows up to 32 belong to the one-lane prefilter), and the `a` sides as reads.  With one probe per read
    (trials = 1) a read is exactly one pair -- the read against the genome from its hit -- so the band cells the locator
    counts for it are those of its failing row.  Ring 2: behind an unrelated filler read that sizes the plan."""
    rng = np.random.RandomState(9800 + NB)
    parts, reads, meta = [ar.rand_seq(rng, 200)], [], []

    def plant(x, y, **m):
        md = ar.max_dst_of(len(x), len(x) + 1, R)
        pos = sum(len(p) for p in parts)
        parts.extend([y, ar.rand_seq(rng, 150)])
        reads.append(x)
        meta.append(dict(pos=pos, md=md, **m))

    for f, m in fail_cases(NB):
        if f > 32:
            x, y = fail_at(rng, f, m, R)
            md = ar.max_dst_of(m, m + 1, R)                                   # (no base in common as far as the band reaches)
            plant(x, y + np.frombuffer(b"GT", np.uint8)[rng.randint(0, 2, md + 40)].tobytes(), kind="fail", f=f, m=m)
    for m in TRUE_MS:
        x = ar.rand_seq(rng, m)
        plant(x, ar.mutate(rng, x, 0.02, head=20) + ar.rand_seq(rng, ar.max_dst_of(m, m + 1, R)), kind="true", m=m)
    x, y = bunch_pair(rng)
    plant(x, y, kind="bunch", m=BUNCH_M)
    if NB == 2:
        reads.append(ar.pilot(ar.row_of(2, 2)[0], R, seed=2)[0])
        meta.append(dict(kind="filler"))
    return np.frombuffer(b"".join(parts), np.uint8), reads, meta


@pytest.mark.parametrize("NB", [1, 2])
def test_verdict_rows_locate(ctx, oracle, NB):
    """k_locate<NB>: rows, pair counts and the band cells (a function of each failing row) against the oracle."""
    g, texts, meta = locate_case(NB)
    gb = g.tobytes()
    seen = set()
    for t, mt in zip(texts, meta):                                            # the pair of each read, from the oracle
        if mt["kind"] == "filler":
            continue
        assert gb.count(t[:16]) == 1 and gb.find(t[:16]) == mt["pos"]          # its one probe hits where it was planted, only
        x = oracle.align(t, gb[mt["pos"]:mt["pos"] + 2 * len(t) + 8], R)
        if mt["kind"] == "fail":
            assert x["rc"] == -1 and x["fail_row"] == mt["f"] > 32 and x["len_a"] == mt["m"], (mt, x)
            seen.add((mt["f"], mt["m"]))
        else:
            assert x["rc"] >= 0 and x["len_a"] == mt["m"], (mt, x)
    assert seen == {c for c in fail_cases(NB) if c[0] > 32} and len(seen) >= 14
    reads = np.frombuffer(b"".join(texts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
    mask = eng.mask_from_pattern(MASK_PAT)
    T = ctx.seqs_from_list([gb], strict_acgt=True)
    Rd = ctx.seqs_from_text(reads, offs, strict_acgt=True)
    ix = ctx.index_build(T, 0, mask, PBA_INDEX_ALL)
    rows, st = ctx.locate(ix, T, 0, Rd, R, 1, 33, kernel=PBA_KERNEL_BITVEC)
    prof = ctx.last_profile()
    assert prof["nb_first"] == NB and prof["n_redo"] == 0
    want, wst = oracle.locator(g, mask, R, reads, offs, 1, 33, nthreads=8)
    for c in ("nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs"):
        assert (rows[c] == want[c]).all(), c
    assert st == wst, (st, wst)
    n = sum(mt["kind"] != "filler" for mt in meta)
    assert wst["n_pairs"] == n and wst["n_located"] == n - len(seen)
    for r, mt in enumerate(meta):                                             # locator.cpp:86: the cell at the end of the diagonal
        if mt["kind"] in ("true", "bunch"):
            x = oracle.align(texts[r], gb[mt["pos"]:mt["pos"] + 2 * len(texts[r]) + 8], R)
            m = min(x["len_a"], x["len_b"])
            assert int(rows["diag_cost"][r]) == oracle.cell(m, m)[0], mt


# ----------------------------------------------------------------------------- a sweep the all-vs-all walk gives up
BAIL_R, BAIL_M, BAIL_E = 0.9, 2200, 0.85


def test_bail_through_the_overlap_walk(ctx, oracle):
    """Two reads with a common 40-base head, one over A / C, the other a copy with 85 % of its bases behind the head replaced
    by G / T: cost(i, i) is the number of replaced bases among the first i, whatever the path.  At R = 0.9 every row passes,
    max_dst = 1 981 is beyond the one-block ring's window (1 384), and at row 1 024 the diagonal projects a cost above that
    window with four standard deviations to spare: the narrow sweep is given up there (bitvec_pass: BAIL), the run is parked
    and resumed at the reference band, and the rows are the oracle's.  What this cannot show: a sweep that never gave up
    would end uncertified (cost above the window), be parked all the same and give the same rows and counters -- no counter
    of the walk separates the two.  The CPU side proves that the condition holds at row 1 024; the GPU side is held to the
    ring that condition was proved for (the whole call in the narrow ring of its plan, both runs parked by it) and to an
    unchanged result."""
    rng = np.random.RandomState(9900)
    head = ar.rand_seq(rng, 40)
    x = head + np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, BAIL_M - 40)].tobytes()
    yb = bytearray(x)
    u = rng.rand(BAIL_M)
    for i in range(40, BAIL_M):
        if u[i] < BAIL_E:
            yb[i] = b"GT"[rng.randint(2)]
    texts = [x, bytes(yb)]
    md = ar.max_dst_of(BAIL_M, BAIL_M, BAIL_R)
    w = ar.bv_pass1_w(md, 1)
    assert ar.nb1(md) == 1 and w == 1384 < md
    res = oracle.align(texts[0], texts[1], BAIL_R)
    assert res["rc"] >= 0 and res["cost"] > w                                  # the reference accepts it, beyond the window
    f32 = np.float32
    end = oracle.cell(1024, 1024)[0]
    assert end == sum(c in b"GT" for c in texts[1][40:1024])
    for i in range(32, 1024, 32):                                             # nothing fails or is given up before row 1 024 ...
        assert oracle.cell(i, i)[0] <= i * BAIL_R
    assert (f32(end) - f32(4.0) * np.sqrt(f32(end))) * f32(BAIL_M) > f32(1024) * f32(w) * f32(1.05)   # ... and there it is, clearly
    file = b"".join(eng.text2bin(t) for t in texts)
    rec_offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in texts[:-1]]).astype(np.uint64)
    mask = eng.mask_from_pattern(MASK_PAT)
    want, pairs = [], 0
    for t in range(2):
        rows = oracle.spaced_round(texts[t], mask, BAIL_R, file, rec_offs, 32, 64, buggy=False, nthreads=2)
        pairs += int(rows["n_pairs"].sum()) - int(rows["n_pairs"][t])
        for q in range(2):
            if q != t and rows["found"][q]:
                want.append((t, q, int(rows["j"][q]), int(rows["dir"][q]), int(rows["ref_pos"][q]), int(rows["cost"][q]),
                             int(rows["matlen_a"][q]), int(rows["matlen_b"][q])))
    assert len(want) == 2 and all(r[2] == 0 and r[4] == 0 and r[5] > w for r in want)    # found by the head probe, beyond the window
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    got, st = ctx.overlap_all(S, mask, BAIL_R, 32, 64, kernel=PBA_KERNEL_BITVEC)
    assert [tuple(int(v) for v in r) for r in got] == want
    # every item of so small a call is in the sample, which runs in the plan's narrow ring (ring 1 for this max_dst, above):
    # no part of it started wider, and that ring parked both runs
    assert st["wide_first"] == 0 and st["n_redo"] == 2 and st["n_pairs"] == pairs
