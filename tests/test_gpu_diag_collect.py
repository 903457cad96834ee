"""Where the diagonal's D0 bits are collected (align_bitvec.h: bitvec_pass).  The one-hot of the diagonal cell is one scalar
per wavefront and every lane ORs bits into the word of the diagonal's block, so a lane that does not hold the diagonal
collects garbage until the diagonal enters it; only the word of the diagonal's lane and block is ever read (the form of the
all-vs-all walk keeps the one-hot in the diagonal's lane, and collects in every block of it).  What can go
wrong shows in two directions: a stale bit lowers D(i,i) and a failing pair passes; a bit taken from the wrong block or at
the wrong position raises it and a true pair fails, or a failing pair fails at an earlier row.  So: pairs whose first failing
row sits at the first, second, 31st and last row of every block of superblocks 1, 2, 64 (the first after the ring wrap, whose
lane has collected garbage for a whole revolution) and 65, each once as the last row of the pair and once with clean rows
behind it (a missed failure then passes), and true pairs whose diagonal touches the bound at every segment end.  Half of
the failing pairs and all the true ones interleave matches and substitutions at a density near R (hug_pair): with runs of
equal bits a collection shifted by one position would go unseen.  Every input is built on the CPU and the oracle proves what
it is in the test that runs it.  Rings 1 and 2, ring 3 (every block's word collects there) for superblocks 0 .. 2; through
align_pairs, both traced forms, locate (one probe per read: the band-cell counter is a function of the failing row) and the
all-vs-all walk.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import align_rings as ar
import test_gpu_align_rings as rings
from conftest import MASK_PAT
from diag_collect_inputs import (BEHIND, HEAD, POS, ROW, SUPERBLOCKS, can_fail_first, fail_rows, groups_of, hug_pair,  # noqa: F401
                                 touches_bound)
from event_schedule_inputs import fail_at
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_INDEX_ALL, PBA_KERNEL_BITVEC

pytestmark = pytest.mark.gpu

GROUPS = {NB: groups_of(NB) for NB in (1, 2, 3)}
RS = {NB: GROUPS[NB][0][0] for NB in (1, 2, 3)}      # (the true pairs and the locator's cases run under the first R)


def true_ms(NB):
    """lengths whose last segment has 1, 31 and 32 rows in block 0 and in block 1 of superblock 2; the diagonal entering a
    superblock and ending on its first row; the same behind the ring wrap"""
    RB = 32 * NB
    ms = {2 * RB + 32 * nb + k for nb in range(min(NB, 2)) for k in (1, 31, 32)} | {s * RB + 1 for s in (1, 2, 3)}
    return sorted(ms | ({64 * RB + 1} if NB <= 2 else set()))


def pair_batch(NB, g=0) -> ar.Batch:
    """the pairs of group g of the ring: its failing rows, and with group 0 the true pairs"""
    (R, rows), RB = GROUPS[NB][g], 32 * NB
    rng = np.random.RandomState(9950 + 10 * g + NB)
    B = ar.Batch()
    for k, f in enumerate(rows):
        for last in (True, False):
            m = f if last else f + BEHIND
            shape = "hug" if (k + last) % 2 else "plain"
            x, y = hug_pair(rng, m, R, f, f) if shape == "hug" else fail_at(rng, f, m, R)
            y = y + ar.rand_seq(rng, (k % 3) * 20)
            a, b = (y, x) if k % 2 else (x, y)
            B.add_pair(B.place(rng, a, False, ar.MODS[k % 3]), B.place(rng, b, False, ar.MODS[(k + 1) % 3]), False, False,
                       kind="fail", f=f, m=m, shape=shape, tag=f"collect{NB}:{shape}:fail{f}:m{m}")
    for k, m in enumerate(true_ms(NB) if g == 0 else []):
        x, y = hug_pair(rng, m, R, 3 * RB)
        y = y + ar.rand_seq(rng, (k % 2) * ar.max_dst_of(m, m + 1, R))
        a, b = (y, x) if k % 3 == 1 else (x, y)
        B.add_pair(B.place(rng, a, False, ar.MODS[m % 3]), B.place(rng, b, False, ar.MODS[(m + 1) % 3]), False, False,
                   kind="true", m=m, tag=f"collect{NB}:true:m{m}")
    return B


def forced(NB, B, R):
    """ring 1 holds these pairs by themselves; rings 2 and 3 behind a pilot of the first max_dst of their plan row"""
    return B if NB == 1 else B.with_pilot(ar.pilot(ar.row_of(*ROW[NB])[0], R))


def prove_pairs(oracle, B, NB, R):
    """every pair is what it is named for, from the oracle alone; the failing (row, last row or not) seen"""
    seen = set()
    for q, (meta, x) in enumerate(zip(B.meta, ar.expected(oracle, B, R))):
        if meta["kind"] == "fail":
            assert x["rc"] == -1 and x["fail_row"] == meta["f"] and min(x["len_a"], x["len_b"]) == meta["m"], (meta, x)
            seen.add((meta["f"], meta["m"] == meta["f"]))
        elif meta["kind"] == "true":
            a, b = B.elems(q)
            assert oracle.align(a, b, R)["rc"] >= 0 and min(x["len_a"], x["len_b"]) == meta["m"], (meta, x)
            assert touches_bound(oracle, a, b, meta["m"], R, 32 * NB), meta
    return seen


def all_cases(NB):
    return {(f, last) for f in fail_rows(NB) for last in (True, False)}


def test_inputs_cover_the_blocks():
    """the rows the cases are named for, from the ring's geometry alone"""
    for NB in (1, 2, 3):
        RB = 32 * NB
        got = {((f - 1) // RB, ((f - 1) % RB) >> 5, (f - 1) % 32 + 1) for f in fail_rows(NB)}
        want = {(s, nb, p) for s in SUPERBLOCKS[NB] for nb in range(NB) for p in POS} - {(0, 0, 1), (0, 0, 2)}   # rows <= 10: never checked
        assert got == want and sorted(f for _, rows in GROUPS[NB] for f in rows) == fail_rows(NB)
        assert ar.nb1(ar.row_of(*ROW[NB])[0]) == NB and (NB == 3 or len(GROUPS[NB]) == 1)
        meta = [m for g in range(len(GROUPS[NB])) for m in pair_batch(NB, g).meta if m["kind"] == "fail"]
        assert {m["shape"] for m in meta if m["m"] == m["f"]} == {"hug", "plain"}
        assert {m["shape"] for m in meta if m["m"] > m["f"]} == {"hug", "plain"}


@pytest.mark.parametrize("NB", [1, 2, 3])
def test_collect_align_pairs(ctx, oracle, NB):
    """k_align_pairs<NB>: rc, lengths, max_dst and, where the pair passes, cost and match lengths against the oracle; nothing
    re-run."""
    seen = set()
    for g, (R, _) in enumerate(GROUPS[NB]):
        B = forced(NB, pair_batch(NB, g), R)
        seen |= prove_pairs(oracle, B, NB, R)
        prof = rings.check_batch(ctx, oracle, B, R, PBA_KERNEL_BITVEC)
        assert prof["nb_first"] == NB and prof["n_first"] == len(B.pairs) and prof["n_redo"] == 0
    assert seen == all_cases(NB)


@pytest.mark.parametrize("form", ["checkpoint", "stream"])
@pytest.mark.parametrize("NB", [1, 2, 3])
def test_collect_traced(ctx, oracle, NB, form, monkeypatch):
    """k_trace_pairs<NB> in both forms (TRACE == 2 and TRACE == 1 of the sweep): results and edit scripts."""
    if form == "stream":
        monkeypatch.setenv("PBA_TRACE_STREAM", "1")
    seen = set()
    for g, (R, _) in enumerate(GROUPS[NB]):
        B = forced(NB, pair_batch(NB, g), R)
        seen |= prove_pairs(oracle, B, NB, R)
        prof = rings.check_batch(ctx, oracle, B, R, PBA_KERNEL_BITVEC, scripts=True)
        assert prof["nb_first"] == NB and prof["n_redo"] == 0
    assert seen == all_cases(NB)


def locate_case(NB):
    """A genome that holds, between random spacers, the `b` side of every pair, and the `a` sides as reads.  With one probe
    per read (trials = 1) a read is exactly one pair -- the read against the genome from its hit -- so the band cells the
    locator counts for it are those of its failing row.  Ring 2: behind an unrelated filler read that sizes the plan."""
    R, RB = RS[NB], 32 * NB
    rng = np.random.RandomState(9960 + NB)
    parts, reads, meta = [ar.rand_seq(rng, 200)], [], []

    def plant(x, y, **m):
        pos = sum(len(p) for p in parts)
        parts.extend([y, ar.rand_seq(rng, 150)])
        reads.append(x)
        meta.append(dict(pos=pos, **m))

    for k, f in enumerate(fail_rows(NB)):
        for last in (True, False):
            m = f if last else f + BEHIND
            x, y = fail_at(rng, f, m, R) if (k + last) % 2 else hug_pair(rng, m, R, f, f)
            md = ar.max_dst_of(m, m + 1, R)                                   # (no base in common as far as the band reaches)
            tail = np.frombuffer(b"GT" if set(x[-8:]) <= set(b"AC") else b"AC", np.uint8)[rng.randint(0, 2, md + 40)].tobytes()
            plant(x, y + (tail if last else ar.rand_seq(rng, md + 40)), kind="fail", f=f, m=m)
    for m in true_ms(NB):
        x, y = hug_pair(rng, m, R, 3 * RB)
        plant(x, y + ar.rand_seq(rng, ar.max_dst_of(m, m + 1, R)), kind="true", m=m)
    if NB == 2:
        reads.append(ar.pilot(ar.row_of(2, 2)[0], R, seed=2)[0])
        meta.append(dict(kind="filler"))
    return np.frombuffer(b"".join(parts), np.uint8), reads, meta


@pytest.mark.parametrize("NB", [1, 2])
def test_collect_locate(ctx, oracle, NB):
    """k_locate<NB>: rows, pair counts and the band cells (a function of each failing row) against the oracle."""
    R = RS[NB]
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
            seen.add((mt["f"], mt["m"] == mt["f"]))
        else:
            assert x["rc"] >= 0 and x["len_a"] == mt["m"], (mt, x)
    assert seen == all_cases(NB)
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


# ----------------------------------------------------------------------------- the all-vs-all walk (the BAIL form), ring 2
WALK_R, WALK_LEN, WALK_F = 0.30, 8300, 103       # row 103: superblock 1 of ring 2 (rows 65 .. 128), block 1, bit 6


def test_collect_through_the_overlap_walk(ctx, oracle):
    """Two pairs of 8.3 kb reads (max_dst 2 491: ring 2), each a read and its copy with substitutions that keep the diagonal on
    the bound through three superblocks.  The first pair has one substitution more at row 103 -- behind the 64 rows of the
    one-lane prefilter, in block 1 -- and is clean behind it: the reference fails it there, a sweep that missed that bit would
    report an overlap.  The second pair passes and must be found.  One probe per read, so a pair is one alignment."""
    R = WALK_R
    md = ar.max_dst_of(WALK_LEN, WALK_LEN, R)
    assert ar.nb1(md) == 2 and can_fail_first(WALK_F, R) and ((WALK_F - 1) // 64, ((WALK_F - 1) % 64) >> 5) == (1, 1)
    rng = np.random.RandomState(9970)
    x0, y0 = hug_pair(rng, WALK_LEN, R, WALK_F, WALK_F)
    x1, y1 = hug_pair(rng, WALK_LEN, R, 192)
    texts = [x0, y0, x1, y1]
    res = oracle.align(x0, y0, R)
    assert res["rc"] == -1 and res["fail_row"] == WALK_F
    assert oracle.align(x1, y1, R)["rc"] >= 0 and touches_bound(oracle, x1, y1, WALK_LEN, R, 64)
    file = b"".join(eng.text2bin(t) for t in texts)
    rec_offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in texts[:-1]]).astype(np.uint64)
    mask = eng.mask_from_pattern(MASK_PAT)
    want, pairs = [], 0
    for t in range(len(texts)):
        rows = oracle.spaced_round(texts[t], mask, R, file, rec_offs, 1, 64, buggy=False, nthreads=4)
        pairs += int(rows["n_pairs"].sum()) - int(rows["n_pairs"][t])
        for q in range(len(texts)):
            if q != t and rows["found"][q]:
                want.append((t, q, int(rows["j"][q]), int(rows["dir"][q]), int(rows["ref_pos"][q]), int(rows["cost"][q]),
                             int(rows["matlen_a"][q]), int(rows["matlen_b"][q])))
    assert {(r[0], r[1]) for r in want} == {(2, 3), (3, 2)} and pairs >= 4      # the failing pair was tried both ways, and found by neither
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    got, st = ctx.overlap_all(S, mask, R, 1, 64, kernel=PBA_KERNEL_BITVEC)
    assert [tuple(int(v) for v in r) for r in got] == want
    assert st["wide_first"] == 0 and st["n_redo"] == 0 and st["n_pairs"] == pairs
