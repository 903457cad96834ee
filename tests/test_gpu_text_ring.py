"""The text ring of the score-only bit-vector sweep (align_bitvec.h: bitvec_pass<.., RING>, csrc/text_ring.h): the text's
mask pairs come from a 128-element ring in the wavefront's LDS, written 32 elements per chunk and read at a per-lane
address that runs one element per step.  What can go wrong is a text shifted against the pattern, a stale element after a
wrap, a lane that looks 64 elements back into a slot already rewritten, or a ring left by the previous sweep.  So: true
pairs that are substitutions only, at a density near R (a shift by one column turns them into strangers), with m around the
chunk (32), the lanes (64), the ring's capacity C = 128 and 2 C + 1, origins pos % 32 in {0, 1, 31} in both directions, on the
first and last sequence of the set, n - m around max_dst; pairs whose first failing row is the row of a wrap and the rows
next to it; pairs long enough for a lane to take its second superblock in the middle of a chunk (rows past 2 048 in ring 1,
past 4 096 in ring 2 behind a pilot); a batch of long and short pairs mixed through every wavefront.  Through k_align_pairs,
k_locate (one probe per read: the band-cell counter is a function of each alignment) and the spaced round.  Every input is
proved by the oracle in the test that runs it; csrc/text_ring.h itself is played against a model in test_text_ring_cpu.py.
Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import align_rings as ar
import test_gpu_align_rings as rings
from conftest import MASK_PAT
from diag_collect_inputs import BEHIND, ROW, can_fail_first, greedy_groups, groups_of, hug_pair
from event_schedule_inputs import fail_at
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PAIR_DTYPE, PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL, PBA_KERNEL_BITVEC
from test_gpu_parity import check_result

pytestmark = pytest.mark.gpu

C = 128                                                       # PBA_TXR_COLS (test_text_ring_cpu.py holds the header to it)
EDGE_MS = (31, 32, 33, 63, 64, 65, C - 1, C, C + 1, 2 * C + 1)
RS = {NB: groups_of(NB)[0][0] for NB in (1, 2)}              # the R of the diag-collect tests' first group of each ring
WRAP_ROWS = (C - 1, C, C + 1, C + 2, 2 * C, 2 * C + 1)       # element C goes over element 0: column C + 1 is the first from a rewritten slot


def forced(NB, B, R):
    return B if NB == 1 else B.with_pilot(ar.pilot(ar.row_of(*ROW[NB])[0], R))


def edge_batch(NB) -> ar.Batch:
    """true pairs of every m of EDGE_MS: a substitutions-only copy on the bound (hug_pair), the longer side m + delta for
    delta in {0, 1, max_dst - 1, max_dst, max_dst + 40}; directions and origins drawn so that all occur; the first pair on
    sequence 0, the last on the last sequence"""
    R = RS[NB]
    rng = np.random.RandomState(8800 + NB)
    B = ar.Batch()
    k = 0
    for m in EDGE_MS:
        md = ar.max_dst_of(m, m + 1, R)
        for delta in sorted({0, 1, md - 1, md, md + 40}):
            x, y = hug_pair(rng, m, R, m)
            y = y + ar.rand_seq(rng, delta)
            a, b = (y, x) if k % 2 else (x, y)
            fa, fb = bool(k & 2), bool(k & 4)
            ma, mb = ar.MODS[k % 3], ar.MODS[(k // 3) % 3]
            B.add_pair(B.place(rng, a[::-1] if fa else a, fa, ma), B.place(rng, b[::-1] if fb else b, fb, mb), fa, fb,
                       kind="true", m=m, delta=delta, aback=fa, bback=fb, amod=ma, bmod=mb, tag=f"ring{NB}:m{m}+{delta}")
            k += 1
    return B


def prove_true(oracle, B, R):
    """every true pair passes the diagonal's checks with exactly its planted substitutions at (m, m); the reference accepts
    it unless the longer side is b and its random tail is too long for seq_aligner.h:114 (short m, delta >= max_dst), which
    is the reference's answer too -- at least three deltas of every m are accepted"""
    ok = {}
    for q, (meta, x) in enumerate(zip(B.meta, ar.expected(oracle, B, R))):
        if meta["kind"] == "true":
            a, b = B.elems(q)
            n = min(len(a), len(b))
            assert x["fail_row"] == 0 and n == min(x["len_a"], x["len_b"]) == meta["m"], (meta, x)
            oracle.align(a, b, R)
            assert oracle.cell(n, n)[0] == sum(p != q_ for p, q_ in zip(a[:n], b[:n])) > 0, meta
            assert x["rc"] >= 0 or (x["len_b"] > x["len_a"] and x["matlen_b"] < x["len_b"] * (1.0 - R)), (meta, x)
            ok[meta["m"]] = ok.get(meta["m"], 0) + (x["rc"] >= 0)
    assert ok and min(ok.values()) >= 3, ok


@pytest.mark.parametrize("NB", [1, 2])
def test_true_pairs_at_the_ring_edges(ctx, oracle, NB):
    R = RS[NB]
    B = edge_batch(NB)
    metas = B.meta
    assert {(m["aback"], m["bback"]) for m in metas} == {(False, False), (True, False), (False, True), (True, True)}
    assert {m["amod"] for m in metas} == {m["bmod"] for m in metas} == set(ar.MODS)
    assert B.pairs[0][0] == 0 and max(B.pairs[-1][0], B.pairs[-1][3]) == len(B.seqs) - 1
    F = forced(NB, B, R)
    prove_true(oracle, F, R)
    prof = rings.check_batch(ctx, oracle, F, R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == NB and prof["n_first"] == len(F.pairs)


def wrap_batches(NB):
    """[(R, batch)]: pairs failing first at each row of WRAP_ROWS, as the pair's last row and with clean rows behind, plain
    (no base in common behind the failure) and on the bound up to it"""
    out = []
    for g, (R, rows) in enumerate(greedy_groups([f for f in WRAP_ROWS])):
        rng = np.random.RandomState(8820 + 10 * g + NB)
        B = ar.Batch()
        for k, f in enumerate(rows):
            assert can_fail_first(f, R)
            for last in (True, False):
                m = f if last else f + BEHIND
                x, y = hug_pair(rng, m, R, f, f) if (k + last) % 2 else fail_at(rng, f, m, R)
                a, b = (y, x) if k % 2 else (x, y)
                B.add_pair(B.place(rng, a, False, ar.MODS[k % 3]), B.place(rng, b, False, ar.MODS[(k + 1) % 3]), False, False,
                           kind="fail", f=f, m=m, tag=f"wrap{NB}:fail{f}:m{m}")
        out.append((R, B))
    return out


@pytest.mark.parametrize("NB", [1, 2])
def test_first_failing_row_at_a_wrap(ctx, oracle, NB):
    seen = set()
    for R, B in wrap_batches(NB):
        F = forced(NB, B, R)
        for meta, x in zip(F.meta, ar.expected(oracle, F, R)):
            if meta["kind"] == "fail":
                assert x["rc"] == -1 and x["fail_row"] == meta["f"] and min(x["len_a"], x["len_b"]) == meta["m"], (meta, x)
                seen.add((meta["f"], meta["m"] == meta["f"]))
        prof = rings.check_batch(ctx, oracle, F, R, PBA_KERNEL_BITVEC)
        assert prof["nb_first"] == NB and prof["n_redo"] == 0
    assert seen == {(f, last) for f in WRAP_ROWS for last in (True, False)}


LONG = {1: 2100, 2: 4200}


@pytest.mark.parametrize("NB", [1, 2])
def test_second_superblock_in_the_middle_of_a_chunk(ctx, oracle, NB):
    """rows past 64 superblocks: lane 0 closes superblock 0 and looks 64 elements back while the chunk's 32 new ones are
    already written.  One pair on the bound (substitutions only), one with indels, the longer side as a and as b."""
    R, m = 0.30, LONG[NB]
    md = ar.max_dst_of(m, m + 1, R)
    assert m + min(md, ar.bv_pass1_w(md, NB)) > 64 * 32 * NB and (NB == 1 or ar.nb1(md) == 1)
    rng = np.random.RandomState(8840 + NB)
    B = ar.Batch()
    for k in range(3):
        if k == 0:
            x, y = hug_pair(rng, m, 0.12, m)
        else:
            x = ar.rand_seq(rng, m)
            y = ar.fit(rng, ar.mutate(rng, x, 0.10), m)
        y = y + ar.rand_seq(rng, md + 30)
        a, b = (y, x) if k == 2 else (x, y)
        B.add_pair(B.place(rng, a, False, ar.MODS[k]), B.place(rng, b, False, ar.MODS[(k + 1) % 3]), False, False,
                   kind="long", m=m, tag=f"long{NB}:{k}")
    F = forced(NB, B, R)
    for meta, x in zip(F.meta, ar.expected(oracle, F, R)):
        assert meta["kind"] == "pilot" or (x["rc"] >= 0 and min(x["len_a"], x["len_b"]) == m), (meta, x)
    prof = rings.check_batch(ctx, oracle, F, R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == NB


def test_long_and_short_pairs_through_every_wavefront(ctx, oracle):
    """32 distinct pairs, long (300 .. 420) and short (31 .. 65) in turn, true and failing, 640 times each: more pairs than
    the chip has wavefronts, so every wavefront sweeps several, a short one behind a long one's ring and the other way."""
    R = RS[1]
    rng = np.random.RandomState(8860)
    B = ar.Batch()
    fails = [f for f in range(40, 64) if can_fail_first(f, R)]
    for k in range(32):
        m = (300 + 4 * k) if k % 2 == 0 else (31, 32, 33, 63, 64, 65)[(k // 2) % 6]
        if k % 8 < 6:
            x, y = hug_pair(rng, m, R, m)
            kind = "true"
        else:
            f = fails[k % len(fails)] if m >= 63 or m > 100 else 0
            x, y = (hug_pair(rng, m, R, f, f) if f else (ar.rand_seq(rng, m), ar.rand_seq(rng, m)))
            kind = "fail"
        B.add_pair(B.place(rng, x, False, ar.MODS[k % 3]), B.place(rng, y + ar.rand_seq(rng, 7 * (k % 4)), False, ar.MODS[(k + 1) % 3]),
                   False, False, kind=kind, m=m, tag=f"mix:{k}:m{m}:{kind}")
    want = ar.expected(oracle, B, R)
    for meta, x in zip(B.meta, want):
        assert (x["rc"] >= 0) == (meta["kind"] == "true"), (meta, x)
    reps = 640
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs * reps, PAIR_DTYPE)
    assert pairs.size > 2 * 256 * 32
    out = ctx.align_batch(S, S, pairs, R, kernel=PBA_KERNEL_BITVEC)
    assert ctx.last_profile()["nb_first"] == 1
    for q in range(len(B.pairs)):
        check_result(out[q], want[q], B.meta[q]["tag"])
    first = out[:len(B.pairs)]
    for r in range(1, reps):
        assert (out[r * len(B.pairs):(r + 1) * len(B.pairs)] == first).all(), r


# ----------------------------------------------------------------------------- the drivers
def driver_case(NB):
    """A reference that holds, between spacers, the longer side of true pairs of the edge lengths and of pairs failing at the
    wrap rows, and the shorter sides as reads; ring 2 behind an unrelated filler read that sizes the plan."""
    R = RS[NB]
    rng = np.random.RandomState(8880 + NB)
    parts, reads, meta = [ar.rand_seq(rng, 200)], [], []

    def plant(x, y, **m):
        pos = sum(len(p) for p in parts)
        parts.extend([y, ar.rand_seq(rng, 150)])
        reads.append(x)
        meta.append(dict(pos=pos, **m))

    for m in EDGE_MS[3:] + (LONG[1],):
        x, y = hug_pair(rng, m, R, m)
        plant(x, y + ar.rand_seq(rng, ar.max_dst_of(m, m + 1, R)), kind="true", m=m)
    for f in [f for f in WRAP_ROWS if can_fail_first(f, R)]:
        x, y = hug_pair(rng, f + BEHIND, R, f, f)
        plant(x, y + ar.rand_seq(rng, 80), kind="fail", f=f, m=f + BEHIND)
    if NB == 2:
        reads.append(ar.pilot(ar.row_of(2, 2)[0], R, seed=3)[0])
        meta.append(dict(kind="filler"))
    return np.frombuffer(b"".join(parts), np.uint8), reads, meta


@pytest.mark.parametrize("NB", [1, 2])
def test_locate_through_the_ring(ctx, oracle, NB):
    """k_locate<NB>, one probe per read: rows, pair counts and the band cells against the oracle."""
    R = RS[NB]
    g, texts, meta = driver_case(NB)
    gb = g.tobytes()
    n_true = n_fail = 0
    for t, mt in zip(texts, meta):
        if mt["kind"] == "filler":
            continue
        assert gb.count(t[:16]) == 1 and gb.find(t[:16]) == mt["pos"]
        x = oracle.align(t, gb[mt["pos"]:mt["pos"] + 2 * len(t) + 8], R)
        if mt["kind"] == "fail":
            assert x["rc"] == -1 and x["fail_row"] == mt["f"], (mt, x)
            n_fail += 1
        else:
            assert x["rc"] >= 0 and x["len_a"] == mt["m"], (mt, x)
            n_true += 1
    assert n_true == len(EDGE_MS) - 2 and n_fail >= 2
    reads = np.frombuffer(b"".join(texts), np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
    mask = eng.mask_from_pattern(MASK_PAT)
    T = ctx.seqs_from_list([gb], strict_acgt=True)
    Rd = ctx.seqs_from_text(reads, offs, strict_acgt=True)
    ix = ctx.index_build(T, 0, mask, PBA_INDEX_ALL)
    rows, st = ctx.locate(ix, T, 0, Rd, R, 1, 33, kernel=PBA_KERNEL_BITVEC)
    assert ctx.last_profile()["nb_first"] == NB
    want, wst = oracle.locator(g, mask, R, reads, offs, 1, 33, nthreads=8)
    for c in ("nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs"):
        assert (rows[c] == want[c]).all(), c
    assert st == wst and "n_cells" in st and wst["n_located"] == n_true, (st, wst)


@pytest.mark.parametrize("NB", [1, 2])
def test_spaced_round_through_the_ring(ctx, oracle, NB):
    """k_spaced_round<NB> over the same reads as records, in both seed placements."""
    R = RS[NB]
    g, texts, meta = driver_case(NB)
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
