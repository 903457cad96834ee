"""Layout of reads into contigs from overlap rows on the device (pba_layout_*): the per-read table, the contig
info, the counters and the stitched set must be IDENTICAL to tests/layout_ref.py, the semantics restated sequentially
(tests/test_layout_cpu.py pins that reference by hand and on a tiling with a known answer).  Needs a real MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

from conftest import MASK_PAT
from layout_ref import ACGT, COUNTERS, HAND_CASES, ROW_FIELDS, combine, hand_texts, layout_ref, make_rows, rc, tiling
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PbaError

pytestmark = pytest.mark.gpu


def exported(ctx, S):
    """The packed arena of a set (pba_seqs_export) and its offsets, on the host.  torch clears the buffer on ITS stream and
    the export copies on the ctx's own non-blocking stream: the clear must have finished before the copy is enqueued, or it
    can land on top of the copied bytes."""
    import torch
    buf = torch.zeros(max(S.packed_bytes, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs = S.export(buf.data_ptr(), buf.numel())
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:S.packed_bytes].tobytes(), offs.tolist()


def same_set(ctx, got, want):
    """tests/test_gpu_strands.py: same_set, with the buffer's clear ordered before the export."""
    assert got.count == want.count and got.max_len == want.max_len
    assert got.lengths().tolist() == want.lengths().tolist()
    for i in range(want.count):
        assert got.get_text(i) == want.get_text(i), i
    assert exported(ctx, got) == exported(ctx, want)          # byte for byte, pad bits and layout included


def check_against_ref(ctx, texts, rows, hang=64, min_reads=2, S=None):
    """Layout on the device == the reference: table, contigs, counters, stitched texts (byte for byte, pad bits included).
    Returns (reference result, device table)."""
    want = layout_ref([len(x) for x in texts], rows, hang, min_reads, texts)
    S = S if S is not None else ctx.seqs_from_list(texts, strict_acgt=True)
    lay = ctx.layout(S, rows, hang, min_reads)
    table = lay.rows()
    assert [tuple(int(r[f]) for f in ROW_FIELDS) for r in table] == want["table"]
    assert [tuple(int(v) for v in c) for c in lay.contigs()] == want["contigs"]
    st = lay.stats
    assert {k: int(st[k]) for k in COUNTERS} == want["stats"]
    got = lay.stitch(S)
    same_set(ctx, got, ctx.seqs_from_list(want["texts"]))
    assert lay.stats["stitch_ms"] > 0 or not want["texts"]
    lay.close()
    return want, table


@pytest.mark.parametrize("case", HAND_CASES, ids=[c["name"] for c in HAND_CASES])
def test_hand_rows(ctx, case):
    """Rows written by hand (tests/layout_ref.py: HAND_CASES, with the arithmetic next to each); no overlapper runs."""
    want, _ = check_against_ref(ctx, hand_texts(case), make_rows(case["rows"]), case["hang"], case["min_reads"])
    assert want["table"] == case["table"] and want["contigs"] == case["contigs"] and want["stats"] == case["stats"]


CHAIN_READS = (1, 2, 3, 4, 5, 63, 64, 65, 1000)


def test_chain_lengths_at_the_jump_round_edges(ctx):
    """One layout with chains of 1 .. 1 000 reads (2^k - 1, 2^k, 2^k + 1 among them): exact tiling rows, random strands,
    shuffled ids and rows.  1 203 reads = 2 406 states: 12 rounds of pointer jumping."""
    rng = np.random.default_rng(301)
    tilings = [tiling(rng, [60] * n, rng.integers(20, 41, n - 1)) for n in CHAIN_READS]
    texts, rows, ids = combine(rng, tilings)
    want, table = check_against_ref(ctx, texts, rows)
    assert sorted(c[1] for c in want["contigs"]) == list(CHAIN_READS[1:]) and want["stats"]["n_unplaced"] == 1
    for (genome, _, _, _, _), new, contig in zip(tilings[1:], ids[1:], sorted(want["contigs"], key=lambda c: c[1])):
        text = want["texts"][want["contigs"].index(contig)]
        assert text in (genome, rc(genome)) and contig[0] == min(int(new[0]), int(new[-1]))


def test_rings_of_many_sizes(ctx):
    """Rings of 2 .. 257 reads next to a path, ids shuffled: every ring is cut at side 0 of its smallest read and only there."""
    rng = np.random.default_rng(304)
    sizes = (2, 3, 7, 63, 64, 65, 257)
    perm = [int(x) for x in rng.permutation(sum(sizes) + 10)]
    tup, at = [], 0
    for k in sizes:
        ring = perm[at:at + k]
        tup += [(ring[i], ring[(i + 1) % k], 1, 0, 40, 100, 0, 60) for i in range(k)]
        at += k
    path = perm[at:]
    tup += [(path[i], path[i + 1], 1, 0, 40, 100, 0, 60) for i in range(9)]
    texts = [rng.choice(ACGT, 100).tobytes() for _ in perm]
    want, _ = check_against_ref(ctx, texts, make_rows([tup[int(k)] for k in rng.permutation(len(tup))]))
    assert want["stats"]["n_cycles"] == len(sizes) and sorted(c[1] for c in want["contigs"]) == sorted(sizes + (10,))


def test_empty_set_and_empty_rows(ctx):
    none = make_rows([])
    want, table = check_against_ref(ctx, [], none, min_reads=1)
    assert table.size == 0 and want["contigs"] == []
    texts = [b"ACGTACGTAC", b"", b"TTG"]
    want, _ = check_against_ref(ctx, texts, none, min_reads=1)      # every read its own contig, the empty one included
    assert want["contigs"] == [(0, 1, 10), (1, 1, 0), (2, 1, 3)]
    want, _ = check_against_ref(ctx, texts, none, min_reads=2)
    assert want["contigs"] == [] and want["stats"]["n_unplaced"] == 3


STITCH_ADV = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33)


def test_packing_edges_in_stitch(ctx):
    """Reads that supply 1 .. 33 bases in both orientations, a contig of one read, a contig of 70 001 bases.
    (adv == 0 cannot come out of valid rows: the row that joins a read to its predecessor is a dovetail, which leaves the
    read a strictly positive overhang beyond the predecessor -- that overhang is adv; DESIGN §5.6.  A slot that supplies
    nothing does reach k_lay_stitch, though: the empty read that is its own contig in test_empty_set_and_empty_rows.)"""
    rng = np.random.default_rng(302)
    n = 2 * len(STITCH_ADV) + 1
    small = tiling(rng, [40] * n, STITCH_ADV + STITCH_ADV, flips=[0] * (len(STITCH_ADV) + 1) + [1] * len(STITCH_ADV))
    big = tiling(rng, [1000] * 100, [700] * 98 + [401])
    one = tiling(rng, [37], [])
    texts, rows, ids = combine(rng, [small, big, one])
    want, table = check_against_ref(ctx, texts, rows, min_reads=1)
    assert sorted(c[2] for c in want["contigs"]) == [37, 40 + 2 * sum(STITCH_ADV), 70001]
    placed = table[np.isin(table["read"], ids[0])]
    seen = {(int(r["adv"]), int(r["orient"])) for r in placed if r["rank"] > 0}
    assert seen == {(a, o) for a in STITCH_ADV for o in (0, 1)}


def test_fuzz_random_rows(ctx):
    """2 000 reads of 50-300 bases, 20 000 random valid rows: an arbitrary graph that has nothing to do with real overlaps.
    Any disagreement between the atomics or the pointer jumping and the sequential reference shows here."""
    rng = np.random.default_rng(303)
    lens = rng.integers(50, 301, 2000)
    texts = [rng.choice(ACGT, int(n)).tobytes() for n in lens]
    tup = []
    for _ in range(20000):
        t = int(rng.integers(0, 2000))
        q = int((t + rng.integers(1, 2000)) % 2000)
        tb, te = sorted(rng.choice(int(lens[t]) + 1, 2, replace=False))
        qb, qe = sorted(rng.choice(int(lens[q]) + 1, 2, replace=False))
        tup.append((t, q, int(rng.choice((1, -1))), int(rng.integers(0, 40)), int(tb), int(te), int(qb), int(qe)))
    want, _ = check_against_ref(ctx, texts, make_rows(tup))
    st = want["stats"]
    assert st["n_contain"] > 100 and st["n_contain_refused"] > 100 and st["n_dovetail"] > st["n_dovetail_dropped"] > 100
    assert st["n_contigs"] > 20 and max(c[1] for c in want["contigs"]) >= 3
    for min_reads in (1, 3):
        check_against_ref(ctx, texts, make_rows(tup), hang=20, min_reads=min_reads)


def test_engine_rows(ctx):
    """Rows of the engine's own overlapper on error-free reads of both strands (the shape of
    test_overlap_strands_vs_oracle_composition: 64 reads of 1 300 bases, 9 000-base genome).  Besides equality with the
    reference: no row is internal, and every contig is a substring of the genome or of its reverse complement.
    Seeds 71 / 72 / 73: tests/test_layout_cpu.py::test_reference_on_oracle_rows runs the reference alone on the same rows,
    composed from the CPU oracle, and meets the same conditions: 1 250 rows, none internal, one read contained, one contig of
    63 reads and 8 085 bases."""
    g = eng.synth_genome(71, 9000)
    reads, offs, _ = eng.synth_reads(72, g, 64, 1300, 0.0, 0.0, 0.0)
    texts = [reads[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(64)]
    flip = np.random.default_rng(73).permutation(64) < 32
    texts = [rc(x) if f else x for x, f in zip(texts, flip)]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    rows, _ = ctx.overlap_strands(S, eng.mask_from_pattern(MASK_PAT), 0.30, 32, 64)
    want, _ = check_against_ref(ctx, texts, rows, hang=64, S=S)
    assert want["stats"]["n_internal"] == 0 and len(rows) > 100
    genome = g.tobytes()
    assert want["texts"] and all(t in genome or t in rc(genome) for t in want["texts"])
    assert max(c[1] for c in want["contigs"]) >= 3
    contigs, lay, rows2, _ = ctx.layout_reads(S, eng.mask_from_pattern(MASK_PAT), 0.30, targets_per_call=17)
    assert np.array_equal(rows2, rows)
    same_set(ctx, contigs, ctx.seqs_from_list(want["texts"]))


def test_refusals(ctx):
    """Every refusal gives its status, and a valid call on the same ctx succeeds afterwards.  Of the PBA_E_TOOLONG limits
    only the read length is produced here (one read of 65 536 bases); 2^32 rows, 2^28 reads and a contig of 0x7FFFFFF0
    bases would take gigabytes of input and are NOT tested."""
    case = HAND_CASES[0]
    texts = hand_texts(case)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    good = case["rows"][0]

    def status(rows, hang=64, min_reads=2):
        with pytest.raises(PbaError) as e:
            ctx.layout(S, make_rows(rows), hang, min_reads)
        return e.value.status

    bad_rows = {
        "target == query": (0, 0, 1, 0, 40, 100, 0, 60), "target outside": (2, 1, 1, 0, 40, 100, 0, 60),
        "query negative": (0, -1, 1, 0, 40, 100, 0, 60), "t interval beyond its read": (0, 1, 1, 0, 40, 101, 0, 60),
        "q interval negative": (0, 1, 1, 0, 40, 100, -1, 60), "t interval empty": (0, 1, 1, 0, 40, 40, 0, 60),
        "q interval reversed": (0, 1, 1, 0, 40, 100, 60, 0), "strand 0": (0, 1, 0, 0, 40, 100, 0, 60), "strand 2": (0, 1, 2, 0, 40, 100, 0, 60),
    }
    for what, row in bad_rows.items():
        assert status([good, row]) == -1, what
        check_against_ref(ctx, texts, make_rows([good]), S=S)
    assert status([good], hang=-1) == -1 and status([good], min_reads=0) == -1
    long_texts = [np.random.default_rng(305).choice(ACGT, 65536).tobytes(), texts[1]]
    with pytest.raises(PbaError) as e:
        ctx.layout(ctx.seqs_from_list(long_texts, strict_acgt=True), make_rows([good]))
    assert e.value.status == -4                                                          # PBA_E_TOOLONG: 16 bits of length in a key
    check_against_ref(ctx, texts, make_rows([good]), S=S)
    check_against_ref(ctx, [long_texts[0][:65535], texts[1]], make_rows([(0, 1, 1, 0, 65475, 65535, 0, 60)]))   # the longest read taken
    lay = ctx.layout(S, make_rows([good]))
    for other in ([texts[0]], [texts[0], texts[1][:-1]], texts + [b"ACGT"]):             # another count, other lengths
        with pytest.raises(PbaError) as e:
            lay.stitch(ctx.seqs_from_list(other, strict_acgt=True))
        assert e.value.status == -1
    out = np.zeros(2, eng.LAYOUT_ROW_DTYPE)
    assert ctx.lib.pba_layout_rows(ctx.h, lay.h, C.c_void_p(out.ctypes.data), 1) == -1        # room for one row of two
    with pytest.raises(PbaError) as e:
        lay.stitch(ctx.seqs_from_list([texts[0], texts[1][:50] + b"N" + texts[1][51:]]))
    assert e.value.status == -6                                                          # PBA_E_ALPHABET
    same_set(ctx, lay.stitch(S), ctx.seqs_from_list([texts[0] + texts[1][60:]]))
    lay.close()
    check_against_ref(ctx, texts, make_rows([good]), S=S)
