"""Homopolymer-compressed sequence sets and rows lifted back on the device (pba_hpc_*): the compressed set, the
run starts, the counters and every lifted row must be IDENTICAL to tests/hpc_ref.py, the rule restated in plain numpy
(tests/test_hpc_cpu.py pins that reference by hand and proves the planted input's condition).  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

from clip_ref import ROW_FIELDS as CLIP_FIELDS, clip_ref
from conftest import MASK_PAT
from correct_helpers import rc
from hpc_ref import (EDGE_LENS, HAND_HPC, HAND_TEXTS, PLANTED, SHAPES, TILE, as_tuples, biased_set, consecutive_pairs_at_cost_0, edge_set,
                     hand_rows, hpc, lift_map_rows, lift_overlaps, n_chunks, overlap_rows, planted_reads, random_map_rows,
                     random_overlap_rows, touching_set)
from layout_ref import COUNTERS as LAYOUT_COUNTERS, ROW_FIELDS as LAYOUT_FIELDS, layout_ref
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PbaError
from test_gpu_clip import same_set

pytestmark = pytest.mark.gpu


def check_against_ref(ctx, texts, S=None, max_bases=0, every=1):
    """seqs_hpc on the device == the reference: the compressed set byte for byte, the run starts of every `every`-th sequence,
    the lengths and the counters.  Returns (the Hpc, the reference's (compressed, S) per sequence)."""
    want = [hpc(t) for t in texts]
    S = S if S is not None else ctx.seqs_from_list(texts, strict_acgt=True)
    comp, m = ctx.seqs_hpc(S, max_bases)
    ctexts = [c for c, _ in want]
    same_set(ctx, comp, ctx.seqs_from_list(ctexts), ctexts)
    for i in range(0, len(texts), every):
        assert m.run_starts(i).tolist() == want[i][1], i
    lin, lout = m.lengths()
    assert lin.tolist() == [len(t) for t in texts] and lout.tolist() == [len(c) for c in ctexts]
    st = m.stats
    assert (st["n_seqs"], st["n_bases_in"], st["n_bases_out"]) == (len(texts), sum(map(len, texts)), sum(map(len, ctexts)))
    assert st["max_len_in"] == max(map(len, texts), default=0) and st["max_len_out"] == max(map(len, ctexts), default=0)
    assert st["n_chunks"] == n_chunks([len(t) for t in texts], max_bases)
    comp.close()
    return m, want


@pytest.mark.parametrize("shape", SHAPES)
def test_compress_edges(ctx, shape):
    """Lengths 0 .. 2 TILE + 1 around every word, wavefront and tile edge of k_hpc_heads / k_hpc_emit, in five shapes."""
    texts = edge_set(shape)
    assert [len(t) for t in texts] == EDGE_LENS and EDGE_LENS[-1] == 2 * TILE + 1
    m, _ = check_against_ref(ctx, texts)
    m.close()


def test_long_single_runs(ctx):
    """70 001 bases of A (every plane word zero, as the pad bits are) and of T: H == 1, the carry crosses nine tiles."""
    m, want = check_against_ref(ctx, [b"A" * 70001, b"T" * 70001])
    assert [w[0] for w in want] == [b"A", b"T"] and m.run_starts(1).tolist() == [0, 70001]
    m.close()


def test_touching_and_empty_sequences(ctx):
    """Neighbours that end and start with the same base, empty sequences between them; only empty sequences; no sequence."""
    m, want = check_against_ref(ctx, touching_set())
    assert all(len(c) >= 1 for c, _ in want if c) and sum(not c for c, _ in want) >= 5
    m.close()
    m, _ = check_against_ref(ctx, [b"", b"", b""])
    assert m.run_starts(1).tolist() == [0]
    m.close()
    m, _ = check_against_ref(ctx, [])
    assert m.n == 0 and m.lift_overlaps(overlap_rows([], [])).size == 0
    m.close()


def test_records_layout_gives_the_same_set(ctx):
    """The same texts as a binary read file's records (bytes as given: no 16-byte alignment) compress to the same set."""
    texts = [t for s in ("random", "runs_past_word") for t in edge_set(s, 505)] + touching_set() + biased_set(506, 20)
    file = b"".join(eng.text2bin(t) for t in texts)
    R = ctx.seqs_from_records(file, 0, 1 << 30)              # (a record file keeps lengths above min_excl: the empty ones drop out)
    keep = [t for t in texts if t]
    assert R.count == len(keep) and R.packed_bytes == len(file)
    m, _ = check_against_ref(ctx, keep, S=R)
    m.close()


@pytest.fixture(scope="module")
def biased():
    texts = biased_set()
    return texts, [hpc(t) for t in texts]


def test_chunks(ctx, biased):
    """200 sequences with biased run lengths at max_bases 0 (one chunk), 1 (every sequence its own chunk), a value that cuts
    between sequences 49 and 50, and one base less (the cut moves to 48 | 49): identical results, n_chunks as the reference counts."""
    texts, _ = biased
    lens = [len(t) for t in texts]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    first50 = sum(lens[:50])
    for max_bases, chunks in ((0, 1), (1, 200), (first50, None), (first50 - 1, None), (sum(lens), 1), (sum(lens) - 1, 2)):
        m, _ = check_against_ref(ctx, texts, S=S, max_bases=max_bases, every=7)
        assert chunks is None or m.stats["n_chunks"] == chunks, max_bases
        m.close()
    assert n_chunks(lens, first50) >= 3


def lift_and_compare(m, rows, want_S, lens):
    want = lift_overlaps(rows, want_S, lens)
    got = m.lift_overlaps(rows)
    assert np.array_equal(got, want)
    return got


def test_lift_hand_rows(ctx):
    """The hand rows of tests/test_hpc_cpu.py::test_hand_rows_lifted, every strand x dir combination."""
    m, want = check_against_ref(ctx, HAND_TEXTS)
    assert want == HAND_HPC
    rows, lifted = hand_rows()
    got = lift_and_compare(m, rows, [s for _, s in want], [len(t) for t in HAND_TEXTS])
    assert as_tuples(got) == lifted
    m.close()


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_lift_random_rows(ctx, biased, count):
    """Random valid rows, every fourth from index 0 to the sentinel S[H], on a set that also holds reads with H == 1; the C
    entry point with out aliasing rows."""
    texts, want = biased
    texts = texts + [b"C" * 40, b"G", b"A" * 33]
    want = want + [hpc(t) for t in texts[-3:]]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    comp, m = ctx.seqs_hpc(S)
    comp.close()
    hs, lens = [len(c) for c, _ in want], [len(t) for t in texts]
    rng = np.random.default_rng(520 + count)
    rows = random_overlap_rows(rng, hs, count)
    if count >= 63:                                           # reads with H == 1: [0, 1) is index 0 and the sentinel at once
        rows[:3] = overlap_rows([(200, 201, 1, 1, 0, 0, 1, 0, 1), (201, 202, -1, -1, 0, 0, 1, 0, 1), (202, 5, -1, 1, 0, 0, 1, 0, hs[5])], hs)
    ws = [s for _, s in want]
    lift_and_compare(m, rows, ws, lens)
    alias = rows.copy()
    assert ctx.lib.pba_hpc_lift_overlaps(ctx.h, m.h, alias.ctypes.data, alias.size, alias.ctypes.data) == 0
    assert np.array_equal(alias, lift_overlaps(rows, ws, lens))
    m.close()


@pytest.mark.parametrize("count", [0, 1, 64, 257])
def test_lift_map_rows(ctx, biased, count):
    """pba_map_row through two different maps, every third row found == 0 and passed through unchanged."""
    reads, want_r = biased
    contigs = biased_set(521, 6, 500, 4000) + [b"T" * 100]
    want_c = [hpc(t) for t in contigs]
    cr, mr = ctx.seqs_hpc(ctx.seqs_from_list(reads, strict_acgt=True))
    cc, mc = ctx.seqs_hpc(ctx.seqs_from_list(contigs, strict_acgt=True))
    rng = np.random.default_rng(530 + count)
    rows = random_map_rows(rng, [len(c) for c, _ in want_r], [len(c) for c, _ in want_c], count)
    want = lift_map_rows(rows, [s for _, s in want_r], [len(t) for t in reads], [s for _, s in want_c])
    assert np.array_equal(mr.lift_map_rows(rows, mc), want)
    alias = rows.copy()
    assert ctx.lib.pba_hpc_lift_map_rows(ctx.h, mr.h, mc.h, alias.ctypes.data, alias.size, alias.ctypes.data) == 0
    assert np.array_equal(alias, want)
    for x in (cr, cc, mr, mc):
        x.close()


def test_refusals(ctx):
    """Every refusal gives its status, and a valid call on the same ctx succeeds afterwards."""
    with_n = ctx.seqs_from_list([HAND_TEXTS[0], b"ACGTNACGT"])
    with pytest.raises(PbaError) as e:
        ctx.seqs_hpc(with_n)
    assert e.value.status == -6                               # PBA_E_ALPHABET
    m, want = check_against_ref(ctx, HAND_TEXTS)
    hs = [7, 6]
    bad = {
        "target outside": (2, 1, 1, 1, 0, 1, 4, 0, 4), "query negative": (0, -1, 1, 1, 0, 1, 4, 0, 4), "self pair": (0, 0, 1, 1, 0, 1, 4, 0, 4),
        "t interval empty": (0, 1, 1, 1, 0, 4, 4, 0, 4), "q interval reversed": (0, 1, 1, 1, 0, 1, 4, 4, 0),
        "t beyond the compressed length (inside the original one)": (0, 1, 1, 1, 0, 1, 8, 0, 4),
        "q beyond the compressed length": (0, 1, 1, 1, 0, 1, 4, 0, 7), "strand 0": (0, 1, 0, 1, 0, 1, 4, 0, 4), "dir 0": (0, 1, 1, 0, 0, 1, 4, 0, 4),
        "dir 2": (0, 1, 1, 2, 0, 1, 4, 0, 4),
    }
    good = (0, 1, 1, 1, 0, 1, 4, 0, 4)
    for what, row in bad.items():
        rows = overlap_rows([good, (0, 1, 1, 1, 0, 0, 1, 0, 1)], hs)
        for k, f in enumerate(("target", "query", "strand", "dir", "cost", "t_beg", "t_end", "q_beg", "q_end")):
            rows[1][f] = row[k]
        with pytest.raises(PbaError) as e:
            m.lift_overlaps(rows)
        assert e.value.status == -1, what
    one = np.zeros(2, eng.MAP_ROW_DTYPE)
    one[1]["read"], one[1]["found"], one[1]["strand"], one[1]["contig"] = 1, 1, -1, 0
    one[1]["r_beg"], one[1]["r_end"], one[1]["c_beg"], one[1]["c_end"] = 2, 6, 1, 4
    ws, lens = [s for _, s in want], [len(t) for t in HAND_TEXTS]
    assert np.array_equal(m.lift_map_rows(one, m), lift_map_rows(one, ws, lens, ws))
    for f, v in (("contig", 2), ("contig", -1), ("read", 2), ("strand", 0), ("c_end", 8), ("r_end", 7), ("r_beg", 6)):
        row = one.copy()
        row[1][f] = v
        with pytest.raises(PbaError) as e:
            m.lift_map_rows(row, m)
        assert e.value.status == -1, (f, v)
    for seq in (2, 0xFFFFFFFF):
        with pytest.raises(PbaError) as e:
            m.run_starts(seq)
        assert e.value.status == -1
    lift_and_compare(m, overlap_rows([good], hs), ws, lens)    # the ctx and the map still work
    m.close()


def test_through_the_overlapper(ctx):
    """The planted reads of tests/test_hpc_cpu.py (only their run lengths differ from the genome's): overlap_hpc == the lift of
    overlap_strands on the compressed set; every consecutive pair has a cost-0 row; a cost-0 row's lifted intervals compress
    to the same text; clip and layout take the lifted rows in original coordinates and equal their references on them."""
    P = PLANTED
    texts, _ = planted_reads()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    mask = eng.mask_from_pattern(MASK_PAT)
    rows, _, m = ctx.overlap_hpc(S, mask, P["R"], overlap_min=P["overlap_min"])
    want = [hpc(t) for t in texts]
    comp = ctx.seqs_from_list([c for c, _ in want], strict_acgt=True)
    crows, _ = ctx.overlap_strands(comp, mask, P["R"], overlap_min=P["overlap_min"])
    lens = [len(t) for t in texts]
    assert len(crows) > 0 and np.array_equal(rows, lift_overlaps(crows, [s for _, s in want], lens))
    assert consecutive_pairs_at_cost_0(rows, P["n"]) == list(range(P["n"] - 1))
    n0 = 0
    for r in rows:
        if int(r["cost"]) != 0:
            continue
        n0 += 1
        T, Q, lq = texts[int(r["target"])], texts[int(r["query"])], lens[int(r["query"])]
        qb, qe = int(r["q_beg"]), int(r["q_end"])
        walked = Q[qb:qe] if r["strand"] > 0 else rc(Q)[lq - qe:lq - qb]
        assert hpc(T[int(r["t_beg"]):int(r["t_end"])])[0] == hpc(walked)[0]
    assert n0 >= P["n"] - 1
    # downstream, on the ORIGINAL reads
    cw = clip_ref(lens, rows, 20, 1, 0, 3, texts)
    cl = ctx.clip(S, rows, 20, 1)
    assert [tuple(int(x[f]) for f in CLIP_FIELDS) for x in cl.rows()] == cw["table"]
    cl.close()
    lw = layout_ref(lens, rows, 64, 2, texts)
    lay = ctx.layout(S, rows, 64, 2)
    assert [tuple(int(x[f]) for f in LAYOUT_FIELDS) for x in lay.rows()] == lw["table"]
    assert [tuple(int(v) for v in c) for c in lay.contigs()] == lw["contigs"]
    assert {k: int(lay.stats[k]) for k in LAYOUT_COUNTERS} == lw["stats"]
    lay.close()
    m.close()
