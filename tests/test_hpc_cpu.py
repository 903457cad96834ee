"""tests/hpc_ref.py -- homopolymer compression and the lifting of rows in plain numpy, the expectation
pba_hpc_* is held to on the device (tests/test_gpu_hpc.py) -- pinned without a GPU: on cases written out by hand, on the two
facts the row rules rest on, and on the planted read set whose rows come from the CPU oracle the way the engine's overlapper
composes them.  The condition the GPU end-to-end test relies on is proven here, for the same input, before any device is
involved."""
import numpy as np

from conftest import MASK_PAT
from correct_helpers import ACGT, intervals, oracle_rows, rc
from hpc_ref import (EDGE_LENS, HAND_HPC, HAND_TEXTS, PLANTED, SHAPES, TILE, as_tuples, biased_set, consecutive_pairs_at_cost_0,
                     edge_set, hand_rows, hpc, lift_map_rows, lift_overlaps, n_chunks, planted_reads, random_map_rows,
                     random_overlap_rows, redraw_runs, touching_set)
from pacbioassembly_amd import engine as eng


def test_written_out_cases():
    assert hpc(b"") == (b"", [0])
    assert hpc(b"A") == (b"A", [0, 1])
    assert hpc(b"AAAA") == (b"A", [0, 4])
    assert hpc(b"ACGT") == (b"ACGT", [0, 1, 2, 3, 4])
    assert hpc(b"AACCCGT") == (b"ACGT", [0, 2, 5, 6, 7])
    assert [hpc(x) for x in HAND_TEXTS] == HAND_HPC


def test_rc_and_hpc_commute_and_slices_compress_to_slices():
    rng = np.random.default_rng(510)
    for x in biased_set(511, 40) + [rng.choice(ACGT, int(n)).tobytes() for n in rng.integers(0, 300, 40)]:
        c, S = hpc(x)
        assert hpc(rc(x))[0] == rc(c)
        assert all(a < b for a, b in zip(S, S[1:])) and S[-1] == len(x) and len(S) == len(c) + 1
        for _ in range(8):
            b, e = sorted(int(v) for v in rng.integers(0, len(c) + 1, 2))
            assert hpc(x[S[b]:S[e]])[0] == c[b:e]
        assert hpc(redraw_runs(rng, x))[0] == c


def test_input_builders():
    """The edge sets are what their names say."""
    assert EDGE_LENS[-4:] == [TILE - 1, TILE, TILE + 1, 2 * TILE + 1] and TILE == 256 * 32
    for shape in SHAPES:
        texts = edge_set(shape)
        assert [len(t) for t in texts] == EDGE_LENS
        for t in texts:
            c, S = hpc(t)
            if not t:
                continue
            if shape == "single_run":
                assert len(c) == 1
            elif shape == "alternating":
                assert len(c) == len(t)
            elif shape == "runs_of_32":
                assert all(s % 32 == 0 for s in S[:-1])
            elif shape == "runs_past_word":
                assert all(s % 32 == 1 for s in S[1:-1])
    T = touching_set()
    live = [t for t in T if t]
    assert all(a[-1] == b[0] for a, b in zip(live, live[1:])) and T.count(b"") >= 5
    assert any(a[-1:] == b"A" for a in live[:-1]) and any(a[-1:] != b"A" for a in live[:-1])
    B = biased_set()
    assert len(B) == 200 and min(len(t) for t in B) >= 2 and sum(len(t) > TILE for t in B) == 3
    lens = [len(t) for t in B]
    assert n_chunks(lens, 0) == 1 and n_chunks(lens, 1) == 200 and n_chunks([], 0) == 0
    assert n_chunks(lens, sum(lens[:50])) >= 2 and n_chunks([5, 0, 0, 7], 5) == 2 and n_chunks([5, 5], 9) == 2


def test_hand_rows_lifted():
    """Every strand x dir combination, the lifted row written out next to its arithmetic (tests/hpc_ref.py: HAND_ROWS); the
    interval identities of include/pba.h recomputed from the lifted j / ref_pos / matlen_*."""
    rows, want = hand_rows()
    S, lens = [s for _, s in HAND_HPC], [len(t) for t in HAND_TEXTS]
    got = lift_overlaps(rows, S, lens)
    assert as_tuples(got) == want
    assert {(int(r["strand"]), int(r["dir"])) for r in got} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    for r in got:
        assert intervals(r, lens[int(r["query"])]) == tuple(int(r[k]) for k in ("t_beg", "t_end", "q_beg", "q_end"))
    # ... and of random rows, whose compressed form satisfies the identities too
    rng = np.random.default_rng(512)
    texts = biased_set(513, 30)
    H = [hpc(t) for t in texts]
    rows = random_overlap_rows(rng, [len(c) for c, _ in H], 300)
    for r in rows:
        assert intervals(r, len(H[int(r["query"])][0])) == tuple(int(r[k]) for k in ("t_beg", "t_end", "q_beg", "q_end"))
    for r in lift_overlaps(rows, [s for _, s in H], [len(t) for t in texts]):
        assert intervals(r, len(texts[int(r["query"])])) == tuple(int(r[k]) for k in ("t_beg", "t_end", "q_beg", "q_end"))
        assert 0 <= r["t_beg"] < r["t_end"] <= len(texts[int(r["target"])]) and 0 <= r["q_beg"] < r["q_end"] <= len(texts[int(r["query"])])


def test_map_rows_lifted():
    """Two maps; found == 0 rows pass through; a found row's intervals as include/pba.h states them for pba_map_row."""
    rng = np.random.default_rng(514)
    reads, contigs = biased_set(515, 20), biased_set(516, 5, 300, 2000)
    Hr, Hc = [hpc(t) for t in reads], [hpc(t) for t in contigs]
    rows = random_map_rows(rng, [len(c) for c, _ in Hr], [len(c) for c, _ in Hc], 60)
    got = lift_map_rows(rows, [s for _, s in Hr], [len(t) for t in reads], [s for _, s in Hc])
    assert sum(int(r["found"]) == 0 for r in rows) == 20
    for a, b in zip(rows, got):
        if not a["found"]:
            assert a == b
            continue
        L = len(reads[int(b["read"])])
        j, ma, mb, pos = (int(b[k]) for k in ("j", "matlen_a", "matlen_b", "pos"))
        walked = (j, j + ma) if b["strand"] > 0 else (L - j - ma, L - j)
        assert walked == (int(b["r_beg"]), int(b["r_end"])) and (pos, pos + mb) == (int(b["c_beg"]), int(b["c_end"]))
        assert int(b["seglen"]) == L - j
        assert all(a[k] == b[k] for k in ("read", "nseq", "found", "strand", "contig", "cost", "n_pairs", "diag_cost"))
    # one row by hand: read 1 of HAND_TEXTS on contig 0; r [2, 6) -> [5, 11), c [1, 4) -> [3, 10); strand -1: j = 11 - 11 = 0
    one = np.zeros(1, eng.MAP_ROW_DTYPE)
    one[0]["read"], one[0]["found"], one[0]["strand"], one[0]["contig"] = 1, 1, -1, 0
    one[0]["r_beg"], one[0]["r_end"], one[0]["c_beg"], one[0]["c_end"] = 2, 6, 1, 4
    o = lift_map_rows(one, [s for _, s in HAND_HPC], [14, 11], [s for _, s in HAND_HPC])[0]
    assert tuple(int(o[k]) for k in ("r_beg", "r_end", "c_beg", "c_end", "pos", "matlen_a", "matlen_b", "j", "seglen")) == (5, 11, 3, 10, 3, 6, 7, 0, 11)


def test_planted_reads_overlap_at_cost_0_when_compressed(lib, oracle):
    """The planted input of tests/test_gpu_hpc.py::test_through_the_overlapper: the reads differ from the genome only in their
    run lengths, so their compressed texts agree wherever they overlap, and the CPU oracle -- composed the way the engine's
    overlapper composes its rows -- gives every consecutive pair of reads a row at cost 0 in at least one role."""
    P = PLANTED
    texts, clean = planted_reads()
    assert len(texts) == P["n"] == 12 and all(len(x) == P["rl"] for x in clean)
    for k, (t, x) in enumerate(zip(texts, clean)):
        assert hpc(rc(t) if k & 1 else t)[0] == hpc(x)[0] and t != x
    comp = [hpc(t)[0] for t in texts]
    rows = oracle_rows(oracle, comp, eng.mask_from_pattern(MASK_PAT), P["R"], overlap_min=P["overlap_min"], nthreads=16)
    have = consecutive_pairs_at_cost_0(rows, P["n"])
    print(len(rows), "rows on the compressed reads; consecutive pairs at cost 0:", have)
    assert have == list(range(P["n"] - 1))
    S, lens = [hpc(t)[1] for t in texts], [len(t) for t in texts]
    for r in lift_overlaps(rows, S, lens):
        assert intervals(r, lens[int(r["query"])]) == tuple(int(r[k]) for k in ("t_beg", "t_end", "q_beg", "q_end"))
