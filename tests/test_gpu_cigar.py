"""Run-length alignments from the device: the CigarSink of the traced bit-vector pass (k_cigar_pairs) at the edges of its
64-op groups, under all four flag combinations, in every ring and in the reference-band re-run, and the row-level entry
points for mapped reads and overlap rows, chunked and capped -- every comparison exact, against tests/cigar_ref.py applied to
the CPU oracle's own scripts.  tests/test_cigar_cpu.py proves the planted inputs' shapes.  Needs a real MI355X (-m gpu)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_rings as ar
import cigar_ref as cr
from conftest import MASK_PAT, ROOT
from map_ref import many_contig_case, rc
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import ALN_COUNTS_DTYPE, MAP_ROW_DTYPE, PAIR_DTYPE, PBA_KERNEL_BITVEC, RESULT_DTYPE, PbaError
from test_align_rings_cpu import EDGE_R, excursion_case, must_redo
from test_cigar_cpu import overlap_case
from test_gpu_align_rings import EDGE_ROWS, forced
from test_gpu_parity import check_result

pytestmark = pytest.mark.gpu
FLAGS = (0, cr.REVERSED, cr.B_IS_QUERY, cr.REVERSED | cr.B_IS_QUERY)
CNT = ("n_eq", "n_x", "n_ins", "n_del")


def same_pair(got_runs, got_counts, x, a, b, flags, tag):
    """runs and counts of one pair equal cigar_ref of the oracle's script (nothing at all for a failure)"""
    if x["rc"] < 0:
        assert len(got_runs) == 0 and all(int(got_counts[n]) == 0 for n in CNT), tag
        return
    want, wc = cr.runs(x["ops"], a, b, flags)
    assert got_runs.tolist() == want, (tag, flags, cr.string(got_runs), cr.string(want))
    assert {n: int(got_counts[n]) for n in CNT} == wc, (tag, flags)
    assert cr.identities(wc, x, flags), tag


def check_batch(ctx, oracle, B, R, flags=0):
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    out, runs, counts = ctx.align_batch_cigar(S, S, np.array(B.pairs, PAIR_DTYPE), R, flags=flags)
    prof = ctx.last_profile()
    for q, (got, exp) in enumerate(zip(out, ar.expected(oracle, B, R))):
        check_result(got, exp, B.meta[q]["tag"])
        same_pair(runs[q], counts[q], exp, *B.elems(q), flags, B.meta[q]["tag"])
    return prof


def test_group_edges_of_the_sink(ctx, oracle):
    """planted edits as the 1st .. 129th op from the goal, exact copies over several groups, 1 .. 129 ops in all, two edits
    across a group edge, an X inside a long diagonal, the row-sweep corner, the border loops, failures"""
    B = ar.Batch()
    rng = np.random.RandomState(1)
    for tag, a, b, _ in cr.planted_pairs():
        B.add_pair(B.place(rng, a, False, 0), B.place(rng, b, False, 1), False, False, tag=tag)
    prof = check_batch(ctx, oracle, B, cr.PLANT_R)
    assert prof["nb_first"] == 1
    exp = ar.expected(oracle, B, cr.PLANT_R)
    assert sum(x["rc"] < 0 for x in exp) == 2 and len(exp) == 42


def flags_case():
    B = ar.Batch()
    rng = np.random.RandomState(2)
    for k, (a, fa, b, fb) in enumerate(cr.flags_batch()):
        B.add_pair(B.place(rng, a, fa, k % 3), B.place(rng, b, fb, (k + 1) % 3), fa, fb, tag=f"flags{k}")
    return B


@pytest.mark.parametrize("flags", FLAGS)
def test_flag_combinations(ctx, oracle, flags):
    B = flags_case()
    check_batch(ctx, oracle, B, cr.PLANT_R, flags)
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs, PAIR_DTYPE)
    _, base, bc = ctx.align_batch_cigar(S, S, pairs, cr.PLANT_R, flags=0)
    _, got, gc = ctx.align_batch_cigar(S, S, pairs, cr.PLANT_R, flags=flags)
    swap = {cr.INS: cr.DEL, cr.DEL: cr.INS, cr.EQ: cr.EQ, cr.X: cr.X}
    for q in range(len(B.pairs)):
        want = [int(w) for w in base[q]]
        if flags & cr.B_IS_QUERY:                              # I and D exchanged, nothing else
            want = [(w >> 4 << 4) | swap[w & 15] for w in want]
            assert (gc["n_ins"][q], gc["n_del"][q]) == (bc["n_del"][q], bc["n_ins"][q])
        if flags & cr.REVERSED:                                # the mirror of origin-first
            want = want[::-1]
        assert got[q].tolist() == want and len(want) > 3, q
        assert (gc["n_eq"][q], gc["n_x"][q]) == (bc["n_eq"][q], bc["n_x"][q])


@pytest.mark.parametrize("row", EDGE_ROWS)
def test_every_ring(ctx, oracle, row):
    """k_cigar_pairs<nb1> on the edge set built for that ring, behind its pilot"""
    B = forced(row, ar.edge_pairs(row[0], EDGE_R))
    assert check_batch(ctx, oracle, B, EDGE_R)["nb_first"] == row[0]


def test_rerun_excursions(ctx, oracle):
    B, w, wl = excursion_case()
    need = len(must_redo(ar.expected(oracle, B, ar.EXC_R), B.meta, w, wl))
    prof = check_batch(ctx, oracle, B, ar.EXC_R)
    assert prof["nb_first"] == 1 and prof["nb_redo"] == 2 and prof["n_redo"] >= need


@pytest.mark.parametrize("row", sorted(ar.WIDE))
def test_rerun_reference_band(ctx, oracle, row):
    B, R = ar.wide_pairs(row)
    prof = check_batch(ctx, oracle, B.subset([0]), R)
    assert prof["nb_redo"] == row[1] and prof["n_redo"] == 1


# ----------------------------------------------------------------------------- rows
MAP_R = 0.30


@pytest.fixture(scope="module")
def mapped(ctx, oracle):
    """many_contig_case mapped with strands 3, and the oracle's runs on the mapper's own pair for every found row"""
    contigs, reads, _ = many_contig_case(961, n_reads=120)
    mask = eng.mask_from_pattern(MASK_PAT)
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    Rc = ctx.seqs_revcomp(Rd)
    rows, _ = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, MAP_R, 50, 500, strands=3, reads_rc=Rc)
    want_runs, want_counts = [], []
    for r in rows:
        if not r["found"]:
            want_runs.append([])
            want_counts.append(dict.fromkeys(CNT, 0))
            continue
        _, ap, al, _, bp, bl, _ = cr.map_row_aln_pair(r, len(contigs[int(r["contig"])]), len(reads[int(r["read"])]), MAP_R)
        text = reads[int(r["read"])] if r["strand"] == 1 else rc(reads[int(r["read"])])
        a, b = text[ap:ap + al], contigs[int(r["contig"])][bp:bp + bl]
        x = oracle.align(a, b, MAP_R, want_ops=True)
        assert (x["rc"] >= 0, x["cost"], x["matlen_a"], x["matlen_b"]) == (True, r["cost"], r["matlen_a"], r["matlen_b"])
        w, c = cr.runs(x["ops"], a, b, 0)
        want_runs.append(w)
        want_counts.append(c)
    assert sum(1 for r in rows if r["found"]) >= 60 and {int(s) for s in rows["strand"]} == {1, -1, 0}
    return dict(contigs=contigs, reads=reads, T=T, Rd=Rd, Rc=Rc, rows=rows, runs=want_runs, counts=want_counts)


def test_mapped_rows(ctx, mapped):
    m = mapped
    runs, counts, off, res, total = ctx.map_cigar(m["T"], m["Rd"], m["rows"], MAP_R, reads_rc=m["Rc"])
    woff, wtotal, _ = cr.layout(m["runs"])
    assert off.tolist() == woff and total == wtotal
    for k, r in enumerate(m["rows"]):
        assert runs[k].tolist() == m["runs"][k], k
        assert {n: int(counts[k][n]) for n in CNT} == m["counts"][k], k
        if r["found"]:
            assert (res[k]["cost"], res[k]["matlen_a"], res[k]["matlen_b"]) == (r["cost"], r["matlen_a"], r["matlen_b"])
        else:
            assert res[k]["rc"] == -1
    rl, cl = [len(x) for x in m["reads"]], [len(x) for x in m["contigs"]]
    lines = eng.paf_map_lines(m["rows"], counts, runs, rl, cl)
    assert lines == cr.paf_map_lines(m["rows"], m["counts"], m["runs"], rl, cl) and len(lines) >= 60


def raw_map_cigar(ctx, m, rows, cap, max_slots):
    n = len(rows)
    rows = np.ascontiguousarray(rows, MAP_ROW_DTYPE)
    cig = np.full(max(cap, 1), 0xFFFFFFFF, np.uint32)
    off = np.zeros(n + 1, np.uint64)
    total = C.c_uint64()
    st = ctx.lib.pba_map_rows_cigar_budget(ctx.h, m["T"].h, m["Rd"].h, m["Rc"].h, rows.ctypes.data, n, MAP_R, cig.ctypes.data, cap,
                                           off.ctypes.data, C.byref(total), None, None, max_slots)
    return st, cig, off, total.value


def test_mapped_rows_chunks_and_cap(ctx, mapped):
    m = mapped
    woff, wtotal, wdense = cr.layout(m["runs"])
    bounds = [cr.bound(*cr.map_row_aln_pair(r, len(m["contigs"][int(r["contig"])]), len(m["reads"][int(r["read"])]), MAP_R)[2:6:3], MAP_R)
              for r in m["rows"] if r["found"]]
    max_slots = sum(bounds) // 3 - 1                            # at least three chunks (four, by the greedy take)
    assert max_slots > max(bounds)
    for ms in (0, max_slots, 1):                               # the default, >= 3 chunks, one row per chunk
        st, cig, off, total = raw_map_cigar(ctx, m, m["rows"], wtotal, ms)
        assert st == 0 and total == wtotal and off.tolist() == woff and cig[:wtotal].tolist() == wdense, ms
    cap = woff[len(woff) // 2] + 1                              # below the total: whole rows only, offsets and total complete
    _, _, dense = cr.layout(m["runs"], cap)
    st, cig, off, total = raw_map_cigar(ctx, m, m["rows"], cap, 0)
    assert st == 0 and total == wtotal and off.tolist() == woff and 0 < len(dense) < cap
    assert cig[:len(dense)].tolist() == dense and (cig[len(dense):] == 0xFFFFFFFF).all()


def test_mapped_row_with_another_cost_is_refused(ctx, mapped):
    m = mapped
    rows = m["rows"].copy()
    k = int(np.flatnonzero(rows["found"] == 1)[3])
    rows["cost"][k] += 1
    with pytest.raises(PbaError) as e:
        ctx.map_cigar(m["T"], m["Rd"], rows, MAP_R, reads_rc=m["Rc"])
    assert e.value.status == -1 and f"row {k} " in str(e.value)
    with pytest.raises(PbaError) as e:                          # a strand -1 row without reads_rc
        ctx.map_cigar(m["T"], m["Rd"], m["rows"], MAP_R)
    assert e.value.status == -1


def test_overlap_rows(ctx, oracle):
    texts = overlap_case()
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, mask, 0.30, 32, 64, strands=3, reads_rc=Src)
    assert {(int(r["strand"]), int(r["dir"])) for r in rows} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    runs, counts, off, res, total = ctx.overlap_cigar(S, rows, 0.30, reads_rc=Src)
    want_runs, want_counts = [], []
    for k, r in enumerate(rows):
        t, q = texts[int(r["target"])], texts[int(r["query"])]
        qt = q if r["strand"] == 1 else rc(q)
        p = eng.overlap_row_pair(r, len(t), len(q))
        back = int(p["flags"]) == 3
        assert back == (r["dir"] == -1) and int(p["flags"]) in (0, 3)
        ap, al, bp, bl = int(p["a_pos"]), int(p["a_len"]), int(p["b_pos"]), int(p["b_len"])
        a = t[ap - al + 1:ap + 1][::-1] if back else t[ap:ap + al]
        b = qt[bp - bl + 1:bp + 1][::-1] if back else qt[bp:bp + bl]
        x = oracle.align(a, b, 0.30, want_ops=True)
        assert (x["rc"] >= 0, x["cost"], x["matlen_a"], x["matlen_b"]) == (True, r["cost"], r["matlen_a"], r["matlen_b"]), k
        fl = cr.B_IS_QUERY | (cr.REVERSED if back else 0)
        w, c = cr.runs(x["ops"], a, b, fl)
        want_runs.append(w)
        want_counts.append(c)
        assert runs[k].tolist() == w and {n: int(counts[k][n]) for n in CNT} == c, k
        # the target's forward order: the runs replay the target interval against the query interval, both forward
        ta, qa = t[int(r["t_beg"]):int(r["t_end"])], q[int(r["q_beg"]):int(r["q_end"])]
        qa = qa if r["strand"] == 1 else rc(qa)
        i = j = 0
        for word in w:
            n, op = word >> 4, word & 15
            if op in (cr.EQ, cr.X):
                assert all((ta[i + d] == qa[j + d]) == (op == cr.EQ) for d in range(n)), k
            i += n if op != cr.INS else 0
            j += n if op != cr.DEL else 0
        assert (i, j) == (len(ta), len(qa)), k
    woff, wtotal, wdense = cr.layout(want_runs)
    assert off.tolist() == woff and total == wtotal and len(rows) >= 4
    runs3, _, off3, _, _ = ctx.overlap_cigar(S, rows, 0.30, reads_rc=Src, max_slots=max(1, sum(len(w) for w in want_runs) // 2))
    assert off3.tolist() == woff and [x.tolist() for x in runs3] == want_runs
    rl = [len(x) for x in texts]
    assert eng.paf_overlap_lines(rows, counts, runs, rl) == cr.paf_overlap_lines(rows, want_counts, want_runs, rl)
    bad = rows.copy()
    bad["matlen_b"][1] -= 1
    with pytest.raises(PbaError) as e:
        ctx.overlap_cigar(S, bad, 0.30, reads_rc=Src)
    assert e.value.status == -1


def test_refusals(ctx):
    B = flags_case()
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs, PAIR_DTYPE)
    n = pairs.size

    def raw(S_a, S_b, pairs, off, R=cr.PLANT_R):
        n = pairs.size
        out, ncig, counts = np.zeros(n, RESULT_DTYPE), np.zeros(n, np.int32), np.zeros(n, ALN_COUNTS_DTYPE)
        cig = np.zeros(int(off[-1]) + 1, np.uint32)
        return ctx.lib.pba_align_batch_cigar(ctx.h, S_a.h, S_b.h, pairs.ctypes.data, n, R, 0, 0, 0, out.ctypes.data, cig.ctypes.data,
                                             off.ctypes.data, ncig.ctypes.data, counts.ctypes.data)

    bounds = [cr.bound(int(p["a_len"]), int(p["b_len"]), cr.PLANT_R) for p in pairs]
    off = np.concatenate([[0], np.cumsum(bounds)]).astype(np.uint64)
    assert raw(S, S, pairs, off) == 0
    short = off.copy()
    short[5:] -= 1                                              # pair 4 is one slot short of the bound
    assert raw(S, S, pairs, short) == -1
    N = ctx.seqs_from_list([s[:-1] + b"N" if len(s) > 3 else s for s in B.seqs])
    assert raw(N, S, pairs, off) == -6 and raw(S, N, pairs, off) == -6
    # a band too wide for the bit-vector array: there is no row-sweep form
    pil = ar.pilot(10795, EDGE_R)
    W = ctx.seqs_from_list([pil[0], pil[1]], strict_acgt=True)
    wp = np.array([(0, 0, len(pil[0]), 1, 0, len(pil[1]), 0)], PAIR_DTYPE)
    woff = np.array([0, cr.bound(len(pil[0]), len(pil[1]), EDGE_R)], np.uint64)
    assert raw(W, W, wp, woff, EDGE_R) == -4


def test_example_prints_the_paf_lines(ctx, mapped, tmp_path):
    """examples/map_paf_gpu.cpp builds with g++ -Wall -Werror over the C ABI and prints what paf_map_lines gives"""
    m = mapped
    libdir = os.path.join(ROOT, "pacbioassembly_amd", "lib")
    exe = str(tmp_path / "map_paf_gpu")
    subprocess.run(["g++", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "examples", "map_paf_gpu.cpp"), "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}"], check=True)
    contig_file = tmp_path / "contigs.txt"
    contig_file.write_bytes(b"".join(c + b"\n" for c in m["contigs"]))       # (an empty line is an empty contig)
    r = subprocess.run([exe, str(contig_file), MASK_PAT, str(MAP_R), "3"], input=b"".join(x + b"\n" for x in m["reads"]),
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    runs, counts, _, _, _ = ctx.map_cigar(m["T"], m["Rd"], m["rows"], MAP_R, reads_rc=m["Rc"])
    want = eng.paf_map_lines(m["rows"], counts, runs, [len(x) for x in m["reads"]], [len(c) for c in m["contigs"]])
    assert r.stdout.decode().splitlines() == want and len(want) >= 60
