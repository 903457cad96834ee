"""Run-length alignments without a GPU: the host twins of the device sink (pba_cigar_from_script, pba_cigar_string,
pba_cigar_bound, pba_map_row_aln_pair) against the plain Python of tests/cigar_ref.py on the oracle's own scripts, the bound
and the count identities on every success, and the planted inputs of tests/test_gpu_cigar.py proven to have the script
shapes they are named for.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import align_rings as ar
import cigar_ref as cr
from conftest import MASK_PAT
from map_ref import many_contig_case, map_reads_ref, rc
from pacbioassembly_amd import _lib
from pacbioassembly_amd import engine as eng
from test_align_rings_cpu import EDGE_R

FLAGS = (0, cr.REVERSED, cr.B_IS_QUERY, cr.REVERSED | cr.B_IS_QUERY)
MAP_R = 0.30


def check_helpers(lib, x, a, b, R, tag):
    """the four host helpers on one oracle answer; returns the fill of the slot (runs / bound) of a success"""
    bound = eng.cigar_bound(len(a), len(b), R)
    assert bound == cr.bound(len(a), len(b), R), tag
    if x["rc"] < 0:
        return None
    for fl in FLAGS:
        want, wc = cr.runs(x["ops"], a, b, fl)
        got, gc = eng.cigar_from_script(x["ops"], a, b, fl)
        assert got.tolist() == want and {n: int(gc[n]) for n in wc} == wc, (tag, fl)
        assert eng.cigar_string(got) == cr.string(want), (tag, fl)
        assert cr.identities(wc, x, fl), (tag, fl, wc, x)
        assert len(want) <= bound, (tag, len(want), bound)
    return len(want) / bound if bound else 0.0


def fuzz_pairs():
    """random pairs of up to 600 bases: R in {0.1, 0.15, 0.3, 0.45}, error 0 .. 30 %, either side the longer one"""
    rng = np.random.RandomState(8801)
    out = []
    for R in (0.1, 0.15, 0.3, 0.45):
        for k in range(60):
            m = int(rng.randint(1, 601)) if k % 6 else int(rng.randint(1, 14))
            e = (0.0, 0.02, 0.08, 0.15, 0.22, 0.30)[k % 6]
            x = ar.rand_seq(rng, m)
            y = ar.mutate(rng, x, e, head=min(40, m // 2)) + ar.rand_seq(rng, int(rng.randint(0, 80)))
            out.append((R,) + ((y, x) if k % 2 else (x, y)))
    return out


def test_scripts_fuzz(lib, oracle):
    fills, n_ok = [], 0
    for R, a, b in fuzz_pairs():
        f = check_helpers(lib, oracle.align(a, b, R, want_ops=True), a, b, R, (R, len(a), len(b)))
        if f is not None:
            n_ok += 1
            fills.append(f)
    assert n_ok >= 120 and max(fills) <= 1.0
    print("fullest slot: %.2f of the bound over %d successes" % (max(fills), n_ok))


def test_scripts_edge_pairs(lib, oracle):
    B = ar.edge_pairs(1, EDGE_R)
    n_ok = 0
    for q, x in enumerate(ar.expected(oracle, B, EDGE_R)):
        a, b = B.elems(q)
        n_ok += check_helpers(lib, x, a, b, EDGE_R, B.meta[q]["tag"]) is not None
    assert n_ok >= 40


def test_helper_refusals_and_caps(lib):
    ops = np.array([1, 1, 3, 1, 2, 2, 1], np.uint8)
    a, b = b"ACGTA", b"ACAGGA"
    want, _ = cr.runs(ops, a, b)
    assert cr.string(want) == "2=1I1X2D1="
    got, _ = eng.cigar_from_script(ops, a, b)
    assert got.tolist() == want
    cig = np.zeros(2, np.uint32)                              # a cap below the runs: the count is still returned
    assert lib.pba_cigar_from_script(ops.ctypes.data, ops.size, a, b, 0, cig.ctypes.data, 2, None) == len(want)
    assert cig.tolist() == want[:2]
    bad = np.array([1, 4], np.uint8)
    assert lib.pba_cigar_from_script(bad.ctypes.data, 2, a, b, 0, cig.ctypes.data, 2, None) == -1
    buf = C.create_string_buffer(64)
    w = np.array(want, np.uint32)
    assert lib.pba_cigar_string(w.ctypes.data, w.size, buf, 64) == 10 and buf.value == b"2=1I1X2D1="
    assert lib.pba_cigar_string(w.ctypes.data, w.size, buf, 10) == 0          # no room for the NUL
    assert lib.pba_cigar_string(w.ctypes.data, w.size, buf, 11) == 10
    assert eng.cigar_string(np.zeros(0, np.uint32)) == ""
    assert eng.cigar_bound(-1, 5, 0.3) == 0 and eng.cigar_bound(5, 5, 1.0) == 0
    assert eng.cigar_bound(10, 500, 0.3) == 10 + 14 and eng.cigar_bound(11, 500, 0.3) == 2 * 4 - 1
    assert C.sizeof(_lib.PbaAlnCounts) == 16 == eng.ALN_COUNTS_DTYPE.itemsize


@pytest.fixture(scope="module")
def mapped(oracle):
    contigs, reads, _ = many_contig_case(961, n_reads=120)
    mask = oracle.mask_from_pattern(MASK_PAT)
    rows, _, _ = map_reads_ref(oracle, contigs, reads, mask, MAP_R, 50, 500, strands=3)
    return contigs, reads, rows


def test_map_row_aln_pair(oracle, mapped):
    """the pair builder equals cigar_ref; the oracle on the clipped pair returns the row's cost and match lengths"""
    contigs, reads, rows = mapped
    found = [r for r in rows if r["found"]]
    assert len(found) >= 60 and {int(r["strand"]) for r in found} == {1, -1}
    longer_read = 0
    for r in found:
        cl, rl = len(contigs[int(r["contig"])]), len(reads[int(r["read"])])
        got = eng.map_row_aln_pair(r, cl, rl, MAP_R)
        assert tuple(int(got[f]) for f in eng.PAIR_DTYPE.names) == cr.map_row_aln_pair(r, cl, rl, MAP_R)
        text = reads[int(r["read"])] if r["strand"] == 1 else rc(reads[int(r["read"])])
        a = text[int(got["a_pos"]):int(got["a_pos"]) + int(got["a_len"])]
        b = contigs[int(r["contig"])][int(got["b_pos"]):int(got["b_pos"]) + int(got["b_len"])]
        assert len(a) == got["a_len"] and len(b) == got["b_len"]
        x = oracle.align(a, b, MAP_R)
        assert (x["rc"] >= 0, x["cost"], x["matlen_a"], x["matlen_b"]) == (True, r["cost"], r["matlen_a"], r["matlen_b"]), r
        longer_read += rl - int(r["j"]) > cl - int(r["pos"])
    assert longer_read >= 1                                   # a read whose remainder is longer than the contig's: a is clipped
    bad = np.zeros(1, eng.MAP_ROW_DTYPE)
    with pytest.raises(eng.PbaError):
        eng.map_row_aln_pair(bad[0], 100, 100, MAP_R)         # found == 0


def test_paf_formatters(mapped):
    contigs, reads, rows = mapped
    rng = np.random.default_rng(5)
    counts = np.zeros(len(rows), eng.ALN_COUNTS_DTYPE)
    for n in counts.dtype.names:
        counts[n] = rng.integers(0, 900, len(rows))
    cigars = [np.array([(int(rng.integers(1, 500)) << 4) | c for c in (7, 8, 1, 7, 2, 7)], np.uint32) for _ in rows]
    rl, cl = [len(x) for x in reads], [len(x) for x in contigs]
    got = eng.paf_map_lines(rows, counts, cigars, rl, cl)
    assert got == cr.paf_map_lines(rows, counts, cigars, rl, cl) and len(got) == int((rows["found"] == 1).sum())
    f = got[0].split("\t")
    assert len(f) == 14 and f[0].startswith("read") and f[5].startswith("contig") and f[11] == "255" and f[12].startswith("NM:i:")
    names = [f"r{k}" for k in range(len(reads))]
    assert eng.paf_map_lines(rows, counts, cigars, rl, cl, names, None) == cr.paf_map_lines(rows, counts, cigars, rl, cl, names, None)
    ov = np.zeros(3, eng.STRAND_OVERLAP_DTYPE)
    ov["target"], ov["query"], ov["strand"] = (0, 1, 2), (3, 4, 5), (1, -1, 1)
    ov["t_beg"], ov["t_end"], ov["q_beg"], ov["q_end"], ov["cost"] = (1, 2, 3), (100, 200, 300), (4, 5, 6), (90, 190, 290), (7, 8, 9)
    assert eng.paf_overlap_lines(ov, counts, cigars, rl) == cr.paf_overlap_lines(ov, counts, cigars, rl)
    assert eng.paf_overlap_lines(ov, counts, cigars, rl)[1].split("\t")[:6] == ["read4", str(rl[4]), "5", "190", "-", "read1"]


def test_planted_inputs_have_their_shapes(oracle):
    """every planted pair of the GPU test: the oracle's script, goal-first, is what the pair is named for"""
    R = cr.PLANT_R
    seen = set()
    for tag, a, b, exp in cr.planted_pairs():
        x = oracle.align(a, b, R, want_ops=True)
        if exp.get("fails"):
            assert x["rc"] < 0, tag
            seen.add("fails")
            continue
        assert x["rc"] >= 0, tag
        goal_first = cr.codes(x["ops"], a, b)[::-1]
        if exp.get("all_eq"):
            assert goal_first == [cr.EQ] * exp["n"], tag
            seen.add(("n", exp["n"]))
        if "edit" in exp:
            kind, k = exp["edit"]
            non_eq = [(i + 1, c) for i, c in enumerate(goal_first) if c != cr.EQ]
            assert len(non_eq) == 1 and non_eq[0][0] == k, (tag, non_eq)
            if kind != "any":
                assert cr.OPCH[non_eq[0][1]] == kind, (tag, non_eq)
            seen.add(("edit", kind, k))
        if "adjacent" in exp:
            k = exp["adjacent"]
            non_eq = [(i + 1, c) for i, c in enumerate(goal_first) if c != cr.EQ]
            assert [i for i, _ in non_eq] == [k, k + 1] and non_eq[0][1] != non_eq[1][1], (tag, non_eq)
            seen.add(("adjacent", k))
        if exp.get("corner"):
            assert min(x["len_a"], x["len_b"]) <= 10, tag
            seen.add("corner")
        if "border" in exp:
            assert int(x["ops"][0]) == exp["border"] and int(x["ops"][1]) == 1, (tag, x["ops"][:4])
            seen.add(("border", exp["border"]))
    assert {("n", n) for n in cr.TOTAL_OPS} <= seen and {("adjacent", 64), ("adjacent", 128), "corner", "fails"} <= seen
    assert {("edit", kind, k) for k in cr.GROUP_EDGES[1:] for kind in "XID"} | {("edit", "any", 1)} <= seen
    assert {("border", 2), ("border", 3)} <= seen
    # the flags batch: forward, both-backward and len_a > len_b pairs, all successes with X, I and D among their ops
    kinds, shapes = set(), set()
    for a, fa, b, fb in cr.flags_batch():
        ea, eb = (a[::-1] if fa else a), (b[::-1] if fb else b)
        x = oracle.align(ea, eb, R, want_ops=True)
        assert x["rc"] >= 0
        kinds |= set(cr.codes(x["ops"], ea, eb))
        shapes.add((fa, fb, len(a) > len(b)))
    assert kinds == {cr.EQ, cr.X, cr.INS, cr.DEL} and {(False, False, False), (True, True, False)} <= shapes
    assert any(s[2] for s in shapes)


def overlap_case():
    """the smallest read set tests/test_gpu_strands.py uses (12 reads of 900 bases of a 4 kb genome), every second one, by a
    seeded draw, reverse-complemented"""
    from test_gpu_strands import mixed_set
    texts, _ = mixed_set(61, 62, 12, 900, 4000)
    flip = np.random.default_rng(63).integers(0, 2, len(texts)).astype(bool)
    return [rc(x) if f else x for x, f in zip(texts, flip)]


def test_overlap_case_has_all_four_kinds(oracle):
    """(strand, dir) in {+1, -1}^2 all occur among the oracle's locked rounds of every target against the reads and against
    their reverse complements"""
    texts = overlap_case()
    mask = oracle.mask_from_pattern(MASK_PAT)
    kinds = set()
    for strand, qs in ((1, texts), (-1, [rc(x) for x in texts])):
        file = b"".join(eng.text2bin(t) for t in qs)
        offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in qs[:-1]]).astype(np.uint64)
        for t in range(len(texts)):
            rows = oracle.spaced_round(texts[t], mask, 0.30, file, offs, 32, 64, buggy=False, nthreads=4)
            kinds |= {(strand, int(rows["dir"][q])) for q in range(len(texts)) if q != t and rows["found"][q]}
    assert kinds == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
