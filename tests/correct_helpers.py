"""Shared by tests/test_correct_cpu.py and tests/test_gpu_correct.py: mixed-strand read sets, the overlap rows the CPU
oracle gives for them, and read correction composed from the oracle's pieces (ref_seq ctor, align with traceback, elect,
evolve) -- the expectation the device pile-up is held to."""
import numpy as np

from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import STRAND_OVERLAP_DTYPE

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def rc(x: bytes) -> bytes:
    return x.translate(_COMP)[::-1]


def mixed_reads(seed_g, seed_r, n, rl, glen, rl_min=None, extra=0):
    """n reads of a synthetic genome (15 % error), cut to lengths in [rl_min, rl] when rl_min is given, every second one
    (by a seeded draw) reverse-complemented; `extra` unrelated random reads are appended.  Returns (texts, starts, flip)."""
    g = eng.synth_genome(seed_g, glen)
    reads, offs, starts = eng.synth_reads(seed_r, g, n, rl)
    rng = np.random.default_rng(seed_r + 1000)
    texts = [reads[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
    if rl_min is not None:
        texts = [t[:int(rng.integers(rl_min, rl + 1))] for t in texts]
    flip = rng.integers(0, 2, n).astype(bool)
    texts = [rc(x) if f else x for x, f in zip(texts, flip)]
    for _ in range(extra):
        texts.append(rng.choice(ACGT, rl).tobytes())
    return texts, starts, flip


def record_file(texts):
    file = b"".join(eng.text2bin(t) for t in texts)
    offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in texts[:-1]]).astype(np.uint64)
    return file, offs


def intervals(row, qlen):
    """(t_beg, t_end, q_beg, q_end) of a row as include/pba.h defines them for pba_strand_overlap."""
    j, d, p, ma, mb = (int(row[k]) for k in ("j", "dir", "ref_pos", "matlen_a", "matlen_b"))
    if d > 0:
        tb, te, b0, b1 = p, p + ma, j, j + mb
    else:
        tb, te, b0, b1 = p + 16 - ma, p + 16, qlen - j - mb, qlen - j
    return (tb, te, b0, b1) if int(row["strand"]) > 0 else (tb, te, qlen - b1, qlen - b0)


def oracle_rows(oracle, texts, mask, R=0.30, max_trial=32, overlap_min=64, targets=None, nthreads=8):
    """The rows pba_overlap_strands is specified to return, from the oracle: a locked spaced_seed round of every target
    over the file of the reads (+1) and over the file of their reverse complements (-1), q != t; sorted by
    (target, query, strand) with +1 first."""
    n = len(texts)
    files = {1: record_file(texts), -1: record_file([rc(x) for x in texts])}
    out = []
    for t in (range(n) if targets is None else targets):
        per = {s: oracle.spaced_round(texts[t], mask, R, f, o, max_trial, overlap_min, buggy=False, nthreads=nthreads)
               for s, (f, o) in files.items()}
        for q in range(n):
            for s in (1, -1):
                w = per[s][q]
                if q == t or not w["found"]:
                    continue
                r = np.zeros(1, STRAND_OVERLAP_DTYPE)[0]
                r["target"], r["query"], r["strand"] = t, q, s
                for k in ("j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b"):
                    r[k] = w[k]
                r["t_beg"], r["t_end"], r["q_beg"], r["q_end"] = intervals(r, len(texts[q]))
                out.append(r)
    return np.array(out, STRAND_OVERLAP_DTYPE) if out else np.zeros(0, STRAND_OVERLAP_DTYPE)


def pair_texts(pair, texts, strand):
    """(a, b, fwd): the elements of a pair's two accessors in memory order (a backward accessor starts at its last byte),
    b taken from the reverse complement of the query for a strand -1 row."""
    T = texts[int(pair["a_seq"])]
    Q = texts[int(pair["b_seq"])]
    if strand < 0:
        Q = rc(Q)
    fwd = int(pair["flags"]) == 0
    ap, al, bp, bl = (int(pair[k]) for k in ("a_pos", "a_len", "b_pos", "b_len"))
    if fwd:
        return T[ap:ap + al], Q[bp:bp + bl], True
    return T[ap - al + 1:ap + 1], Q[bp - bl + 1:bp + 1], False


def oracle_correct(oracle, texts, t, rows_t, weight, R=0.30):
    """Target t corrected by the oracle's pieces: ref_seq(T, weight), for every row align with traceback and elect, evolve.
    Returns (sel, sup, tot before evolve, corrected text)."""
    T = texts[t]
    c = oracle.consensus(T, weight)
    for r in rows_t:
        pr = eng.overlap_row_pair(r, len(T), len(texts[int(r["query"])]))
        a, b, fwd = pair_texts(pr, texts, int(r["strand"]))
        res = oracle.align(a, b, R, a_fwd=fwd, b_fwd=fwd, want_ops=True)
        assert (res["rc"] >= 0 and res["cost"] == int(r["cost"]) and res["matlen_a"] == int(r["matlen_a"])
                and res["matlen_b"] == int(r["matlen_b"])), (r, res)
        c.elect(int(pr["a_pos"]), fwd, res["ops"], eng.script_vals(res["ops"], b, fwd))
    sel, sup, tot, _ = c.dump(len(T) + 8)
    c.evolve()
    return sel, sup, tot, c.text(2 * len(T) + 8)


def check_dump_cap(dump, full, cap=7):
    """dump(sel, sup, tot, cap, n_ref) -> status is a box dump of the C ABI bound to its object; full: (sel, sup, tot) of all
    its boxes.  With room for `cap` boxes it reports the whole count, writes the first `cap` and leaves the next slot alone."""
    import ctypes as C
    sel = np.full((cap + 1, 4), 0xABCD, np.uint16); sup = np.full((cap + 1, 4), 0xABCD, np.uint16); tot = np.full(cap + 1, -77, np.int32)
    n = C.c_int32()
    assert dump(sel.ctypes.data_as(C.c_void_p), sup.ctypes.data_as(C.c_void_p), tot.ctypes.data_as(C.c_void_p), cap, C.byref(n)) == 0
    assert n.value == len(full[2]) and n.value > cap
    for got, want in zip((sel, sup, tot), full):
        assert (got[:cap] == want[:cap]).all()
    assert (sel[cap] == 0xABCD).all() and (sup[cap] == 0xABCD).all() and tot[cap] == -77
