"""Shared by tests/test_polish_cpu.py and tests/test_gpu_polish.py: contig polishing composed from the CPU oracle's pieces
(ref_seq ctor, align with traceback, try_align's gate, elect, evolve) over pba_map_reads rows -- the expectation
pba_pileup_vote_mapped and pba_polish_contigs are held to -- and the builders of the inputs, so that their seeds can be
chosen on the CPU (PYTHONPATH=.:tests python tests/polish_helpers.py SEED ... prints what the conditions of
tests/test_gpu_polish.py see for each seed)."""
import numpy as np

from map_ref import map_reads_ref, mutate, rand_text, rc
from pacbioassembly_amd import engine as eng

R = 0.30
OVERLAP_MIN = 64
TILE = 4096
POLISH_LENS = [0, 12, 700, 4097, 9000, 70001]
RES_KEYS = ("rc", "cost", "matlen_a", "matlen_b", "len_a", "len_b", "max_dst")


def clip_len(rem_a: int, b_len: int, R: float) -> int:
    """a_len of the pair a mapped row votes with, by hand: the contig remainder cut to b_len + max_dst."""
    return min(rem_a, b_len + 1 + int(b_len * R))


def row_texts(row, contigs, reads, R):
    """(pair, a, b): pba_map_row_pair of a found row and the elements of its two accessors (b from rc(read) on strand -1)."""
    T = contigs[int(row["contig"])]
    Q = reads[int(row["read"])]
    if int(row["strand"]) < 0:
        Q = rc(Q)
    pr = eng.map_row_pair(row, len(T), len(Q), R)
    ap, al, bp, bl = (int(pr[k]) for k in ("a_pos", "a_len", "b_pos", "b_len"))
    return pr, T[ap:ap + al], Q[bp:bp + bl]


def oracle_vote(oracle, contigs, reads, rows, c, weight=1, R=R, overlap_min=OVERLAP_MIN):
    """Contig c as ref_seq(T, weight) with every found row of `rows` on it through try_align's align + gate + elect, no
    growth.  Returns (the consensus object, {row index: align result}, rows voted)."""
    cons = oracle.consensus(contigs[c], weight)
    res, voted = {}, 0
    for k, r in enumerate(rows):
        if not r["found"] or int(r["contig"]) != c:
            continue
        pr, a, b = row_texts(r, contigs, reads, R)
        out = oracle.align(a, b, R, want_ops=True)
        res[k] = out
        if out["rc"] >= 0 and out["matlen_a"] >= overlap_min:
            cons.elect(int(pr["a_pos"]), True, out["ops"], eng.script_vals(out["ops"], b, True))
            voted += 1
    return cons, res, voted


def oracle_boxes(cons, n):
    sel, sup, tot, _ = cons.dump(n + 8)
    return sel, sup, tot


def oracle_evolve(cons, n) -> bytes:
    cons.evolve()
    return cons.text(2 * n + 8)


def oracle_polish_round(oracle, contigs, reads, rows, weight=1, R=R, overlap_min=OVERLAP_MIN):
    """One round: (next contigs, rows voted per contig)."""
    out, voted = [], []
    for c, T in enumerate(contigs):
        if len(T) == 0:
            out.append(b""); voted.append(0)
            continue
        cons, _, v = oracle_vote(oracle, contigs, reads, rows, c, weight, R, overlap_min)
        out.append(oracle_evolve(cons, len(T))); voted.append(v)
    return out, voted


def check_result(got, exp, tag):
    assert int(got["rc"]) == exp["rc"], (tag, int(got["rc"]), exp)
    for k in ("len_a", "len_b", "max_dst"):
        assert int(got[k]) == exp[k], (tag, k)
    if exp["rc"] >= 0:
        for k in ("cost", "matlen_a", "matlen_b"):
            assert int(got[k]) == exp[k], (tag, k, int(got[k]), exp)


# ----------------------------------------------------------------------------- inputs
def polish_case(seed: int, n_reads: int = 300, err: float = 0.12):
    """(contigs, reads): POLISH_LENS contigs and n_reads reads of 600 - 1 500 bases at `err` error, every second one (by a
    seeded draw) reverse-complemented.  Planted: reads beyond position 65 535 of the long contig; reads that run over a
    contig's last base into random text; reads that start 30 - 60 bases before a contig's end (found by the mapper, but the
    contig remainder is below OVERLAP_MIN); 6 unrelated reads.  The rest is drawn over the contigs by length."""
    rng = np.random.default_rng(seed)
    contigs = [rand_text(rng, n) for n in POLISH_LENS]
    real = [c for c, n in enumerate(POLISH_LENS) if n >= 700]
    reads = []
    long_c = POLISH_LENS.index(70001)
    for s in (65600, 66000, 67111, 68000, 68400):
        reads.append(mutate(rng, contigs[long_c][s:s + int(rng.integers(600, 1500))], err, keep=20))
    for c in real[1:]:
        T = contigs[c]
        for over in (40, 200):
            L = int(rng.integers(600, 1200))
            reads.append(mutate(rng, T[len(T) - L:], err, keep=20) + rand_text(rng, over))
        for tail in (30, 45, 60):
            reads.append(T[len(T) - tail:] + rand_text(rng, 700))
    for _ in range(6):
        reads.append(rand_text(rng, int(rng.integers(600, 1501))))
    w = np.array([len(contigs[c]) for c in real], float)
    while len(reads) < n_reads:
        T = contigs[real[int(rng.choice(len(real), p=w / w.sum()))]]
        L = int(rng.integers(600, min(1500, len(T)) + 1))
        s = int(rng.integers(0, len(T) - L + 1))
        reads.append(mutate(rng, T[s:s + L], err, keep=20))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    flip = rng.integers(0, 2, len(reads)).astype(bool)
    return contigs, [rc(x) if f else x for x, f in zip(reads, flip)]


def case_conditions(oracle, contigs, reads, rows):
    """What tests/test_gpu_polish.py requires of its input, from the oracle alone: voted rows per strand, found rows that do
    not vote, voted rows with pos > 65 535."""
    out = {"voted": {1: 0, -1: 0}, "found_not_voted": 0, "voted_far": 0}
    for c in range(len(contigs)):
        if not len(contigs[c]):
            continue
        _, res, _ = oracle_vote(oracle, contigs, reads, rows, c)
        for k, o in res.items():
            if o["rc"] >= 0 and o["matlen_a"] >= OVERLAP_MIN:
                out["voted"][int(rows[k]["strand"])] += 1
                out["voted_far"] += int(rows[k]["pos"]) > 65535
            else:
                out["found_not_voted"] += 1
    return out


EDGE_INS = (4095, 8191)            # an inserted base right after these contig positions (boxes = 4 095 mod 4 096: two characters)
EDGE_DEL = ((12287, 12288), (16384,))   # contig bases the reads lack (12 287: a tile's last box; 12 288, 16 384: a tile's first box)


def edge_case(seed: int, length: int = 70001):
    """(contig of `length` bases, 24 reads): 6 reads over each planted site, exact copies of 900 bases of the contig apart from
    the plant, starting 400 - 485 bases before it (every read ends below 16 900).  The contig reads ACGT around every site and
    the inserted base is a T between the C and the G, so that the cheapest alignment is unique and puts the edit on the
    planted box."""
    rng = np.random.default_rng(seed)
    T = bytearray(rand_text(rng, length))
    reads = []
    for site in EDGE_INS:
        T[site - 1:site + 3] = b"ACGT"                                  # C at `site`, G behind it
    for dels in EDGE_DEL:
        T[dels[0] - 1:dels[0] + 3] = b"ACGT" if len(dels) == 2 else b"ACGA"   # the bases lost: C, G / C
    T = bytes(T)
    for site, lost in [(s, 0) for s in EDGE_INS] + [(d[0], len(d)) for d in EDGE_DEL]:
        for k in range(6):
            s = site - 400 - 17 * k
            seg = bytearray(T[s:s + 900])
            at = site - s
            if lost:
                del seg[at:at + lost]
            else:
                seg.insert(at + 1, ord("T"))
            reads.append(bytes(seg))
    return T, reads


def yields(sel, sup, tot):
    """Characters every box of a dump yields in evolve (ref_seq.h:327, 336: has_supply(0.5) + is_valid(0.5))."""
    return (sel.max(axis=1) > 0.5 * tot).astype(int) + (sup.max(axis=1) > 0.5 * tot).astype(int)


class PileupAs:
    """A pile-up handle presented with another set as its own (what a caller that mixes up its sets passes)."""

    def __init__(self, pile, reads):
        self.ctx, self.h, self.reads = pile.ctx, pile.h, reads


if __name__ == "__main__":
    import sys
    from oraclelib import Oracle
    orc = Oracle()
    mask = eng.mask_from_pattern("111*11*11*1*1111")
    for seed in [int(x) for x in sys.argv[1:]] or [701]:
        contigs, reads = polish_case(seed)
        rows, _, _ = map_reads_ref(orc, contigs, reads, mask, R)
        print(seed, "found", int(rows["found"].sum()), case_conditions(orc, contigs, reads, rows))
