"""Homopolymer compression and the lifting of rows (pba_hpc_*) restated in plain numpy, and the inputs of
tests/test_hpc_cpu.py (which pins this file by hand) and tests/test_gpu_hpc.py (which holds the device to it exactly).

For a sequence x of L bases: position p is a run head iff p == 0 or x[p] != x[p - 1]; hpc(x) is the bases at the heads;
S[k] is the position of head k, S[H] = L.  A half-open interval [b, e) of hpc(x) lifts to [S[b], S[e]) of x."""
import numpy as np

from correct_helpers import ACGT, rc

TILE = 8192                                                   # csrc/hpc.h: HPC_TILE, the bases a workgroup takes (256 plane words)
MAX_BASES_DEFAULT = 0x7FFFFFF0                                # csrc/pba_hpc.hip: kHpcMaxBases


def hpc(text: bytes):
    """(hpc(text), S) with S a list of H + 1 positions."""
    a = np.frombuffer(text, np.uint8)
    if a.size == 0:
        return b"", [0]
    heads = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
    return a[heads].tobytes(), heads.tolist() + [int(a.size)]


def n_chunks(lens, max_bases):
    """Consecutive sequences, at most max_bases input bases a chunk (0: the default), one sequence at least."""
    limit = min(max_bases, MAX_BASES_DEFAULT) if max_bases else MAX_BASES_DEFAULT
    k, lo = 0, 0
    while lo < len(lens):
        hi, bases = lo + 1, lens[lo]
        while hi < len(lens) and bases + lens[hi] <= limit:
            bases += lens[hi]
            hi += 1
        k, lo = k + 1, hi
    return k


def lift_overlaps(rows, S, lens):
    """pba_strand_overlap rows of the compressed set -> rows of the original set.  S[i]: the run starts of sequence i (H + 1
    entries); lens[i]: its original length."""
    out = rows.copy()
    for o in out:
        t, q, lq = int(o["target"]), int(o["query"]), int(lens[int(o["query"])])
        tb, te, qb, qe = S[t][int(o["t_beg"])], S[t][int(o["t_end"])], S[q][int(o["q_beg"])], S[q][int(o["q_end"])]
        o["t_beg"], o["t_end"], o["q_beg"], o["q_end"] = tb, te, qb, qe
        o["matlen_a"], o["matlen_b"] = te - tb, qe - qb
        o["ref_pos"] = tb if o["dir"] > 0 else te - 16
        wb, we = (qb, qe) if o["strand"] > 0 else (lq - qe, lq - qb)      # the walked query interval
        o["j"] = wb if o["dir"] > 0 else lq - we
    return out


def lift_map_rows(rows, S_reads, lens_reads, S_target):
    """pba_map_row rows of compressed reads against compressed contigs -> rows of the original sets."""
    out = rows.copy()
    for o in out:
        if not o["found"]:
            continue
        r, c, lr = int(o["read"]), int(o["contig"]), int(lens_reads[int(o["read"])])
        rb, re, cb, ce = S_reads[r][int(o["r_beg"])], S_reads[r][int(o["r_end"])], S_target[c][int(o["c_beg"])], S_target[c][int(o["c_end"])]
        o["r_beg"], o["r_end"], o["c_beg"], o["c_end"] = rb, re, cb, ce
        o["pos"], o["matlen_b"], o["matlen_a"] = cb, ce - cb, re - rb
        o["j"] = rb if o["strand"] > 0 else lr - re
        o["seglen"] = lr - int(o["j"])
    return out


# ----------------------------------------------------------------------------------------------------------------- inputs
def make_overlap_row(t, q, strand, d, cost, tb, te, qb, qe, lq):
    """A pba_strand_overlap record from its intervals (forward strand) on reads whose query has lq bases: j, ref_pos and the
    match lengths by include/pba.h's identities read backwards."""
    from pacbioassembly_amd.engine import STRAND_OVERLAP_DTYPE
    o = np.zeros(1, STRAND_OVERLAP_DTYPE)[0]
    o["target"], o["query"], o["strand"], o["dir"], o["cost"] = t, q, strand, d, cost
    o["t_beg"], o["t_end"], o["q_beg"], o["q_end"] = tb, te, qb, qe
    o["matlen_a"], o["matlen_b"] = te - tb, qe - qb
    o["ref_pos"] = tb if d > 0 else te - 16
    wb, we = (qb, qe) if strand > 0 else (lq - qe, lq - qb)
    o["j"] = wb if d > 0 else lq - we
    return o


def overlap_rows(tuples, hs):
    """[(t, q, strand, dir, cost, tb, te, qb, qe)] on compressed reads of hs[i] bases"""
    from pacbioassembly_amd.engine import STRAND_OVERLAP_DTYPE
    return np.array([make_overlap_row(*x, hs[x[1]]) for x in tuples], STRAND_OVERLAP_DTYPE) if tuples else np.zeros(0, STRAND_OVERLAP_DTYPE)


def random_overlap_rows(rng, hs, count, sentinel_every=4):
    """`count` valid rows on compressed reads of hs[i] bases (reads with hs == 0 are never named); every sentinel_every-th row
    spans [0, H) on both reads: index 0 and the sentinel S[H]."""
    live = [i for i, h in enumerate(hs) if h > 0]
    out = []
    while len(out) < count:
        t, q = (live[int(x)] for x in rng.integers(0, len(live), 2))
        if t == q:
            continue
        if len(out) % sentinel_every == 0:
            tb, te, qb, qe = 0, hs[t], 0, hs[q]
        else:
            tb, te = sorted(int(x) for x in rng.choice(hs[t] + 1, 2, replace=False))
            qb, qe = sorted(int(x) for x in rng.choice(hs[q] + 1, 2, replace=False))
        out.append((t, q, int(rng.choice((1, -1))), int(rng.choice((1, -1))), int(rng.integers(0, 50)), tb, te, qb, qe))
    return overlap_rows(out, hs)


def random_map_rows(rng, hs_reads, hs_target, count):
    """`count` pba_map_row records, every third one found == 0 (with the values a row that found nothing carries)."""
    from pacbioassembly_amd.engine import MAP_ROW_DTYPE
    live_r = [i for i, h in enumerate(hs_reads) if h > 0]
    live_c = [i for i, h in enumerate(hs_target) if h > 0]
    out = np.zeros(count, MAP_ROW_DTYPE)
    for k, o in enumerate(out):
        r = live_r[int(rng.integers(0, len(live_r)))]
        o["read"], o["nseq"], o["n_pairs"] = r, k, int(rng.integers(0, 9))
        if k % 3 == 2:
            o["j"], o["contig"], o["diag_cost"] = -1, -1, -1
            continue
        c = live_c[int(rng.integers(0, len(live_c)))]
        if k % 4 == 0:
            rb, re, cb, ce = 0, hs_reads[r], 0, hs_target[c]
        else:
            rb, re = sorted(int(x) for x in rng.choice(hs_reads[r] + 1, 2, replace=False))
            cb, ce = sorted(int(x) for x in rng.choice(hs_target[c] + 1, 2, replace=False))
        o["found"], o["strand"], o["contig"] = 1, int(rng.choice((1, -1))), c
        o["r_beg"], o["r_end"], o["c_beg"], o["c_end"] = rb, re, cb, ce
        o["pos"], o["matlen_a"], o["matlen_b"] = cb, re - rb, ce - cb
        o["j"] = rb if o["strand"] > 0 else hs_reads[r] - re
        o["seglen"] = hs_reads[r] - int(o["j"])
        o["cost"], o["diag_cost"] = int(rng.integers(0, 50)), int(rng.integers(0, 50))
    return out


# Two reads by hand.       0123456789.123            0123456789.
HAND_TEXTS = [b"AAACCGTTTTACGG", b"CCGGGTAACCG"]
HAND_HPC = [(b"ACGTACG", [0, 3, 5, 6, 10, 11, 12, 14]), (b"CGTACG", [0, 2, 5, 6, 8, 10, 11])]
# compressed rows (t, q, strand, dir, cost, tb, te, qb, qe) and, next to each, the lifted row written out:
# (target, query, strand, j, dir, ref_pos, cost, matlen_a, matlen_b, t_beg, t_end, q_beg, q_end).  Lq = 11 where the query is
# read 1, 14 where it is read 0.  t [1, 4) -> [3, 10): 7 bases; q [0, 4) -> [0, 8): 8 bases.
HAND_ROWS = [
    ((0, 1, 1, 1, 3, 1, 4, 0, 4), (0, 1, 1, 0, 1, 3, 3, 7, 8, 3, 10, 0, 8)),         # walked [0, 8): j = 0; ref_pos = t_beg
    ((0, 1, 1, -1, 3, 1, 4, 0, 4), (0, 1, 1, 3, -1, -6, 3, 7, 8, 3, 10, 0, 8)),      # j = 11 - 8; ref_pos = 10 - 16
    ((0, 1, -1, 1, 3, 1, 4, 0, 4), (0, 1, -1, 3, 1, 3, 3, 7, 8, 3, 10, 0, 8)),       # walked [11 - 8, 11 - 0) = [3, 11): j = 3
    ((0, 1, -1, -1, 3, 1, 4, 0, 4), (0, 1, -1, 0, -1, -6, 3, 7, 8, 3, 10, 0, 8)),    # j = 11 - 11
    # the whole target, index 0 and the sentinel: t [0, 7) -> [0, 14); q [2, 6) -> [5, 11): walked [0, 6), j = 11 - 6
    ((0, 1, -1, -1, 0, 0, 7, 2, 6), (0, 1, -1, 5, -1, -2, 0, 14, 6, 0, 14, 5, 11)),
    # roles swapped: t = read 1 [5, 6) -> [10, 11); q = read 0 [6, 7) -> [12, 14): one compressed base each, two original
    ((1, 0, 1, 1, 9, 5, 6, 6, 7), (1, 0, 1, 12, 1, 10, 9, 1, 2, 10, 11, 12, 14)),
    ((1, 0, -1, -1, 9, 5, 6, 0, 1), (1, 0, -1, 0, -1, -5, 9, 1, 3, 10, 11, 0, 3)),   # q [0, 1) -> [0, 3): walked [11, 14), j = 14 - 14
]
LIFTED_FIELDS = ("target", "query", "strand", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b", "t_beg", "t_end", "q_beg", "q_end")


def hand_rows():
    hs = [len(c) for c, _ in HAND_HPC]
    return overlap_rows([r for r, _ in HAND_ROWS], hs), [w for _, w in HAND_ROWS]


def as_tuples(rows, fields=LIFTED_FIELDS):
    return [tuple(int(r[f]) for f in fields) for r in rows]


EDGE_LENS = [0, 1, 2, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
SHAPES = ("random", "single_run", "alternating", "runs_of_32", "runs_past_word")


def shaped(rng, shape, n):
    """n bases: random; one single run (H == 1: the carry crosses every word, wave and tile boundary); strictly alternating
    (H == L); runs of exactly 32 (every head at a word start); runs that end one base past a word boundary (heads at 32 k + 1)."""
    if shape == "random":
        return rng.choice(ACGT, n).tobytes()
    if shape == "single_run":
        return bytes([int(ACGT[int(rng.integers(0, 4))])]) * n
    if shape == "alternating":
        a, b = (int(x) for x in rng.choice(ACGT, 2, replace=False))
        return bytes([a, b] * (n // 2 + 1))[:n]
    first = 32 if shape == "runs_of_32" else 33               # the first run's length; every later run has 32 bases
    out, k = bytearray(), int(rng.integers(0, 4))
    while len(out) < n:
        out += bytes([int(ACGT[k % 4])]) * (first if not out else 32)
        k += int(rng.integers(1, 4))                          # another base than the run before
    return bytes(out[:n])


def edge_set(shape, seed=501):
    rng = np.random.default_rng(seed)
    return [shaped(rng, shape, n) for n in EDGE_LENS]


def touching_set():
    """Every sequence ends in the base the next one starts with (ending in A and starting with A included), with empty
    sequences between them: no carry may cross a sequence, and the pad bits (zero = A) of a last word must not count."""
    rng = np.random.default_rng(502)
    out, first = [], b"A"
    for k, n in enumerate([5, 32, 33, 64, 1, 1, 31, 95, 96, 2, 40, 64, 7]):
        last = b"A" if k % 2 == 0 else bytes([int(ACGT[int(rng.integers(1, 4))])])
        x = first if n == 1 else first + rng.choice(ACGT, n - 2).tobytes() + last
        out.append(x)
        first = x[-1:]
        if k % 3 != 2:
            out.append(b"")
    return out


def biased_set(seed=503, n=200, lo=2, hi=900):
    """n sequences of lo .. hi bases (three longer than a tile) whose run lengths are drawn with a heavy tail"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        want = int(rng.integers(lo, hi)) if i not in (17, 101, 180) else int(rng.integers(TILE + 1, 2 * TILE))
        x, k = bytearray(), int(rng.integers(0, 4))
        while len(x) < want:
            run = int(rng.choice((1, 1, 1, 2, 2, 3, 5, 8, 40)))
            x += bytes([int(ACGT[k % 4])]) * run
            k += int(rng.integers(1, 4))
        out.append(bytes(x[:want]))
    return out


def redraw_runs(rng, text: bytes, choices=(1, 1, 2, 2, 3, 4, 6)):
    """text with only its run lengths drawn again (never zero): hpc(result) == hpc(text)"""
    comp, _ = hpc(text)
    return b"".join(bytes([c]) * int(rng.choice(choices)) for c in comp)


PLANTED = dict(glen=6000, n=12, rl=1500, stride=750, seed=504, R=0.30, overlap_min=64)


def planted_reads(P=PLANTED):
    """A random genome of glen bases read as a circle (12 reads of 1 500 bases at a stride of 750 go round a 6 kb genome once and
    a half: read k + 8 covers the span of read k); every read with only its run lengths drawn again; every second read
    reverse-complemented.  Returns (texts, the slices of the genome before the run lengths were drawn again)."""
    rng = np.random.default_rng(P["seed"])
    g = rng.choice(ACGT, P["glen"]).tobytes()
    texts, clean = [], []
    for k in range(P["n"]):
        b = (k * P["stride"]) % P["glen"]
        x = (g + g)[b:b + P["rl"]]
        clean.append(x)
        y = redraw_runs(rng, x)
        texts.append(rc(y) if k & 1 else y)
    return texts, clean


def consecutive_pairs_at_cost_0(rows, n):
    """the k of 0 .. n - 2 for which reads k and k + 1 have a row at cost 0 in at least one role"""
    have = {(int(r["target"]), int(r["query"])) for r in rows if int(r["cost"]) == 0}
    return [k for k in range(n - 1) if (k, k + 1) in have or (k + 1, k) in have]
