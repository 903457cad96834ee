"""Placement of reads on their laid-out contigs from overlap rows (pba_layout_place), restated in plain Python:
one loop over the rows, one dict of winners, no atomics.  The device must equal this exactly.  Also here, shared by
tests/test_place_cpu.py and tests/test_gpu_place.py: the hand cases, the tilings, the fuzz rows, the inputs of the vote tests
and the vote composed from the CPU oracle's pieces (ref_seq ctor, align with traceback, try_align's gate, elect, evolve) --
the expectation pba_pileup_vote_placed and pba_layout_consensus are held to.

PYTHONPATH=.:tests python tests/place_ref.py SEED ... prints what the conditions of the noisy case see for each seed.

rows: records with the fields of pba_strand_overlap that the placement reads (target, query, strand, dir, cost, t_beg, t_end,
q_beg, q_end); lens: the read lengths; table: the layout's per-read table (tuples in layout_ref.ROW_FIELDS order)."""
import numpy as np

from layout_ref import ACGT, CONTAINED, PLACED, UNPLACED, combine, layout_ref, make_rows, rc, tiling
from pacbioassembly_amd import engine as eng

PLACE_FIELDS = ("read", "found", "row", "contig", "pos", "dir", "strand", "j")
PLACE_COUNTERS = ("n_rows", "n_target_not_placed", "n_outside", "n_eligible", "n_found", "n_found_placed", "n_found_contained",
                  "n_found_unplaced")
R = 0.30
OVERLAP_MIN = 64
RES_KEYS = ("rc", "cost", "matlen_a", "matlen_b", "len_a", "len_b", "max_dst")


def make_place_rows(tuples):
    """[(target, query, strand, cost, t_beg, t_end, q_beg, q_end, dir)] -> records with every pba_strand_overlap field."""
    out = make_rows([t[:8] for t in tuples])
    for k, t in enumerate(tuples):
        out[k]["dir"] = t[8]
    return out


def geometry(row, lens, table):
    """"not_placed" | "outside" | (contig, pos, dir', strand', j'): where the first pair of elements the row's alignment
    compares lies on the target's contig, and how the query's text runs from there."""
    t, q, strand, d = int(row["target"]), int(row["query"]), int(row["strand"]), int(row["dir"])
    lt, lq = int(lens[t]), int(lens[q])
    _, state, contig, _, orient, offset, skip, adv, _ = table[t]
    if state != PLACED:
        return "not_placed"
    if strand == 1:
        qb, qe = int(row["q_beg"]), int(row["q_end"])
    else:                                                     # the coordinates of the walked text rc(q)
        qb, qe = lq - int(row["q_end"]), lq - int(row["q_beg"])
    xa, yb = (int(row["t_beg"]), qb) if d == 1 else (int(row["t_end"]) - 1, qe - 1)
    at = xa if orient == 0 else lt - 1 - xa                   # the anchor base in the text the contig holds of t
    if not skip <= at < skip + adv:
        return "outside"
    pos = offset + at - skip
    if orient == 0:
        return contig, pos, d, strand, yb
    return contig, pos, -d, -strand, lq - 1 - yb              # the contig holds rc(t) there: everything turns round


def place_key(row, k):
    return (int(row["q_end"]) - int(row["q_beg"]), -min(max(int(row["cost"]), 0), 0xFFFF), -k)


def place_ref(lens, table, rows):
    """(placements: one tuple in PLACE_FIELDS order per read, counters)."""
    n = len(lens)
    st = dict.fromkeys(PLACE_COUNTERS, 0)
    st["n_rows"] = len(rows)
    best = {}                                                 # query -> (key, row index, geometry)
    for k, row in enumerate(rows):
        g = geometry(row, lens, table)
        if g == "not_placed":
            st["n_target_not_placed"] += 1
        elif g == "outside":
            st["n_outside"] += 1
        else:
            st["n_eligible"] += 1
            q, key = int(row["query"]), place_key(row, k)
            if q not in best or key > best[q][0]:
                best[q] = (key, k, g)
    out = []
    for r in range(n):
        if r not in best:
            out.append((r, 0, 0, -1, 0, 0, 0, 0))
            continue
        _, k, g = best[r]
        out.append((r, 1, k) + g)
        st["n_found"] += 1
        st[{PLACED: "n_found_placed", CONTAINED: "n_found_contained", UNPLACED: "n_found_unplaced"}[table[r][1]]] += 1
    return out, st


def place_pair(p, contig_len, read_len, R=R):
    """pba_place_row_pair by hand: (a_seq, a_pos, a_len, b_seq, b_pos, b_len, flags) of a found placement."""
    read, _, _, contig, pos, d, _, j = p
    b_len = read_len - j if d == 1 else j + 1
    rem = contig_len - pos if d == 1 else pos + 1
    return (contig, pos, min(rem, b_len + 1 + int(b_len * R)), read, j, b_len, 0 if d == 1 else 3)


def pair_texts(pair, contig, read, strand):
    """(a, b, fwd): the elements of the two accessors in memory order (a backward accessor starts at its last byte), b from
    rc(read) for strand -1."""
    _, ap, al, _, bp, bl, flags = (int(x) for x in pair)
    Q = read if strand == 1 else rc(read)
    if flags == 0:
        return contig[ap:ap + al], Q[bp:bp + bl], True
    return contig[ap - al + 1:ap + 1], Q[bp - bl + 1:bp + 1], False


def accessors_agree(p, contig, read):
    """The elements of an exact placement's two accessors, in walking order, over the shorter one: (a, b), both non-empty."""
    _, _, _, _, pos, d, strand, j = p
    Q = read if strand == 1 else rc(read)
    a, b = (contig[pos:], Q[j:]) if d == 1 else (contig[:pos + 1][::-1], Q[:j + 1][::-1])
    m = min(len(a), len(b))
    return a[:m], b[:m]


# ----------------------------------------------------------------------------- tilings and fuzz (CPU and GPU tests)
def place_tilings(seed):
    """Three error-free tilings of 2 .. 39 reads of 40 .. 199 bases, steps 1 .. 59, min_ov 1 .. 29, as one set with shuffled
    ids and rows, dir drawn +1 / -1 per row (an exact row is the same row in either direction).  Returns (texts, rows)."""
    rng = np.random.default_rng(seed)
    tilings = []
    for _ in range(3):
        n = int(rng.integers(2, 40))
        tilings.append(tiling(rng, rng.integers(40, 200, n), rng.integers(1, 60, n - 1), min_ov=int(rng.integers(1, 30))))
    texts, rows, _ = combine(rng, tilings)
    rows["dir"] = rng.choice((1, -1), rows.size)
    return texts, rows


def fuzz_rows(rng, lens, n_rows, targets=None):
    """Random valid rows that have nothing to do with real overlaps: costs beyond both clamps among them.  targets: the reads
    the targets are drawn from (all of them by default)."""
    n, tup = len(lens), []
    for _ in range(n_rows):
        t = int(rng.integers(0, n)) if targets is None else int(rng.choice(targets))
        q = int((t + rng.integers(1, n)) % n)
        tb, te = sorted(rng.choice(int(lens[t]) + 1, 2, replace=False))
        qb, qe = sorted(rng.choice(int(lens[q]) + 1, 2, replace=False))
        cost = int(rng.choice((rng.integers(0, 40), -3, 65535, 70000, 65534)))
        tup.append((t, q, int(rng.choice((1, -1))), cost, int(tb), int(te), int(qb), int(qe), int(rng.choice((1, -1)))))
    return make_place_rows(tup)


# ----------------------------------------------------------------------------- hand-computed cases
# The layout under all of them, HAND_LENS with HAND_LAY_ROWS at hang 64, min_reads 2 (layout_ref.HAND_CASES:
# three_reads_middle_reversed, plus a contained read and two reads without rows):
#   read 0  PLACED  contig 0 rank 0 orient 0 offset   0 skip  0 adv 100      contig 0 = r0 + rc(r1)[60:] + r2[50:], 190 bases
#   read 1  PLACED  contig 0 rank 1 orient 1 offset 100 skip 60 adv  40
#   read 2  PLACED  contig 0 rank 2 orient 0 offset 140 skip 50 adv  50
#   read 3  CONTAINED in read 0 (50 bases)        reads 4, 5  UNPLACED (100 and 80 bases)
HAND_LENS = [100, 100, 100, 50, 100, 80]
HAND_LAY_ROWS = [(0, 1, -1, 0, 40, 100, 40, 100), (1, 2, -1, 0, 0, 50, 0, 50), (3, 0, 1, 0, 0, 50, 10, 60)]
_U = (UNPLACED, -1, 0, 0, 0, 0, 0, -1)
HAND_TABLE = [(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1, PLACED, 0, 1, 1, 100, 60, 40, -1), (2, PLACED, 0, 2, 0, 140, 50, 50, -1),
              (3, CONTAINED, -1, 0, 0, 0, 0, 0, 0), (4,) + _U, (5,) + _U]


def _nf(*reads):
    return {r: (r, 0, 0, -1, 0, 0, 0, 0) for r in reads}


def _st(n_rows, **kw):
    st = dict.fromkeys(PLACE_COUNTERS, 0)
    st["n_rows"] = n_rows
    st.update(kw)
    return st


# rows: (target, query, strand, cost, t_beg, t_end, q_beg, q_end, dir); found: {read: its placement}, every other read _nf
HAND_PLACE = [
    dict(name="span_then_cost_then_lower_row_index",
         rows=[(0, 4, 1, 7, 30, 80, 0, 50, 1), (0, 4, 1, 7, 20, 80, 5, 65, 1), (0, 4, 1, 7, 10, 70, 0, 60, 1), (0, 4, 1, 9, 0, 60, 40, 100, 1)],
         # spans of q: 50, 60, 60, 60; cost 7 beats 9; rows 1 and 2 tie on (60, 7): row 1.  Its anchor: t_beg 20 of read 0
         # (orient 0, skip 0): pos = 0 + 20 - 0; the read runs forward from q_beg 5
         found={4: (4, 1, 1, 0, 20, 1, 1, 5)}, stats=_st(4, n_eligible=4, n_found=1, n_found_unplaced=1)),
    dict(name="cost_clamped_at_65535_and_at_0",
         rows=[(0, 4, 1, 70000, 10, 70, 0, 60, 1), (0, 4, 1, 65535, 20, 80, 0, 60, 1), (0, 5, 1, 0, 10, 70, 0, 60, 1), (0, 5, 1, -5, 20, 80, 0, 60, 1)],
         # 70 000 counts as 65 535: rows 0 and 1 tie, row 0 wins (unclamped it would lose).  -5 counts as 0: rows 2 and 3 tie,
         # row 2 wins (unclamped row 3 would)
         found={4: (4, 1, 0, 0, 10, 1, 1, 0), 5: (5, 1, 2, 0, 10, 1, 1, 0)}, stats=_st(4, n_eligible=4, n_found=2, n_found_unplaced=2)),
    dict(name="anchor_edges_orient_0",
         rows=[(2, 3, 1, 0, 49, 90, 0, 41, 1), (2, 4, 1, 0, 50, 90, 3, 43, 1), (2, 5, -1, 0, 60, 100, 10, 50, -1)],
         # read 2 supplies its bases [50, 100).  Row 0: anchor t_beg 49 = skip - 1: outside.  Row 1: anchor 50 = skip:
         # pos = 140 + 50 - 50.  Row 2, backward: anchor t_end - 1 = 99 = skip + adv - 1: pos = 140 + 99 - 50 = 189, the
         # contig's last base; walked rc(read 5) [80 - 50, 80 - 10) = [30, 70): j = qe - 1 = 69, running backward
         found={4: (4, 1, 1, 0, 140, 1, 1, 3), 5: (5, 1, 2, 0, 189, -1, -1, 69)},
         stats=_st(3, n_outside=1, n_eligible=2, n_found=2, n_found_unplaced=2)),
    dict(name="anchor_edges_orient_1",
         rows=[(1, 3, 1, 0, 10, 41, 0, 31, -1), (1, 4, 1, 0, 10, 40, 60, 90, -1), (1, 5, -1, 0, 0, 30, 20, 50, 1)],
         # the contig holds rc(read 1)[60, 100) at 100.  Row 0, backward: anchor t_end - 1 = 40, in rc(t) 99 - 40 = 59 =
         # skip - 1: outside.  Row 1, backward: anchor 39 -> 60 = skip: pos = 100; dir' = +1, strand' = -1, j' = 100 - 1 - 89
         # (yb = q_end - 1 = 89).  Row 2, forward: anchor t_beg 0 -> 99 = skip + adv - 1: pos = 100 + 99 - 60 = 139; walked
         # rc(read 5) [80 - 50, 80 - 20) = [30, 60): yb = 30, j' = 80 - 1 - 30 = 49 in the read as given, running backward
         found={4: (4, 1, 1, 0, 100, 1, -1, 10), 5: (5, 1, 2, 0, 139, -1, 1, 49)},
         stats=_st(3, n_outside=1, n_eligible=2, n_found=2, n_found_unplaced=2)),
    dict(name="target_contained_or_unplaced_and_queries_of_every_state",
         rows=[(3, 5, 1, 0, 0, 40, 0, 40, 1), (4, 5, 1, 0, 0, 40, 0, 40, 1), (0, 3, 1, 0, 10, 60, 0, 50, 1), (0, 1, -1, 0, 40, 100, 40, 100, 1),
               (2, 1, 1, 0, 0, 40, 0, 40, 1)],
         # rows 0 and 1: the target is CONTAINED / UNPLACED, read 5 finds nothing.  Row 2: the contained read 3 at
         # pos 10.  Row 3: the PLACED read 1 by the row that joined it: anchor 40 of read 0, walked rc(read 1) from
         # 100 - 100 = 0.  Row 4: read 2's base 0 is not one it supplies (skip 50): outside
         found={3: (3, 1, 2, 0, 10, 1, 1, 0), 1: (1, 1, 3, 0, 40, 1, -1, 0)},
         stats=_st(5, n_target_not_placed=2, n_outside=1, n_eligible=2, n_found=2, n_found_placed=1, n_found_contained=1)),
    dict(name="no_rows", rows=[], found={}, stats=_st(0)),
]


def hand_placements(case):
    return [case["found"].get(r, _nf(r)[r]) for r in range(len(HAND_LENS))]


def hand_texts(seed=0):
    rng = np.random.default_rng(2000 + seed)
    return [rng.choice(ACGT, n).tobytes() for n in HAND_LENS]


# ----------------------------------------------------------------------------- the vote, composed from the oracle
def oracle_vote_placed(oracle, contigs, reads, places, c, weight=1, R=R, overlap_min=OVERLAP_MIN):
    """Contig c as ref_seq(T, weight) with every found placement on it through align + try_align's gate + elect, no growth.
    places: records or tuples in PLACE_FIELDS order.  Returns (consensus object, {index: align result}, placements voted)."""
    cons = oracle.consensus(contigs[c], weight)
    res, voted = {}, 0
    for k, p in enumerate(places):
        p = tuple(int(x) for x in p)
        if not p[1] or p[3] != c:
            continue
        pr = place_pair(p, len(contigs[c]), len(reads[p[0]]), R)
        a, b, fwd = pair_texts(pr, contigs[c], reads[p[0]], p[6])
        out = oracle.align(a, b, R, a_fwd=fwd, b_fwd=fwd, want_ops=True)
        res[k] = out
        if out["rc"] >= 0 and out["matlen_a"] >= overlap_min:
            cons.elect(pr[1], fwd, out["ops"], eng.script_vals(out["ops"], b, fwd))
            voted += 1
    return cons, res, voted


def oracle_boxes(cons, n):
    sel, sup, tot, _ = cons.dump(n + 8)
    return sel, sup, tot


def oracle_evolve(cons, n) -> bytes:
    cons.evolve()
    return cons.text(2 * n + 8)


def oracle_consensus(oracle, contigs, reads, places, weight=1, R=R, overlap_min=OVERLAP_MIN):
    """(next contigs, placements voted per contig): one round of vote and evolve over every contig."""
    out, voted = [], []
    for c, T in enumerate(contigs):
        if len(T) == 0:
            out.append(b""); voted.append(0)
            continue
        cons, _, v = oracle_vote_placed(oracle, contigs, reads, places, c, weight, R, overlap_min)
        out.append(oracle_evolve(cons, len(T))); voted.append(v)
    return out, voted


def check_result(got, exp, tag):
    assert int(got["rc"]) == exp["rc"], (tag, int(got["rc"]), exp)
    for k in ("len_a", "len_b", "max_dst"):
        assert int(got[k]) == exp[k], (tag, k)
    if exp["rc"] >= 0:
        for k in ("cost", "matlen_a", "matlen_b"):
            assert int(got[k]) == exp[k], (tag, k, int(got[k]), exp)


# ----------------------------------------------------------------------------- inputs of the vote tests
NOISY_SEED = 811


def noisy_reads(seed, n=200, glen=24000, err=0.12):
    """n reads of 600 - 1 500 bases of a synthetic genome at `err` error (a third each of insertions, deletions and
    substitutions), every second one (by a seeded draw) reverse-complemented."""
    g = eng.synth_genome(seed, glen)
    reads, offs, _ = eng.synth_reads(seed + 1, g, n, 1500, err / 3, err / 3, err / 3)
    rng = np.random.default_rng(seed + 2)
    texts = [reads[int(offs[i]):int(offs[i + 1])].tobytes()[:int(rng.integers(600, 1501))] for i in range(n)]
    flip = rng.integers(0, 2, n).astype(bool)
    return [rc(x) if f else x for x, f in zip(texts, flip)]


def noisy_conditions(oracle, texts, rows, hang=64, min_reads=2):
    """What tests/test_gpu_place.py requires of its noisy input, from the layout and placement references and the oracle's
    aligner alone: voting placements per (dir', strand'), voting CONTAINED reads, found placements that fail the gate."""
    lens = [len(x) for x in texts]
    lay = layout_ref(lens, rows, hang, min_reads, texts)
    places, st = place_ref(lens, lay["table"], rows)
    out = {"contigs": [(c[1], c[2]) for c in lay["contigs"]], "found": st["n_found"], "voted": {(d, s): 0 for d in (1, -1) for s in (1, -1)},
           "voted_contained": 0, "found_not_voted": 0}
    for c in range(len(lay["texts"])):
        _, res, _ = oracle_vote_placed(oracle, lay["texts"], texts, places, c)
        for k, o in res.items():
            if o["rc"] >= 0 and o["matlen_a"] >= OVERLAP_MIN:
                out["voted"][(places[k][5], places[k][6])] += 1
                out["voted_contained"] += lay["table"][k][1] == CONTAINED
            else:
                out["found_not_voted"] += 1
    return out, lay, places, st


EDGE_LEN = 70001
# (anchor pos on the contig, dir, strand, read length, anchor index j in the text b reads): exact copies of the contig
EDGE_PLACES = [
    (4095, 1, 1, 900, 0), (4096, 1, -1, 900, 0), (8191, 1, 1, 700, 50),          # forward from a tile's last / first box
    (4095, -1, 1, 900, 899), (4096, -1, -1, 900, 899), (8191, -1, 1, 700, 649),   # backward from them
    (66000, 1, 1, 1200, 0), (66500, 1, -1, 800, 10), (69000, -1, 1, 1000, 999), (67000, -1, -1, 650, 600),   # pos > 65 535
    (300, -1, 1, 900, 899), (120, -1, -1, 700, 650),                              # backward, off base 0
    (69500, 1, 1, 900, 0), (69801, 1, -1, 700, 20),                               # forward, off the last base
    (70000 - 40, 1, 1, 600, 0), (40, -1, 1, 600, 599),                            # 41 bases of the contig left: fails the gate
]


def edge_case(seed=821):
    """(contig of 70 001 bases, reads, placement tuples): every read is an exact copy of the contig around its anchor --
    read text b with b[j] on contig base pos, running in direction dir, random text where it hangs over an end of the contig
    -- given reverse-complemented where strand is -1 (b is then rc of the read as given)."""
    rng = np.random.default_rng(seed)
    T = rng.choice(ACGT, EDGE_LEN).tobytes()
    reads, places = [], []
    for r, (pos, d, strand, L, j) in enumerate(EDGE_PLACES):
        # b[i] lies on contig base pos + (i - j): b is forward contig text either way; only the walking direction differs
        lo = pos - j
        b = bytearray(rng.choice(ACGT, L).tobytes())
        for i in range(L):
            if 0 <= lo + i < EDGE_LEN:
                b[i] = T[lo + i]
        b = bytes(b)
        reads.append(b if strand == 1 else rc(b))
        places.append((r, 1, r, 0, pos, d, strand, j))
    return T, reads, places


if __name__ == "__main__":
    import sys
    from correct_helpers import oracle_rows
    from oraclelib import Oracle
    orc = Oracle()
    mask = eng.mask_from_pattern("111*11*11*1*1111")
    for seed in [int(x) for x in sys.argv[1:]] or [NOISY_SEED]:
        texts = noisy_reads(seed)
        cond, _, _, st = noisy_conditions(orc, texts, oracle_rows(orc, texts, mask))
        print(seed, cond, st)
