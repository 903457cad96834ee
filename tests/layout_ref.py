"""Layout of reads into contigs from overlap rows (pba_layout_*), restated in plain Python: loops and dicts,
chains walked by following succ, no atomics and no pointer jumping.  The device must equal this exactly.

rows: records with the fields of pba_strand_overlap that the layout reads (target, query, strand, cost, t_beg, t_end,
q_beg, q_end); lens: the read lengths; texts (optional): the reads, to stitch the contigs."""
import numpy as np

UNPLACED, PLACED, CONTAINED = 0, 1, 2
ROW_FIELDS = ("read", "state", "contig", "rank", "orient", "offset", "skip", "adv", "container")
COUNTERS = ("n_rows", "n_internal", "n_contain", "n_contain_refused", "n_dovetail", "n_dovetail_dropped", "n_contained",
            "n_mated_ends", "n_cycles", "n_contigs", "n_placed", "n_unplaced", "n_bases")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(x: bytes) -> bytes:
    return x.translate(_COMP)[::-1]


def make_rows(tuples):
    """[(target, query, strand, cost, t_beg, t_end, q_beg, q_end)] -> records with every pba_strand_overlap field."""
    from pacbioassembly_amd.engine import STRAND_OVERLAP_DTYPE
    out = np.zeros(len(tuples), STRAND_OVERLAP_DTYPE)
    for k, (t, q, s, c, tb, te, qb, qe) in enumerate(tuples):
        out[k]["target"], out[k]["query"], out[k]["strand"], out[k]["cost"] = t, q, s, c
        out[k]["t_beg"], out[k]["t_end"], out[k]["q_beg"], out[k]["q_end"] = tb, te, qb, qe
        out[k]["matlen_a"], out[k]["matlen_b"], out[k]["dir"] = te - tb, qe - qb, 1
    return out


def classify(row, lens, hang):
    """("internal",) | ("refused",) | ("contain", inner, outer) | ("dovetail", end of t, end of q); end = 2 * read + side."""
    t, q, strand = int(row["target"]), int(row["query"]), int(row["strand"])
    lt, lq = int(lens[t]), int(lens[q])
    tb, te = int(row["t_beg"]), int(row["t_end"])
    if strand == 1:
        qb, qe = int(row["q_beg"]), int(row["q_end"])
    else:                                                     # the coordinates of the walked text rc(q)
        qb, qe = lq - int(row["q_end"]), lq - int(row["q_beg"])
    tl, tr, ql, qr = tb, lt - te, qb, lq - qe
    if min(tl, ql) > hang or min(tr, qr) > hang:
        return ("internal",)
    t_in_q, q_in_t = tl <= ql and tr <= qr, ql <= tl and qr <= tr
    if t_in_q or q_in_t:
        def rank(x):
            return (int(lens[x]), -x)
        if t_in_q and q_in_t:
            inner, outer = (t, q) if rank(t) < rank(q) else (q, t)
        elif t_in_q:
            inner, outer = t, q
        else:
            inner, outer = q, t
        return ("contain", inner, outer) if rank(outer) > rank(inner) else ("refused",)
    if tl > ql:                                               # t's last base side joins q's walked-left end
        return ("dovetail", 2 * t + 1, 2 * q + (0 if strand == 1 else 1))
    return ("dovetail", 2 * t, 2 * q + (1 if strand == 1 else 0))


def _key_cost(cost):
    return min(max(int(cost), 0), 0xFFFF)


def layout_ref(lens, rows, hang=64, min_reads=2, texts=None):
    n = len(lens)
    st = dict.fromkeys(COUNTERS, 0)
    st["n_rows"] = len(rows)
    # 1. classify; the container of a read is the outer read of its accepted row with the smallest index
    cls, container = [], {}
    for k, row in enumerate(rows):
        c = classify(row, lens, hang)
        cls.append(c)
        if c[0] == "internal":
            st["n_internal"] += 1
        elif c[0] == "refused":
            st["n_contain_refused"] += 1
        elif c[0] == "contain":
            st["n_contain"] += 1
            container.setdefault(c[1], c[2])
        else:
            st["n_dovetail"] += 1
    st["n_contained"] = len(container)
    # 2. best edge per end among the dovetails of two reads that are not contained
    best = {}                                                 # end -> (key, row index, other end)
    for k, (row, c) in enumerate(zip(rows, cls)):
        if c[0] != "dovetail":
            continue
        t, q = int(row["target"]), int(row["query"])
        if t in container or q in container:
            st["n_dovetail_dropped"] += 1
            continue
        span_q = int(row["q_end"]) - int(row["q_beg"])
        for end, other, span in ((c[1], c[2], int(row["t_end"]) - int(row["t_beg"])), (c[2], c[1], span_q)):
            key = (span, -_key_cost(row["cost"]), -k)
            if end not in best or key > best[end][0]:
                best[end] = (key, k, other)
    # 3. mates: the winners of both ends lead to each other
    mate = {}
    for e, (_, _, f) in best.items():
        if f in best and best[f][2] == e:
            mate[e] = f
    st["n_mated_ends"] = len(mate)

    free = [r for r in range(n) if r not in container]

    def walk_heads():
        """every path, once per direction: lists of states (2 * read + orient) from a head on"""
        paths, seen = [], set()
        for r in free:
            for s in (2 * r, 2 * r + 1):
                if s in mate:                                 # the entry end of state s is end s
                    continue
                p = [s]
                while (p[-1] ^ 1) in mate:                    # succ: the mate of the exit end, entered at that side
                    p.append(mate[p[-1] ^ 1])
                paths.append(p)
                seen.update(p)
        return paths, seen

    # 4. chains; states no head reaches lie on cycles: cut each at side 0 of its smallest read, from both sides
    paths, seen = walk_heads()
    cuts = set()
    for r in free:
        for s in (2 * r, 2 * r + 1):
            if s in seen:
                continue
            cyc = [s]
            while mate[cyc[-1] ^ 1] != s:
                cyc.append(mate[cyc[-1] ^ 1])
            seen.update(cyc)
            cuts.add(min(x >> 1 for x in cyc))
    st["n_cycles"] = len(cuts)
    for m in cuts:
        f = mate.pop(2 * m)
        del mate[f]
    if cuts:
        paths, _ = walk_heads()

    def geom(s):
        """(skip, adv) of state s: from the winning row at the exit end of its predecessor"""
        r, L = s >> 1, int(lens[s >> 1])
        if s not in mate:
            return 0, L
        row = rows[best[mate[s]][1]]
        b, e = (int(row["t_beg"]), int(row["t_end"])) if int(row["target"]) == r else (int(row["q_beg"]), int(row["q_end"]))
        skip = e if (s & 1) == 0 else L - b
        return skip, max(L - skip, 0)

    # 5. canonical chains of at least min_reads reads, numbered by ascending head read
    canon = [p for p in paths if (p[0] >> 1) < ((p[-1] ^ 1) >> 1) or (len(p) == 1 and (p[0] & 1) == 0)]
    canon.sort(key=lambda p: p[0] >> 1)
    table = {r: dict(read=r, state=UNPLACED, contig=-1, rank=0, orient=0, offset=0, skip=0, adv=0, container=-1) for r in range(n)}
    for r, o in container.items():
        table[r]["state"], table[r]["container"] = CONTAINED, o
    contigs, out_texts = [], []
    for p in canon:
        if len(p) < min_reads:
            continue
        cid, off, parts = len(contigs), 0, []
        for k, s in enumerate(p):
            skip, adv = geom(s)
            table[s >> 1].update(state=PLACED, contig=cid, rank=k, orient=s & 1, offset=off, skip=skip, adv=adv)
            if texts is not None:
                x = texts[s >> 1] if (s & 1) == 0 else rc(texts[s >> 1])
                parts.append(x[skip:skip + adv])
            off += adv
        contigs.append((p[0] >> 1, len(p), off))
        out_texts.append(b"".join(parts))
        st["n_placed"] += len(p)
        st["n_bases"] += off
    st["n_contigs"] = len(contigs)
    st["n_unplaced"] = n - st["n_placed"] - st["n_contained"]
    rows_out = [tuple(table[r][f] for f in ROW_FIELDS) for r in range(n)]
    return dict(table=rows_out, contigs=contigs, stats=st, texts=out_texts if texts is not None else None)


# ----------------------------------------------------------------------------- synthetic tilings (shared by the CPU and GPU tests)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def tiling(rng, read_lens, steps, flips=None, min_ov=1):
    """Error-free reads tiling a random genome: read k starts steps[k - 1] bases after read k - 1 (len(steps) = reads - 1),
    flips[k] != 0: its text is the reverse complement.  Returns (genome, starts, flips, texts, rows) with the exact cost-0
    row of every pair overlapping by at least min_ov bases, in both the (t, q) and the (q, t) view, ids = tiling order."""
    n = len(read_lens)
    starts = np.concatenate([[0], np.cumsum(steps)]).astype(int)[:n]
    flips = rng.integers(0, 2, n) if flips is None else np.asarray(flips)
    genome = rng.choice(ACGT, int(max(s + l for s, l in zip(starts, read_lens)))).tobytes()
    texts = [genome[s:s + l] for s, l in zip(starts, read_lens)]
    texts = [rc(x) if f else x for x, f in zip(texts, flips)]

    def fwd(k, lo, hi):                                       # genome [lo, hi) on the forward strand of read k
        a, L = int(starts[k]), int(read_lens[k])
        return (a + L - hi, a + L - lo) if flips[k] else (lo - a, hi - a)

    rows = []
    for t in range(n):
        for q in range(t + 1, n):
            lo, hi = max(starts[t], starts[q]), min(starts[t] + read_lens[t], starts[q] + read_lens[q])
            if starts[q] >= starts[t] + read_lens[t] and read_lens[q] > 0:
                break                                         # (starts ascend: no later read reaches back)
            if hi - lo < min_ov:
                continue
            strand = 1 if flips[t] == flips[q] else -1
            rows.append((t, q, strand, 0) + fwd(t, lo, hi) + fwd(q, lo, hi))
            rows.append((q, t, strand, 0) + fwd(q, lo, hi) + fwd(t, lo, hi))
    return genome, starts, flips, texts, rows


def combine(rng, tilings):
    """Several tilings as one read set with shuffled ids and shuffled rows.  Returns (texts, rows as records, ids: for every
    tiling the new id of each of its reads)."""
    n = sum(len(t[3]) for t in tilings)
    perm = rng.permutation(n)
    texts, rows, ids, base = [None] * n, [], [], 0
    for _, _, _, tx, rw in tilings:
        new = perm[base:base + len(tx)]
        ids.append(new)
        for k, x in enumerate(tx):
            texts[int(new[k])] = x
        rows += [(int(new[r[0]]), int(new[r[1]])) + tuple(int(v) for v in r[2:]) for r in rw]
        base += len(tx)
    order = rng.permutation(len(rows))
    return texts, make_rows([rows[int(k)] for k in order]), ids


# ----------------------------------------------------------------------------- hand-computed cases
# Reads of 100 bases unless said.  "A runs into B" below is the row (A, B, +1, cost, 40, 100, 0, 60): A's last 60 bases are
# B's first 60, so A's side 1 (end 2A + 1) joins B's side 0 (end 2B), and B supplies its bases from 60 on (skip 60, adv 40).
def _into(a, b, cost=0):
    return (a, b, 1, cost, 40, 100, 0, 60)


def _st(n_rows, **kw):
    st = dict.fromkeys(COUNTERS, 0)
    st["n_rows"] = n_rows
    st.update(kw)
    return st


_U = (UNPLACED, -1, 0, 0, 0, 0, 0, -1)                        # the columns after `read` of a read that is not placed
HAND_CASES = [
    # the four dovetail orientations as 2-read chains
    dict(name="dovetail_t_right_plus", lens=[100, 100], rows=[(0, 1, 1, 0, 40, 100, 0, 60)], hang=64, min_reads=2,
         # tl 40 > ql 0: ends 1 and 2 mate; states (0, 0) -> (1, 0); read 1 enters at side 0: skip = q_end = 60
         table=[(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1, PLACED, 0, 1, 0, 100, 60, 40, -1)], contigs=[(0, 2, 140)],
         stats=_st(1, n_dovetail=1, n_mated_ends=2, n_contigs=1, n_placed=2, n_bases=140)),
    dict(name="dovetail_t_left_plus", lens=[100, 100], rows=[(0, 1, 1, 0, 0, 60, 40, 100)], hang=64, min_reads=2,
         # tl 0 < ql 40: ends 0 and 3 mate; the path read 1 -> read 0 is walked from the smaller head, read 0, backwards:
         # states (0, 1) -> (1, 1); read 1 enters at side 1: skip = len - q_beg = 60
         table=[(0, PLACED, 0, 0, 1, 0, 0, 100, -1), (1, PLACED, 0, 1, 1, 100, 60, 40, -1)], contigs=[(0, 2, 140)],
         stats=_st(1, n_dovetail=1, n_mated_ends=2, n_contigs=1, n_placed=2, n_bases=140)),
    dict(name="dovetail_t_right_minus", lens=[100, 100], rows=[(0, 1, -1, 0, 40, 100, 40, 100)], hang=64, min_reads=2,
         # walked rc(q): [0, 60); tl 40 > ql 0: t's side 1 joins q's side 1 (ends 1 and 3); (0, 0) -> (1, 1), skip = 100 - 40
         table=[(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1, PLACED, 0, 1, 1, 100, 60, 40, -1)], contigs=[(0, 2, 140)],
         stats=_st(1, n_dovetail=1, n_mated_ends=2, n_contigs=1, n_placed=2, n_bases=140)),
    dict(name="dovetail_t_left_minus", lens=[100, 100], rows=[(0, 1, -1, 0, 0, 60, 0, 60)], hang=64, min_reads=2,
         # walked rc(q): [40, 100); tl 0 < ql 40: t's side 0 joins q's side 0 (ends 0 and 2); (0, 1) -> (1, 0), skip = q_end = 60
         table=[(0, PLACED, 0, 0, 1, 0, 0, 100, -1), (1, PLACED, 0, 1, 0, 100, 60, 40, -1)], contigs=[(0, 2, 140)],
         stats=_st(1, n_dovetail=1, n_mated_ends=2, n_contigs=1, n_placed=2, n_bases=140)),
    dict(name="three_reads_middle_reversed", lens=[100, 100, 100],
         rows=[(0, 1, -1, 0, 40, 100, 40, 100), (1, 2, -1, 0, 0, 50, 0, 50)], hang=64, min_reads=2,
         # row 1: walked rc(read 2) [50, 100), tl 0 < ql 50: read 1's side 0 joins read 2's side 0 (ends 2 and 4);
         # (0, 0) -> (1, 1) -> (2, 0); read 2 enters at side 0: skip = q_end = 50
         table=[(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1, PLACED, 0, 1, 1, 100, 60, 40, -1), (2, PLACED, 0, 2, 0, 140, 50, 50, -1)],
         contigs=[(0, 3, 190)], stats=_st(2, n_dovetail=2, n_mated_ends=4, n_contigs=1, n_placed=3, n_bases=190)),
    dict(name="containment_equal_lengths_larger_id_goes", lens=[100, 100], rows=[(0, 1, 1, 0, 0, 100, 0, 100)], hang=64, min_reads=2,
         # both conditions hold; rank(1) = (100, -1) < rank(0) = (100, 0): read 1 is the inner read
         table=[(0,) + _U, (1, CONTAINED, -1, 0, 0, 0, 0, 0, 0)], contigs=[],
         stats=_st(1, n_contain=1, n_contained=1, n_unplaced=1)),
    dict(name="containment_refused", lens=[100, 80], rows=[(0, 1, 1, 0, 10, 100, 20, 80)], hang=64, min_reads=2,
         # tl 10 <= ql 20 and tr 0 <= qr 0: t inside q only, but rank(q) = (80, -1) < rank(t) = (100, 0)
         table=[(0,) + _U, (1,) + _U], contigs=[], stats=_st(1, n_contain_refused=1, n_unplaced=2)),
    dict(name="contained_read_drops_its_dovetails_first_row_names_the_container", lens=[100, 100, 50, 100],
         rows=[(2, 1, 1, 0, 0, 50, 10, 60), (2, 0, 1, 0, 0, 50, 30, 80), (3, 2, 1, 0, 80, 100, 0, 20), _into(0, 1)], hang=64, min_reads=2,
         # rows 0 and 1 both put read 2 inside a longer read: the container is row 0's; row 2 is a dovetail of read 2: dropped
         table=[(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1, PLACED, 0, 1, 0, 100, 60, 40, -1), (2, CONTAINED, -1, 0, 0, 0, 0, 0, 1), (3,) + _U],
         contigs=[(0, 2, 140)],
         stats=_st(4, n_contain=2, n_dovetail=2, n_dovetail_dropped=1, n_contained=1, n_mated_ends=2, n_contigs=1, n_placed=2,
                   n_unplaced=1, n_bases=140)),
    dict(name="ties_by_cost_then_row_index_and_no_mate_unless_mutual", lens=[100] * 4,
         rows=[_into(0, 1, 5), _into(0, 2, 3), _into(0, 3, 3)], hang=64, min_reads=2,
         # at end 1 all three span 60 bases: cost 3 beats 5, row 1 beats row 2; ends 2 and 6 lead to end 1, which leads to 4
         table=[(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1,) + _U, (2, PLACED, 0, 1, 0, 100, 60, 40, -1), (3,) + _U], contigs=[(0, 2, 140)],
         stats=_st(3, n_dovetail=3, n_mated_ends=2, n_contigs=1, n_placed=2, n_unplaced=2, n_bases=140)),
    dict(name="overhang_equal_to_hang_kept_one_more_internal", lens=[100] * 3,
         rows=[(0, 1, 1, 0, 40, 90, 10, 60), (0, 2, 1, 0, 40, 89, 11, 60)], hang=10, min_reads=2,
         # row 0: min(tl, ql) = min(tr, qr) = 10; row 1: 11.  Read 1 still supplies from its interval's end, 60, on
         table=[(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1, PLACED, 0, 1, 0, 100, 60, 40, -1), (2,) + _U], contigs=[(0, 2, 140)],
         stats=_st(2, n_internal=1, n_dovetail=1, n_mated_ends=2, n_contigs=1, n_placed=2, n_unplaced=1, n_bases=140)),
    dict(name="singleton_min_reads_1", lens=[30], rows=[], hang=64, min_reads=1,
         table=[(0, PLACED, 0, 0, 0, 0, 0, 30, -1)], contigs=[(0, 1, 30)], stats=_st(0, n_contigs=1, n_placed=1, n_bases=30)),
    dict(name="singleton_min_reads_2", lens=[30], rows=[], hang=64, min_reads=2,
         table=[(0,) + _U], contigs=[], stats=_st(0, n_unplaced=1)),
    dict(name="ring_of_five", lens=[100] * 5, rows=[_into(3, 1), _into(1, 4), _into(4, 0), _into(0, 2), _into(2, 3)], hang=64, min_reads=2,
         # every end is mated; the smallest read is 0: its side 0 (end 0, mated to end 9 of read 4) is cut; 0 -> 2 -> 3 -> 1 -> 4
         table=[(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1, PLACED, 0, 3, 0, 180, 60, 40, -1), (2, PLACED, 0, 1, 0, 100, 60, 40, -1),
                (3, PLACED, 0, 2, 0, 140, 60, 40, -1), (4, PLACED, 0, 4, 0, 220, 60, 40, -1)], contigs=[(0, 5, 260)],
         stats=_st(5, n_dovetail=5, n_mated_ends=10, n_cycles=1, n_contigs=1, n_placed=5, n_bases=260)),
    dict(name="ring_of_two", lens=[100] * 2, rows=[_into(0, 1), _into(1, 0)], hang=64, min_reads=2,
         # ends 1-2 and 3-0 are mated; end 0 is cut: 0 -> 1
         table=[(0, PLACED, 0, 0, 0, 0, 0, 100, -1), (1, PLACED, 0, 1, 0, 100, 60, 40, -1)], contigs=[(0, 2, 140)],
         stats=_st(2, n_dovetail=2, n_mated_ends=4, n_cycles=1, n_contigs=1, n_placed=2, n_bases=140)),
]


def hand_texts(case, seed=0):
    """Texts for a hand case (the rows are not real overlaps of them: the layout never looks at a base before stitch)."""
    rng = np.random.default_rng(1000 + seed)
    return [rng.choice(ACGT, n).tobytes() for n in case["lens"]]
