"""Hand-built inputs of tests/test_gpu_sites.py, made without a GPU so that tests/test_sites_cpu.py can hold them to their
conditions on the CPU oracle: pile-up states whose chosen boxes hold chosen counts (the scan), and overlap rows whose scripts
put sites at chosen ops of the walk (the allele sink)."""
import numpy as np

import sites_ref as sr
from correct_helpers import pair_texts, rc
from map_ref import mutate, rand_text
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PLACE_ROW_DTYPE, STRAND_OVERLAP_DTYPE

R = 0.30
STRICT = (4, 2, 250)            # 6 or 9 rows and the target: N = 7 or 10; 3 of them on the second allele
LOOSE = (1, 1, 0)               # any box with a second allele


def _sub(ch: int) -> int:
    return b"ACGT"[(sr.code(ch) + 1) % 4]


def _with_subs(text: bytes, at) -> bytes:
    t = bytearray(text)
    for p in at:
        t[p] = _sub(t[p])
    return bytes(t)


def _place_row(read: int, contig: int, pos: int, j: int = 0, dir: int = 1):
    """a placement (pba_place_row): base `pos` of the contig against base j of the read, onwards (dir +1) or backwards (-1)"""
    r = np.zeros(1, PLACE_ROW_DTYPE)[0]
    r["read"], r["found"], r["row"], r["contig"], r["pos"], r["dir"], r["strand"], r["j"] = read, 1, read, contig, pos, dir, 1, j
    return r


def place_texts(row, contigs, reads, R):
    """(pair, a, b, fwd) of a placement: the bytes of its two accessors in memory order (a backward accessor ends on its
    origin)"""
    T, Q = contigs[int(row["contig"])], reads[int(row["read"])]
    pr = eng.place_row_pair(row, len(T), len(Q), R)
    fwd = int(pr["flags"]) == 0
    ap, al, bp, bl = (int(pr[k]) for k in ("a_pos", "a_len", "b_pos", "b_len"))
    if fwd:
        return pr, T[ap:ap + al], Q[bp:bp + bl], True
    return pr, T[ap - al + 1:ap + 1], Q[bp - bl + 1:bp + 1], False


def oracle_place_vote(oracle, contigs, reads, rows, c, weight=1, R=R, overlap_min=64):
    """contig c as ref_seq(T, weight) with every placement of `rows` on it through align + gate + elect; (consensus, voted)"""
    cons, voted = oracle.consensus(contigs[c], weight), 0
    for r in rows:
        if int(r["contig"]) != c:
            continue
        pr, a, b, fwd = place_texts(r, contigs, reads, R)
        out = oracle.align(a, b, R, a_fwd=fwd, b_fwd=fwd, want_ops=True)
        if out["rc"] >= 0 and out["matlen_a"] >= overlap_min:
            cons.elect(int(pr["a_pos"]), fwd, out["ops"], eng.script_vals(out["ops"], b, fwd))
            voted += 1
    return cons, voted


# ----------------------------------------------------------------------------- the scan
# Six targets in one arena: 191, 129, 0, 193, 150 and 300 boxes, so that targets start at arena offsets 191 (63 mod 64), 320
# (64) and 513 (65) and bitmap words straddle them.  Every target with sites has three exact reads, three that carry a
# substitution at every site but the last box and are walked forwards from box 0, and three that carry one at the last box
# alone and are walked backwards from it (a mismatch at the far end of a walk is no MATCH: the path ends before it); target
# 0 also loses its base 100 in the forward three (a DEL allele), target 3 gains a T behind its base 100 in the three exact reads (a SUP
# site on a box that is a SEL site too).  Target 4 has reads and no site, target 2 is empty.
# Target 5 has ten reads with a substitution every ten bases, read k at 50 + k, 60 + k, ...: 200 consecutive boxes with one
# second allele each, sites under LOOSE alone.
SCAN_LENS = (191, 129, 0, 193, 150, 300)
SCAN_SUBS = {0: (0, 190), 1: (0, 1, 64, 128), 3: (0, 1, 100, 192)}
SCAN_DEL = (0, 100)             # (target, position)
SCAN_INS = (3, 100)
SCAN_RUN = (5, 50, 250)         # (target, first, one past the last) of the consecutive sites


def scan_case(seed=20):
    """(targets, reads, placements, {target: strict SEL positions}, {target: strict SUP positions})"""
    rng = np.random.default_rng(seed)
    targets = [bytearray(rand_text(rng, n)) for n in SCAN_LENS]
    for t, p in (SCAN_DEL, SCAN_INS):
        targets[t][p - 1:p + 3] = b"ACGT"
    targets = [bytes(t) for t in targets]
    reads, rows = [], []

    def add(t, text, back=False):
        rows.append(_place_row(len(reads), t, len(targets[t]) - 1, len(text) - 1, -1) if back else _place_row(len(reads), t, 0))
        reads.append(text)
    for t in (0, 1, 3, 4):
        T = targets[t]
        for k in range(6):
            x = T if k < 3 or t == 4 else _with_subs(T, SCAN_SUBS[t][:-1])
            if t == SCAN_DEL[0] and k >= 3:
                x = x[:SCAN_DEL[1]] + x[SCAN_DEL[1] + 1:]
            if t == SCAN_INS[0] and k < 3:
                x = x[:SCAN_INS[1] + 1] + b"T" + x[SCAN_INS[1] + 1:]
            add(t, x)
        for k in range(3 if t != 4 else 0):
            add(t, _with_subs(T, SCAN_SUBS[t][-1:]), back=True)
    t, lo, hi = SCAN_RUN
    for k in range(10):
        add(t, _with_subs(targets[t], range(lo + k, hi, 10)))
    sel = {t: sorted(set(SCAN_SUBS.get(t, ())) | ({SCAN_DEL[1]} if t == SCAN_DEL[0] else set())) for t in range(len(targets))}
    sup = {t: [SCAN_INS[1]] if t == SCAN_INS[0] else [] for t in range(len(targets))}
    return targets, reads, np.array(rows, PLACE_ROW_DTYPE), sel, sup


LONG_SITES = (4095, 4096, 65535, 65536)


def long_case(seed=21):
    """(contig of 70 001 bases, reads, placements): six reads of 300 bases over each pair of sites, three of them with both
    bases substituted"""
    rng = np.random.default_rng(seed)
    T = rand_text(rng, 70001)
    reads, rows = [], []
    for p in LONG_SITES[::2]:
        for k in range(6):
            s = p - 120 - 10 * k
            x = T[s:s + 300]
            rows.append(_place_row(len(reads), 0, s))
            reads.append(_with_subs(x, (p - s, p + 1 - s)) if k >= 3 else x)
    return T, reads, np.array(rows, PLACE_ROW_DTYPE)


# ----------------------------------------------------------------------------- the sink
# One set of sequences: every case has a target and a query of its own.  A row's cost and matlens are what a trace of its
# pair gives (fill_rows); the sites of its target are then chosen from its script (choose_sites).
SINK_CASES = ("edges", "ops63", "two", "copy", "del", "back", "minus", "back-minus", "nosite", "tiny")


def sink_case(seed=22):
    """(texts, rows without cost and matlens, tags)"""
    rng = np.random.default_rng(seed)
    texts, rows, tags = [], [], []

    def add(tag, T, seg, ref_pos, dir=1, strand=1, j=0):
        t = len(texts)
        texts.append(T)
        texts.append(seg if strand == 1 else rc(seg))
        r = np.zeros(1, STRAND_OVERLAP_DTYPE)[0]
        r["target"], r["query"], r["strand"], r["j"], r["dir"], r["ref_pos"] = t, t + 1, strand, j, dir, ref_pos
        rows.append(r)
        tags.append(tag)
    for tag in SINK_CASES:
        T = bytearray(rand_text(rng, 700 if tag != "tiny" else 60))
        if tag == "del":
            for p in (200, 263, 264, 330):
                T[p - 1:p + 3] = b"ACGT"
        T = bytes(T)
        if tag == "copy":
            add(tag, T, T[10:310], 10)
        elif tag == "del":
            seg = T[100:500]
            for p in (330, 264, 263, 200):
                seg = seg[:p - 100] + seg[p - 100 + 1:]
            add(tag, T, seg, 100)
        elif tag in ("back", "back-minus"):
            seg = mutate(rng, T[150:616], 0.06)                  # ends on the target's base 615 = ref_pos + 15
            add(tag, T, seg[:-20] + T[596:616], 600, dir=-1, strand=1 if tag == "back" else -1)
        elif tag == "tiny":
            add(tag, T, T[5:14], 5)                              # nine bases: the row-sweep corner of the traced pass
        else:
            add(tag, T, mutate(rng, T[40:560], 0.06, keep=20), 40, strand=-1 if tag == "minus" else 1)
    return texts, np.array(rows, STRAND_OVERLAP_DTYPE), tags


def row_pair(row, texts):
    """(pair, a elements, b elements, a_pos, a backward) of an overlap row, the elements in element order"""
    pr = eng.overlap_row_pair(row, len(texts[int(row["target"])]), len(texts[int(row["query"])]))
    a, b, fwd = pair_texts(pr, texts, int(row["strand"]))
    return pr, (a if fwd else a[::-1]), (b if fwd else b[::-1]), int(pr["a_pos"]), not fwd


def fill_rows(rows, results):
    """the rows with cost and matlens from the results of their pairs' traces"""
    rows = rows.copy()
    for k in ("cost", "matlen_a", "matlen_b"):
        rows[k] = [int(x[k]) for x in results]
    return rows


def consumed(ops):
    """the a-element every op consumes (-1 for an INSERT), origin-first"""
    out, i = [], 0
    for op in ops:
        out.append(-1 if int(op) == 2 else i)
        i += int(op) != 2
    return out


def choose_sites(tag, ops, a_pos, a_back, matlen_a, a_len_clipped, t_len):
    """the SEL positions of a case's target, ascending, from its row's script"""
    e = consumed(ops)
    from_goal = lambda k: e[len(e) - k] if len(e) >= k else -1      # the k-th op of the walk, counted from the goal (1 = the goal's)
    elems = set()
    if tag in ("edges", "back", "minus", "back-minus", "tiny"):
        elems |= {0, matlen_a - 1, matlen_a}                         # matlen_a: one past the covered span
    if tag in ("ops63", "back", "back-minus"):
        elems |= {from_goal(63), from_goal(64), from_goal(65)}
    if tag == "two":
        elems |= {from_goal(70), from_goal(100)}
    if tag == "copy":
        elems |= {from_goal(k) for k in range(65, 129)}              # the whole second group of 64 ops, none in the first
    if tag == "del":
        dels = [i for op, i in zip(ops, e) if int(op) == 3]
        elems |= set(dels) | {d + 1 for d in dels} | {d - 1 for d in dels}
    pos = set()
    for x in elems:
        if 0 <= x < a_len_clipped:
            p = a_pos - x if a_back else a_pos + x
            if 0 <= p < t_len:
                pos.add(p)
    return sorted(pos)


def site_list(texts, positions):
    """records for pba_sites_create: a SEL record at every position of positions[target], and a SUP record behind the first
    and the last SEL record of a target, so that a record's index is not its rank among the SEL sites"""
    out = []
    for t in sorted(positions):
        ps = positions[t]
        for p in ps:
            own = sr.code(texts[t][p])
            out.append((t, p, sr.SEL, own, own, (own + 1 + p % 4) % 5, 9, 6, 3))      # minor: any allele but own, DEL among them
            if p in (ps[0], ps[-1]):
                out.append((t, p, sr.SUP, own, own, (own + 2) % 4, 9, 0, 4))
    return np.array(out, sr.SITE) if out else np.zeros(0, sr.SITE)
