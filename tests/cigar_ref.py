"""Run-length alignments (CIGAR over = X I D) and PAF as plain Python, independent of the engine: the runs of an edit script
and the two accessors' elements under both flags, the counts, the string, the bound on the runs of a success, the pair the
mapper aligned for a row, the rows-level layout (offsets, whole rows under a cap) and the PAF formatters.  Also the planted
inputs tests/test_gpu_cigar.py uses, so that tests/test_cigar_cpu.py can prove their script shapes from the oracle alone.

A script is the reference's: 1 MATCH (a and b advance), 2 INSERT (b advances), 3 DELETE (a advances), origin-first.  A run
is len << 4 | op with BAM's numbering.  By default a is the query: DELETE is I, INSERT is D."""
import numpy as np

INS, DEL, EQ, X = 1, 2, 7, 8
REVERSED, B_IS_QUERY = 1, 2
OPCH = {INS: "I", DEL: "D", EQ: "=", X: "X"}
ALPHA = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(x: bytes) -> bytes:
    return x.translate(_COMP)[::-1]


def codes(ops, a: bytes, b: bytes, flags: int = 0):
    """one code per op, origin-first"""
    out, i, j = [], 0, 0
    for op in ops:
        op = int(op)
        if op == 1:
            out.append(EQ if a[i] == b[j] else X)
            i += 1
            j += 1
        elif op == 2:
            out.append(INS if flags & B_IS_QUERY else DEL)
            j += 1
        else:
            assert op == 3, op
            out.append(DEL if flags & B_IS_QUERY else INS)
            i += 1
    return out


def runs(ops, a: bytes, b: bytes, flags: int = 0):
    """(list of run words, counts dict)"""
    cs = codes(ops, a, b, flags)
    out = []
    for c in cs:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    words = [(n << 4) | c for c, n in out]
    if flags & REVERSED:
        words.reverse()
    counts = dict(n_eq=cs.count(EQ), n_x=cs.count(X), n_ins=cs.count(INS), n_del=cs.count(DEL))
    return words, counts


def string(words) -> str:
    return "".join(f"{int(w) >> 4}{OPCH[int(w) & 15]}" for w in words)


def clip(la: int, lb: int, R: float):
    """(len_a, len_b, max_dst) of seq_aligner.h:94-102"""
    if lb >= la:
        md = 1 + int(la * R)
        return la, min(lb, la + md), md
    md = 1 + int(lb * R)
    return min(la, lb + md), lb, md


def bound(la: int, lb: int, R: float) -> int:
    ca, cb, md = clip(la, lb, R)
    return 2 * md - 1 if min(ca, cb) > 10 else ca + cb


def identities(counts, res, flags: int = 0):
    """the three identities a successful pair's counts obey"""
    qi, qd = ("n_del", "n_ins") if flags & B_IS_QUERY else ("n_ins", "n_del")
    return (counts["n_eq"] + counts["n_x"] + counts[qi] == res["matlen_a"] and
            counts["n_eq"] + counts["n_x"] + counts[qd] == res["matlen_b"] and
            counts["n_x"] + counts["n_ins"] + counts["n_del"] == res["cost"])


def map_row_aln_pair(row, contig_len: int, read_len: int, R: float):
    """(a_seq, a_pos, a_len, b_seq, b_pos, b_len, flags): a = the read from j, b = the contig from pos, clipped as align does"""
    ca, cb, _ = clip(read_len - int(row["j"]), contig_len - int(row["pos"]), R)
    return int(row["read"]), int(row["j"]), ca, int(row["contig"]), int(row["pos"]), cb, 0


def layout(row_runs, cap=None):
    """rows-level output: (offsets, total, dense list with the rows that fit whole, in order, up to the first that does not)"""
    off = [0]
    for r in row_runs:
        off.append(off[-1] + len(r))
    dense, fits = [], True
    for k, r in enumerate(row_runs):
        fits = fits and (cap is None or off[k + 1] <= cap)
        if fits:
            dense.extend(r)
    return off, off[-1], dense


def _paf(qname, qlen, qbeg, qend, strand, tname, tlen, tbeg, tend, c, nm, words):
    block = c["n_eq"] + c["n_x"] + c["n_ins"] + c["n_del"]
    cols = [qname, qlen, qbeg, qend, "+" if strand == 1 else "-", tname, tlen, tbeg, tend, c["n_eq"], block, 255, f"NM:i:{nm}",
            "cg:Z:" + string(words)]
    return "\t".join(str(x) for x in cols)


def paf_map_lines(rows, counts, cigars, read_lens, contig_lens, read_names=None, contig_names=None):
    out = []
    for k, r in enumerate(rows):
        if not r["found"]:
            continue
        q, t = int(r["read"]), int(r["contig"])
        out.append(_paf(read_names[q] if read_names else f"read{q}", int(read_lens[q]), int(r["r_beg"]), int(r["r_end"]), int(r["strand"]),
                        contig_names[t] if contig_names else f"contig{t}", int(contig_lens[t]), int(r["c_beg"]), int(r["c_end"]),
                        {n: int(counts[k][n]) for n in ("n_eq", "n_x", "n_ins", "n_del")}, int(r["cost"]), cigars[k]))
    return out


def paf_overlap_lines(rows, counts, cigars, read_lens, read_names=None):
    name = (lambda i: read_names[i]) if read_names else (lambda i: f"read{i}")
    return [_paf(name(int(r["query"])), int(read_lens[int(r["query"])]), int(r["q_beg"]), int(r["q_end"]), int(r["strand"]),
                 name(int(r["target"])), int(read_lens[int(r["target"])]), int(r["t_beg"]), int(r["t_end"]),
                 {n: int(counts[k][n]) for n in ("n_eq", "n_x", "n_ins", "n_del")}, int(r["cost"]), cigars[k])
            for k, r in enumerate(rows)]


# ----------------------------------------------------------------------------- planted inputs: the sink's group edges
PLANT_R = 0.30
GROUP_EDGES = (1, 63, 64, 65, 127, 128, 129)      # a planted edit as the k-th op from the goal
TOTAL_OPS = (1, 2, 63, 64, 65, 128, 129)          # pairs with that many ops in all


def _other(ch: int) -> int:
    return b"ACGT"[(b"ACGT".index(ch) + 1) % 4]


def _seq(rng, n: int) -> bytes:
    """random, but no base equals its neighbour: an inserted or deleted base cannot slide along a homopolymer, and the
    reference's tie-break does not move a planted edit"""
    out = bytearray(ALPHA[rng.integers(0, 4, 1)].tobytes()) if n else bytearray()
    while len(out) < n:
        c = int(ALPHA[rng.integers(0, 4)])
        if c != out[-1]:
            out.append(c)
    return bytes(out)


def planted_pairs():
    """[(tag, a, b, expect)]: element strings of forward accessors; expect: what the CPU test proves of the oracle's script
    ({'n': ops in all}, {'edit': (kind, k)} = the only non-= op is of `kind` and is the k-th from the goal, ...)."""
    rng = np.random.default_rng(20260)
    out = []
    for n in (20, 150, 400):                                   # exact copies: one `=` run over several groups
        x = _seq(rng, n)
        out.append((f"copy{n}", x, x, dict(n=n, all_eq=True)))
    for n in TOTAL_OPS:                                        # pairs with n ops in all (exact copies of n bases)
        x = _seq(rng, n)
        out.append((f"ops{n}", x, x, dict(n=n, all_eq=True)))
    for k in GROUP_EDGES:                                      # one planted edit, the k-th op from the goal
        n = k + 70                                             # 71 .. 199 bases; the edit sits k - 1 bases before the end
        for kind in ("X", "I", "D") if k > 1 else ("any",):     # (at the goal itself the free end absorbs an indel: one pair,
            x = _seq(rng, n)                                   #  a changed last base, whatever single op the reference makes of it)
            p = n - k                                          # index of the edited base of x
            if kind in ("X", "any"):
                y = x[:p] + bytes([_other(x[p])]) + x[p + 1:]
            elif kind == "I":                                  # a has a base b lacks (the reference's DELETE)
                y = x[:p] + x[p + 1:]
            else:                                              # b has a base a lacks (the reference's INSERT)
                c = next(c for c in b"ACGT" if c != x[p] and c != x[p + 1])
                y = x[:p + 1] + bytes([c]) + x[p + 1:]
            out.append((f"{kind}@{k}", x, y, dict(edit=(kind, k))))
    for k in (64, 128):                                        # two different edits adjacent across a group edge
        n = k + 80
        x = _seq(rng, n)
        p = n - k                                              # op k from the goal is an X, op k + 1 an I
        y = x[:p - 1] + bytes([_other(x[p])]) + x[p + 1:]
        out.append((f"XI@{k}", x, y, dict(adjacent=k)))
    x = _seq(rng, 300)                                         # an X inside a long diagonal: put_run straddles it
    y = x[:150] + bytes([_other(x[150])]) + x[151:]
    out.append(("X-in-diagonal", x, y, dict(edit=("X", 150))))
    for m in (3, 5, 10):                                       # min(len) <= 10: the row-sweep corner
        x = _seq(rng, m)
        y = x[:m // 2] + bytes([_other(x[m // 2])]) + x[m // 2 + 1:] if m == 10 else x
        out.append((f"corner{m}", x, y + _seq(rng, 1), dict(corner=True)))
        out.append((f"corner{m}:swapped", y + _seq(rng, 1), x, dict(corner=True)))
    x = _seq(rng, 120)                                         # the path runs off into a border: row 0 / column 0
    c = bytes([_other(x[0])])                                  # (one base: two would fail the diagonal check at row 11)
    out.append(("border:b-leads", x, c + x, dict(border=2)))   # starts with an INSERT (row 0)
    out.append(("border:a-leads", c + x, x, dict(border=3)))   # starts with a DELETE (column 0)
    a, b = _seq(rng, 200), _seq(rng, 200)                      # unrelated: fails
    out.append(("fails", a, b, dict(fails=True)))
    out.append(("fails:short", a[:40], b[:44], dict(fails=True)))
    return out


def flags_batch():
    """[(a_text, a_back, b_text, b_back)]: forward, both-backward and len_a > len_b pairs with a few edits each; the texts are
    what lies in memory (a backward accessor starts at the last byte)"""
    rng = np.random.default_rng(20261)
    out = []
    for k in range(12):
        n = int(rng.integers(40, 300))
        x = _seq(rng, n)
        y = bytearray(x)
        for p in sorted(rng.choice(np.arange(5, n - 5), 3, replace=False).tolist(), reverse=True):
            t = k % 3 if p % 2 else (k + 1) % 3
            if t == 0:
                y[p] = _other(y[p])
            elif t == 1:
                del y[p]
            else:
                y.insert(p, _other(y[p]))
        y = bytes(y) + _seq(rng, int(rng.integers(0, 30)))
        a, b = (y, x) if k % 4 == 3 else (x, y)                # every fourth: a is the longer side
        back = k % 3 == 1
        out.append((a[::-1] if back else a, back, b[::-1] if back else b, back))
    return out
