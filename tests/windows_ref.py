"""Per-window alignment counts and the trim rule of DESIGN §5.11 (include/pba.h: pba_windows_*, pba_*_rows_windows,
pba_overlap_rows_trim) restated in plain Python, independent of the engine -- the expectation the device is held to, exactly
(tests/test_gpu_windows.py), pinned by hand without a GPU (tests/test_windows_cpu.py) -- and the planted 6 % input both share.

A script is the reference's: 1 MATCH (a and b advance), 2 INSERT (b advances), 3 DELETE (a advances), origin-first.  The a
sequence carries a grid of W-base windows fixed on its own coordinates: a-element e lies at x(e) = a_pos + e (forward
accessor) or a_pos - e (backward), g(e) = x(e) // W, and the pair's local window index is w(e) = |g(e) - g(0)|.  A MATCH or
DELETE that consumes a-element e is counted in window w(e); an INSERT met after i a-elements were consumed in w(max(i-1, 0)).
A window is a dict of the four counts of cigar_ref (I / D exchanged under B_IS_QUERY); origin-first, goal-first under REVERSED."""
import numpy as np

import cigar_ref as cr
from cigar_ref import B_IS_QUERY, DEL, EQ, INS, REVERSED, X
from clip_ref import PLANTED, rc

CNT = ("n_eq", "n_x", "n_ins", "n_del")
_NAME = {EQ: "n_eq", X: "n_x", INS: "n_ins", DEL: "n_del"}
DROPPED, WHOLE, CUT = 0, 1, 2
SPAN_FIELDS = ("state", "n_win", "n_good", "n_runs", "w_beg", "w_end", "a0", "b0", "na", "nb", "cost")
ROW_FIELDS = ("state", "n_win", "n_good", "n_runs", "w_beg", "w_end", "t_beg", "t_end", "q_beg", "q_end", "cost")


def zero():
    return dict.fromkeys(CNT, 0)


def window_of(e: int, a_pos: int, a_back: bool, W: int) -> int:
    x = a_pos - e if a_back else a_pos + e
    assert x >= 0 and W >= 1
    return abs(x // W - a_pos // W)


def from_script(ops, a: bytes, b: bytes, a_pos: int, a_back: bool, W: int, flags: int = 0):
    """the windows of a script; a, b: the accessors' elements in element order.  An empty script has one empty window."""
    codes = cr.codes(ops, a, b, flags)
    out = [zero()]
    i = 0
    for op, c in zip(ops, codes):
        e = max(i - 1, 0) if int(op) == 2 else i
        w = window_of(e, a_pos, a_back, W)
        while len(out) <= w:
            out.append(zero())
        out[w][_NAME[c]] += 1
        i += int(op) != 2
    assert len(out) == window_of(max(i - 1, 0), a_pos, a_back, W) + 1
    return out[::-1] if flags & REVERSED else out


def from_runs(words, a_pos: int, a_back: bool, W: int, flags: int = 0):
    """the same from the runs of cigar_ref.runs(ops, a, b, flags): a second derivation, run by run and not op by op.  A run
    that consumes a is cut where the grid cuts it; a run that consumes b only lies whole in the window of the a-element before."""
    words = [int(w) for w in words]
    if flags & REVERSED:
        words = words[::-1]
    a_only = DEL if flags & B_IS_QUERY else INS              # the code of the reference's DELETE
    b_only = INS if flags & B_IS_QUERY else DEL
    out = [zero()]
    i = 0
    for word in words:
        n, c = word >> 4, word & 15
        if c == b_only:
            w = window_of(max(i - 1, 0), a_pos, a_back, W)
            while len(out) <= w:
                out.append(zero())
            out[w][_NAME[c]] += n
            continue
        assert c in (EQ, X, a_only)
        while n:
            w = window_of(i, a_pos, a_back, W)
            x = a_pos - i if a_back else a_pos + i
            room = (x % W + 1) if a_back else (W - x % W)    # a-elements from i to the end of its window
            take = min(n, room)
            while len(out) <= w:
                out.append(zero())
            out[w][_NAME[c]] += take
            i += take
            n -= take
    return out[::-1] if flags & REVERSED else out


def bound(a_pos: int, a_len: int, b_len: int, R: float, W: int, a_back: bool = False) -> int:
    """windows the clipped len_a touches"""
    la = cr.clip(a_len, b_len, R)[0]
    return window_of(max(la - 1, 0), a_pos, a_back, W) + 1


def total(wins):
    return {n: sum(w[n] for w in wins) for n in CNT}


def consumed_a(w, flags: int = 0):
    return w["n_eq"] + w["n_x"] + (w["n_del"] if flags & B_IS_QUERY else w["n_ins"])


def check_invariants(wins, res, W: int, flags: int = 0):
    """the windows sum to the pair's counts, every window consumes an a-element, interior windows consume exactly W"""
    assert cr.identities(total(wins), res, flags)
    if res["matlen_a"] >= 1:
        assert all(consumed_a(w, flags) >= 1 for w in wins)
    assert all(consumed_a(w, flags) == W for w in wins[1:-1])
    assert all(consumed_a(w, flags) <= W for w in wins)


def tup(w):
    return tuple(int(w[n]) for n in CNT)


# ----------------------------------------------------------------------------- the trim rule
def thr_table(max_err: float, W: int):
    return [int(max_err * float(m)) for m in range(W + 1)]


def trim(wins, W: int, max_err: float, min_span: int):
    """the span (SPAN_FIELDS as a dict) of one item's windows in the order given, I / D named as under the default flags"""
    thr = thr_table(max_err, W)
    na = [w["n_eq"] + w["n_x"] + w["n_ins"] for w in wins]
    nb = [w["n_eq"] + w["n_x"] + w["n_del"] for w in wins]
    err = [w["n_x"] + w["n_ins"] + w["n_del"] for w in wins]
    good = [e <= thr[a] for a, e in zip(na, err)]
    runs, s = [], None
    for k, g in enumerate(good + [False]):
        if g and s is None:
            s = k
        if not g and s is not None:
            runs.append((s, k))
            s = None
    out = dict.fromkeys(SPAN_FIELDS, 0)
    out.update(state=DROPPED, n_win=len(wins), n_good=sum(good), n_runs=len(runs))
    if not runs:
        return out
    beg, end = max(runs, key=lambda r: (sum(na[r[0]:r[1]]), -r[0]))         # the largest sum of na, then the first
    if sum(na[beg:end]) < min_span or sum(nb[beg:end]) == 0:
        return out
    out.update(state=WHOLE if (beg, end) == (0, len(wins)) else CUT, w_beg=beg, w_end=end, a0=sum(na[:beg]), b0=sum(nb[:beg]),
               na=sum(na[beg:end]), nb=sum(nb[beg:end]), cost=sum(err[beg:end]))
    return out


def row_trim(row, slen: int, wins_target_order, W: int, max_err: float, min_span: int):
    """ROW_FIELDS as a dict for one overlap row: its windows in the TARGET's forward order, I / D under the default flags
    (a = the target).  a0 / b0 are counted in element order, the reverse of the target's order for dir -1."""
    s = trim(wins_target_order, W, max_err, min_span)
    out = {n: s[n] for n in ("state", "n_win", "n_good", "n_runs", "w_beg", "w_end", "cost")}
    out.update(t_beg=0, t_end=0, q_beg=0, q_end=0)
    if s["state"] == DROPPED:
        return out
    elem = wins_target_order if int(row["dir"]) == 1 else wins_target_order[::-1]
    beg, end = (s["w_beg"], s["w_end"]) if int(row["dir"]) == 1 else (len(elem) - s["w_end"], len(elem) - s["w_beg"])
    na_of = lambda w: w["n_eq"] + w["n_x"] + w["n_ins"]
    nb_of = lambda w: w["n_eq"] + w["n_x"] + w["n_del"]
    a0, b0 = sum(na_of(w) for w in elem[:beg]), sum(nb_of(w) for w in elem[:beg])
    na, nb = s["na"], s["nb"]
    j = int(row["j"])
    if int(row["dir"]) == 1:
        tb, te = int(row["t_beg"]) + a0, int(row["t_beg"]) + a0 + na
        w0, w1 = j + b0, j + b0 + nb
    else:
        tb, te = int(row["t_end"]) - a0 - na, int(row["t_end"]) - a0
        w0, w1 = slen - j - b0 - nb, slen - j - b0
    qb, qe = (w0, w1) if int(row["strand"]) == 1 else (slen - w1, slen - w0)
    # inside the row's own intervals
    assert int(row["t_beg"]) <= tb <= te <= int(row["t_end"]) and int(row["q_beg"]) <= qb < qe <= int(row["q_end"]), (row, out, tb, te, qb, qe)
    out.update(t_beg=tb, t_end=te, q_beg=qb, q_end=qe)
    return out


def apply_trims(rows, trims):
    """interval rows: the rows that are not DROPPED with their four ends replaced"""
    out = []
    for r, t in zip(rows, trims):
        if t["state"] == DROPPED:
            continue
        r = r.copy()
        for n in ("t_beg", "t_end", "q_beg", "q_end"):
            r[n] = t[n]
        out.append(r)
    return np.array(out, rows.dtype) if out else rows[:0].copy()


def row_elems(row, texts):
    """(a, b, a_pos, back): the elements of an overlap row's two accessors in element order (pba_overlap_row_pair: a = the
    target), b from the reverse complement of the query for strand -1, and a's origin on the target"""
    t, q = texts[int(row["target"])], texts[int(row["query"])]
    qt = q if int(row["strand"]) == 1 else rc(q)
    j, p = int(row["j"]), int(row["ref_pos"])
    if int(row["dir"]) == 1:
        return t[p:], qt[j:], p, False
    return t[:p + 16][::-1], qt[:len(q) - j][::-1], p + 15, True


def row_windows(oracle, row, texts, R: float, W: int, flags: int):
    """the windows of an overlap row from the oracle's script, in the order `flags` gives; also the oracle's result"""
    a, b, a_pos, back = row_elems(row, texts)
    x = oracle.align(a, b, R, want_ops=True)
    assert (x["rc"] >= 0, x["cost"], x["matlen_a"], x["matlen_b"]) == (True, int(row["cost"]), int(row["matlen_a"]), int(row["matlen_b"])), row
    return from_script(x["ops"], a, b, a_pos, back, W, flags), x


def overlap_row_flags(row):
    """target forward: goal-first for dir -1; the query read is the query"""
    return B_IS_QUERY | (REVERSED if int(row["dir"]) == -1 else 0)


# ----------------------------------------------------------------------------- the planted 6 % input
# PLANTED of clip_ref with the generator at 2 % insertions, deletions and substitutions each and no junk tails: rows run
# across a chimeric junction on R's unused budget, which the plain clip rule cannot see.
TRIM = dict(p=0.02, W=100, max_err=0.25, min_span=64)
CLEAN_WHOLE_SLACK = 4                                          # 2 % of the 197 clean reads


def planted_reads_6(P=PLANTED, p=TRIM["p"]):
    """clip_ref.planted_reads at error p + p + p, without the junk tails: (texts, chimeras {read: junction})"""
    from pacbioassembly_amd import engine as eng
    n, rl = P["n"], P["rl"]
    g = eng.synth_genome(P["seed_g"], P["glen"])
    reads, offs, starts = eng.synth_reads(P["seed_r"], g, 2 * n, rl, p, p, p)    # reads n .. 2n - 1: the pool of pieces
    rng = np.random.default_rng(P["seed_p"])
    src = [reads[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(2 * n)]
    texts, chim = src[:n], {}
    pool = list(range(n, 2 * n))
    for i in range(n):
        if i % P["every"] == 3:
            a = pool.pop(int(rng.integers(0, len(pool))))
            far = [k for k in pool if abs(int(starts[k]) - int(starts[a])) >= 2 * rl]
            b = far[int(rng.integers(0, len(far)))]
            pool.remove(b)
            J = int(rng.integers(rl // 3, 2 * rl // 3 + 1))
            tail = src[b][:rl - J]
            texts[i] = src[a][:J] + (rc(tail) if rng.integers(0, 2) else tail)
            chim[i] = J
    for i in range(n):
        if rng.integers(0, 2):
            texts[i] = rc(texts[i])
            if i in chim:
                chim[i] = len(texts[i]) - chim[i]
    return texts, chim


def planted_conditions(plain_table, trimmed_table, chim, margin, say=print):
    """The conditions both planted tests assert, on the clip tables (clip_ref.ROW_FIELDS tuples) made from the plain rows and
    from the trimmed ones; everything else is printed."""
    from clip_ref import PLANTED_CHIMERAS_SPANNED_MAX, planted_report
    plain, trimmed = planted_report(plain_table, chim, {}, margin), planted_report(trimmed_table, chim, {}, margin)
    say("plain  :", plain)
    say("trimmed:", trimmed)
    for i, J in sorted(chim.items()):
        say("chimera", i, "junction", J, "plain ->", plain_table[i], "trimmed ->", trimmed_table[i])
    assert len(chim) == 11
    assert plain["chimeras_whole"] >= 6                        # an input the old rule cannot see
    assert trimmed["chimeras_whole"] == 0
    assert trimmed["chimeras_spanned"] <= PLANTED_CHIMERAS_SPANNED_MAX
    assert trimmed["clean_whole"] >= plain["clean_whole"] - CLEAN_WHOLE_SLACK
    return plain, trimmed
