"""Deterministic inputs for the one-lane prefilters (prefilter.h: prefilter32_planes, prefilter32_fails, prefilter64): pairs
whose FIRST failing row of the reference's diagonal check (cost(i, i) > i R for i > 10) is a chosen row of 11 .. 64, pairs that
fail in one stretch of equal thresholds only, and pairs that ride the bound through row 64 and are then clean.  No GPU in here:
test_prefilter_inputs_cpu.py proves from two references what each input is, test_gpu_prefilter_rows.py runs the kernels on them.

Seed anchoring.  Every pair a prefilter sees begins at a seed hit: rows 1 .. 16 of the two sides agree except where the mask
has a wildcard.  Forward, row i is base i - 1 of the window (MASK_PAT: wildcards at rows 4, 7, 10, 12); a backward pair starts
at the window's LAST base and walks down, so row i is base 16 - i (rows 5, 7, 10, 13).  From row 17 on anything goes.  With
c(i) = the number of rows <= i at which the sides differ (every builder keeps cost(i, i) = c(i): substitutions only, and around
them one side over A / C, the other over G / T, so that no path with an indel is cheaper) and T(i) = floor((double) i R):

    maxc(i) = |free rows <= i|                          for i <= 10   (rows up to 10 are never checked)
    maxc(i) = min(T(i), maxc(i - 1) + [i is free])      for i >= 11   (the most a pair can cost at row i with rows 11 .. i passing)
    row f is reachable as a FIRST failing row  <=>  maxc(f - 1) + [f is free] > T(f)

(fail_at's rule -- an integer c with c <= (f - 1) R and c + 1 > f R -- under the constraint of where the sides may differ.)
Two consequences the CPU test asserts: rows 13 .. 16 are out of reach of a forward MASK_PAT pair at any R (ALT_PAT, a mask with
its wildcards there, reaches them through the locator), and at R = 0.9 no row of 11 .. 64 is in reach of any seeded pair
(the dearest one costs i - 12 at row i, below 0.9 i until row 121): what R = 0.9 can show is that nothing fails falsely."""
import functools

import numpy as np

import align_rings as ar
from conftest import MASK_PAT

ALT_PAT = "1111111111*1****"          # wildcards at rows 11, 13, 14, 15, 16 of a forward pair
HEAVY_PAT = "1111111*11111111"        # 30 care bits: the hashed probe table (row 8 forward, row 9 backward)
# 0.25 and 0.30: i R on or next to integers in FP64; 0.07: T(11 .. 14) = 0; 0.30 and 0.15: the benchmark's; 0.28: the row-10 edge;
# 0.9: threshold bytes up to 57 and a stretch end at nine rows of ten
RS = (0.07, 0.15, 0.25, 0.28, 0.30, 0.9)
TIGHT_RS = (0.07, 0.15, 0.25, 0.28, 0.30)
EDGE10_R = 0.28
LAST = 64

# entry point -> (mask pattern, forward) of the pairs it can be handed
ENTRIES = {
    "locate": (MASK_PAT, True),
    "locate_alt_mask": (ALT_PAT, True),
    "scan_forward": (MASK_PAT, True),             # k_ovl_scan<false>, the walk's rows 33 .. 64, the spaced round: same pairs
    "scan_backward": (MASK_PAT, False),
    "scan_hashed_forward": (HEAVY_PAT, True),
    "scan_hashed_backward": (HEAVY_PAT, False),
}


class Unreachable(ValueError):
    pass


def thresholds(R: float, n: int = LAST + 1) -> np.ndarray:
    """T[i] = floor((double) i * R), i = 0 .. n: an integer cost is above i R iff it is above T[i]"""
    return np.floor(np.arange(n + 1, dtype=np.float64) * np.float64(R)).astype(np.int64)


def stretch_ends(R: float, lo: int = 11, hi: int = LAST):
    """rows lo .. hi that are the last of a stretch of equal thresholds"""
    T = thresholds(R, hi + 1)
    return [i for i in range(lo, hi + 1) if T[i + 1] != T[i]]


def seed_rows(pat: str, fwd: bool = True) -> frozenset:
    """rows 1 .. 16 at which a seeded pair may differ"""
    w = [i + 1 for i, c in enumerate(pat) if c != "1"]
    return frozenset(w if fwd else [17 - i for i in w])


def is_free(i: int, wild) -> bool:
    return i > 16 or i in wild


def max_costs(R: float, pat: str, fwd: bool = True, n: int = LAST) -> np.ndarray:
    T, wild = thresholds(R, n), seed_rows(pat, fwd)
    mc = np.zeros(n + 1, np.int64)
    for i in range(1, n + 1):
        mc[i] = mc[i - 1] + is_free(i, wild)
        if i >= 11:
            mc[i] = min(mc[i], T[i])
    return mc


def reachable(R: float, pat: str, fwd: bool = True, lo: int = 11, hi: int = LAST):
    T, wild, mc = thresholds(R, hi), seed_rows(pat, fwd), max_costs(R, pat, fwd, hi)
    return [f for f in range(lo, hi + 1) if mc[f - 1] + is_free(f, wild) > T[f]]


def diff_rows(R: float, pat: str, fwd: bool, f=None, n: int = LAST):
    """Rows at which the two sides differ, each at the first row the bound allows: up to row n with every row passing
    (f = None: the tightrope), or up to and including a first failing row f."""
    T, wild = thresholds(R, max(n, f or 0) + 1), seed_rows(pat, fwd)
    rows = []
    for i in range(1, (n if f is None else f - 1) + 1):
        if is_free(i, wild):
            chk = max(i, 11)                                          # the first checked row that sees this one (T never falls)
            # (rows that only f itself sees -- f = 11 -- take what makes cost(f, f) = T(f) + 1 and no more)
            if len(rows) + 1 <= (T[chk] if f is None or chk < f else T[f] + (not is_free(f, wild))):
                rows.append(i)
    if f is not None:
        if is_free(f, wild):
            rows.append(f)
        if len(rows) <= T[f]:
            raise Unreachable(f"row {f} cannot fail first at R = {R} behind {pat} ({'forward' if fwd else 'backward'})")
    return rows


def base_side(rng, m: int) -> bytes:
    """the side both builders start from: 16 random bases (the seed window), A / C up to row 64, random behind"""
    x = ar.rand_seq(rng, 16) + np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, LAST - 16)].tobytes() + ar.rand_seq(rng, max(0, m - LAST))
    return x[:m]


def other_side(rng, x: bytes, rows, junk_from=None, wild=frozenset()) -> bytes:
    """x with another base at each row of `rows` (G / T behind the seed window), and from row junk_from on at every free row.
    Drawn again until the plain matrix says that cost(i, i) is the number of differing rows <= i for every i <= 64: the two or
    three substitutions inside the seed window are between random bases, where a path with an indel is cheaper now and then."""
    rows = sorted((set(rows) | ({i for i in range(junk_from, len(x) + 1) if is_free(i, wild)} if junk_from else set())) & set(range(1, len(x) + 1)))
    n = min(LAST, len(x))
    want = np.searchsorted(np.array(rows, np.int64), np.arange(n + 1), side="right")
    for _ in range(200):
        y = bytearray(x)
        for i in rows:
            if i > 16 and x[i - 1] in b"AC":
                y[i - 1] = b"GT"[rng.randint(2)]
            else:
                y[i - 1] = ar.ALPHA[(int(np.searchsorted(ar.ALPHA, x[i - 1])) + 1 + rng.randint(3)) % 4]
        if (plain_diag(x, bytes(y)) == want).all():
            return bytes(y)
    raise RuntimeError("no draw keeps the substitutions the cheapest path: another base side is needed")


def fail_first_at(rng, f: int, R: float, pat: str = MASK_PAT, fwd: bool = True, m: int = 96, x=None):
    """(x, y) in accessor order, m elements each: the first failing row is f, and from f on the sides share nothing a mask lets
    differ.  x: a side made by base_side to build against (one read against many places)."""
    x = base_side(rng, m) if x is None else x
    return x, other_side(rng, x, diff_rows(R, pat, fwd, f), junk_from=f, wild=seed_rows(pat, fwd))


def blip_at(rng, f: int, R: float, pat: str = MASK_PAT, fwd: bool = True, m: int = 96, x=None):
    """like fail_first_at, but equal behind row f: cost(i, i) = T(f) + 1 from row f on, so only the rows from f to the end of
    f's stretch of equal thresholds fail (a verdict that looks at the wrong rows of the stretch lets the pair through)"""
    x = base_side(rng, m) if x is None else x
    return x, other_side(rng, x, diff_rows(R, pat, fwd, f))


def tightrope(rng, R: float, m: int = 96, pat: str = MASK_PAT, fwd: bool = True, x=None):
    """every row passes, cost(i, i) = max_costs(i) at every row, i.e. = T(i) at every stretch end of 11 .. 64 that a seeded pair
    can touch at all (the CPU test says which it cannot: row 16 at R = 0.30), equal behind row 64: the full aligner accepts it"""
    x = base_side(rng, m) if x is None else x
    return x, other_side(rng, x, diff_rows(R, pat, fwd))


def edge10_pair(rng, m: int = 96, x=None):
    """MASK_PAT's wildcard rows 4, 7 and 10 differ and nothing else: at R = 0.28 cost(10, 10) = 3 > 2.8, row 10 is not checked,
    and 3 <= 3.08 at row 11: the pair passes"""
    x = base_side(rng, m) if x is None else x
    return x, other_side(rng, x, (4, 7, 10))


# ----------------------------------------------------------------------------- the second reference
def plain_diag(a: bytes, b: bytes, n: int = LAST) -> np.ndarray:
    """D(i, i), i = 0 .. min(n, len a, len b), of the plain (unbanded) edit-distance matrix of a's and b's first elements"""
    n = min(n, len(a), len(b))
    A, B = np.frombuffer(a[:n], np.uint8), np.frombuffer(b[:n], np.uint8)
    ramp = np.arange(n + 1, dtype=np.int64)
    row, diag = ramp.copy(), [0]
    for i in range(1, n + 1):
        c = np.empty(n + 1, np.int64)
        c[0] = i
        c[1:] = np.minimum(row[1:] + 1, row[:-1] + (A[i - 1] != B))      # from above, from the diagonal
        row = np.minimum.accumulate(c - ramp) + ramp                      # ... and from the left
        diag.append(int(row[i]))
    return np.array(diag, np.int64)


def plain_fail_row(a: bytes, b: bytes, R: float, n: int = LAST) -> int:
    """the first row i in 11 .. n with D(i, i) > (double) i R, 0 if there is none"""
    d = plain_diag(a, b, n)
    bad = [i for i in range(11, d.size) if float(d[i]) > float(np.float64(i) * np.float64(R))]
    return bad[0] if bad else 0


# ----------------------------------------------------------------------------- the locator's case
def key_hits(text: bytes, window: bytes, pat: str):
    """positions of `text` whose 16-base window agrees with `window` at the mask's care positions"""
    t = np.frombuffer(text, np.uint8)
    n = len(text) - 15
    ok = np.ones(max(n, 0), bool)
    for k, c in enumerate(pat):
        if c == "1":
            ok &= t[k:k + n] == window[k]
    return [int(p) for p in np.nonzero(ok)[0]]


LOC_SPECS = ((1, 0, "tight"), (64, 0, "tight"), (65, 5, "tight"), (130, 11, "surv"), (65, 23, "fail"))
LOC_EDGE_MS = (31, 32, 33, 63, 64, 65)
LOC_MIN_LEN = 20


def _kinds(R, pat, k, rot, last):
    """the k places of one read in hit order: a rotation of every reachable first failing row (as a lasting failure and, up
    to row 32, as a blip), a survivor of the first 32 rows first (even rotations) and where `last` says"""
    reach = reachable(R, pat, True)
    pool = [("fail", f) for f in reach] + [("blip", f) for f in reach if f <= 32]
    if not pool:                                                      # R = 0.9: nothing can fail before row 121
        return [("dear", 0)] * (k - 1) + [("tight", 0) if last == "tight" else ("dear", 0)]
    surv = [f for f in reach if f > 32]
    small = [e for e in pool if e[1] <= 32]
    out = [pool[(rot + 7 * i) % len(pool)] for i in range(k)]
    for i in (1, 3, 31, 32, 63):                                      # rows the prefilter finds, at the lanes where masks turn over
        if i < k - 1:
            out[i] = small[(rot + i) % len(small)]
    if k > 3:
        out[2] = ("fail", surv[(rot + 2) % len(surv)])                # ... and a survivor between two of them
    out[0] = ("fail", surv[rot % len(surv)]) if rot % 2 == 0 else small[rot % len(small)]
    if last == "tight":
        out[-1] = ("tight", 0)
    elif last == "surv":
        out[-1] = ("fail", surv[-1])
    elif k > 1:
        out[-1] = ("fail", min(reach))
    return out


def locate_case(R: float, pat: str = MASK_PAT, NB: int = 1, specs=LOC_SPECS):
    """_locate_case from the first seed at which every read's key is found at its places and nowhere else"""
    for attempt in range(8):
        g, reads, meta = _locate_case(R, pat, NB, specs, attempt)
        if all(key_hits(g, x[:16], pat) == [p for p, _, _ in mt.get("places", ())] for x, mt in zip(reads, meta)):
            return g, reads, meta
    raise RuntimeError("no seed without a chance hit")


def _locate_case(R, pat, NB, specs, attempt):
    """(genome, reads, meta).  Every read has one probe (trials = 1) whose key is found at the places planted for it and nowhere
    else: meta[r]["places"] = [(position, kind, row)] in hit order -- kind "fail" / "blip": the pair read-against-genome-from-
    there fails first at `row`; "tight": the tightrope (it succeeds and ends the read's walk); "dear": the dearest seeded pair
    (R = 0.9).  Reads of LOC_EDGE_MS bases follow, one failing place each, then the pair that shows row 10 unchecked (R = 0.28),
    then -- ring 2 -- an unrelated filler read that sizes the plan."""
    rng = np.random.RandomState(9100 + int(R * 100) + 1000 * (pat != MASK_PAT) + 10000 * attempt)
    m = 96 if R < 0.5 else 160
    if R >= 0.5:
        specs = specs[:3]                                             # (longer places: the same few tens of kilobases)
    wild = seed_rows(pat, True)
    parts, reads, meta = [ar.rand_seq(rng, 200)], [], []
    at = [200]

    def plant(y):
        pos = at[0]
        parts.extend([y, ar.rand_seq(rng, int(rng.randint(20, 52)))])
        at[0] += len(y) + len(parts[-1])
        return pos

    def side(x, kind, f):
        if kind == "fail":
            return fail_first_at(rng, f, R, pat, True, x=x)[1]
        if kind == "blip":
            return blip_at(rng, f, R, pat, True, x=x)[1]
        if kind == "tight":
            return tightrope(rng, R, pat=pat, x=x)[1]
        if kind == "edge10":
            return edge10_pair(rng, x=x)[1]
        return other_side(rng, x, (), junk_from=1, wild=wild)        # "dear"

    def add_read(mx, kinds):
        x = base_side(rng, mx) if R < 0.5 else base_side(rng, 64) + np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, mx - 64)].tobytes()
        ys = [side(x, kind, f) for kind, f in kinds]
        reads.append(x)
        meta.append(dict(kind="planted", places=[(plant(y), kind, f) for y, (kind, f) in zip(ys, kinds)]))

    for k, rot, last in specs:
        add_read(m, _kinds(R, pat, k, rot, last))
    reach = reachable(R, pat, True)
    if reach:
        for mx in LOC_EDGE_MS:
            add_read(mx, [("fail", max(f for f in reach if f <= mx))])
    if R == EDGE10_R and pat == MASK_PAT:
        add_read(m, [("edge10", 0)])
    parts.append(ar.rand_seq(rng, 2 * m + 200))
    if NB == 2:
        reads.append(ar.pilot(ar.row_of(2, 2)[0], R, seed=2)[0])
        meta.append(dict(kind="filler"))
    return b"".join(parts), reads, meta


def locate_b_edges(R: float, pat: str = MASK_PAT):
    """(contigs, reads, rows): contig k ends LOC_EDGE_MS[k] bases behind the one place read k hits, so that the genome side is
    the clipped one; the pair fails first at rows[k]"""
    rng = np.random.RandomState(9300 + int(R * 100))
    contigs, reads, rows = [], [], []
    for lb in LOC_EDGE_MS:
        f = max(r for r in reachable(R, pat, True) if r <= (min(lb, 32) if lb < 60 else lb))
        x, y = fail_first_at(rng, f, R, pat, True)
        contigs.append(ar.rand_seq(rng, 100 + lb % 3) + y[:lb])
        reads.append(x)
        rows.append(f)
    return contigs, reads, rows


# ----------------------------------------------------------------------------- the all-vs-all case
OVL_MIN = 20             # OVERLAP_MIN of the calls: below the prefilters' 32 rows, so that sides of 31 .. 33 elements pass the gate
OVL_M = 96
OVL_MODS = (0, 1, 31, 17)
OVL_INDEL_ROWS = (17, 18, 21, 24)


def overlap_case(R: float, pat: str = MASK_PAT):
    """_overlap_case from the first seed at which enumeration finds the designed candidates and the four mirrors only.  (R = 0.9
    takes the first seed as it is: its places are 80 bases of G / T each, and a target's tail window over G / T finds one
    of them here and there -- enumerated and judged by the oracle like every other candidate.)"""
    for attempt in range(8):
        texts, designed, nq, wt = _overlap_case(R, pat, attempt)
        extra = {c[:4] for c in overlap_candidates(texts, pat)[0]} - {d[:4] for d in designed}
        if R >= 0.5 or (len(extra) == 4 and all(t < nq <= q for t, q, _, _ in extra)):
            return texts, designed, nq, wt
    raise RuntimeError("no seed without a chance hit")


def _overlap_case(R: float, pat: str, attempt: int):
    """(texts, designed, n_queries, walk_target).  Reads 0 .. n_queries - 1 are queries: a head whose forward probe (j = 0) and a
    tail whose backward probe hit planted places only; the reads behind them are targets that hold the places.  designed =
    [(target, query, forward, hit position, kind, row)].
      * targets 0 .. 6 (in target order): at the head a backward place and at the tail a forward place that reach the target's
        end after 96 (a tightrope: it is reported), 31, 32, 33, 63, 64, 65 elements; lengths that are multiples of 32 and one
        more; between them every reachable first failing row up to 32 as a lasting failure and as a blip, both directions
        alternating, the lowest base of a place's 32 elements at idx % 32 in 0, 1, 31, 17; queries of 31 .. 65 bases (a blip
        between random sides: kind "short"); and pairs of random sides with one base deleted or inserted at rows 17, 18, 21, 24
        (kind "indel"): behind it cost(i, i) rises to 2 and stays, which only the matrix's horizontal and vertical deltas can
        tell -- every other input here has its cheapest path on the diagonal, where a sweep that lost them would still agree;
      * the walk's target: 64 candidates that survive their first 32 rows, a tightrope in the first and in the last slot of
        the sorted list (the lowest and the highest query), between them 62 pairs that fail first at the reachable rows
        33 .. 64, both directions.
    A tightrope at a target's end is a true overlap, so the target's own probe at that end finds the query: four mirror
    candidates, (query read as target, target read as query), that no design can avoid."""
    rng = np.random.RandomState(9500 + int(R * 100) + 1000 * (pat != MASK_PAT) + 10000 * attempt)
    m = OVL_M
    reach = {True: reachable(R, pat, True), False: reachable(R, pat, False)}
    queries, targets = [], [dict(head=None, tail=None, mids=[]) for _ in range(8)]
    W = 7

    def pair(kind, f, fwd, L=m):
        if kind == "short":                                           # (a random side: its tail window must find nothing)
            return blip_at(rng, f, R, pat, fwd, m, x=ar.rand_seq(rng, m))
        if kind == "dear":                                            # R = 0.9: every free row differs, and every row up to 64 passes
            x = base_side(rng, m)
            return x, other_side(rng, x, (), junk_from=1, wild=seed_rows(pat, fwd))[:L]
        if kind == "indel":                                           # one base of x missing (even rows) or one base more, at row f
            x = ar.rand_seq(rng, m)
            y = x[:f - 1] + x[f:] + ar.rand_seq(rng, 1) if f % 2 == 0 else x[:f - 1] + ar.rand_seq(rng, 1) + x[f - 1:m - 1]
            return x, y[:L]
        if kind == "tight":
            x, y = tightrope(rng, R, m, pat, fwd)
        elif kind == "edge10":
            x, y = edge10_pair(rng, m)
        else:
            x, y = (fail_first_at if kind == "fail" else blip_at)(rng, f, R, pat, fwd, m)
        return x, y[:L]

    def query(head=None, tail=None, short=0):
        """head / tail: (kind, row, target, where) or None; returns the query's id"""
        q = len(queries)
        text = []
        for fwd, spec in ((True, head), (False, tail)):
            if spec is None:
                text.append(ar.rand_seq(rng, m))
                continue
            kind, f, t, where = spec
            x, y = pair(kind, f, fwd, where[1] if where[0] == "end" else m)
            text.append(x if fwd else x[::-1])
            rec = dict(q=q, fwd=fwd, kind=kind, f=f, y=y)
            if where[0] == "end":
                targets[t]["tail" if fwd else "head"] = rec
            else:
                targets[t]["mids"].append(dict(rec, mod=where[1]))
        queries.append(text[0][:short] if short else text[0] + ar.rand_seq(rng, 30) + text[1])
        return q

    big = {d: [f for f in reach[d] if f > 32] or [0] for d in (True, False)}
    small = {d: [f for f in reach[d] if f <= 32] or [0, 0] for d in (True, False)}
    fail = "fail" if reach[True] else "dear"
    below = lambda d, L: max([f for f in reach[d] if f <= (min(L, 32) if L < 60 else L)], default=0)
    # the walk's target first: the lowest query's tail, 31 queries with a place each way, the highest query's head
    query(tail=("tight", 0, W, ("end", m)))
    for i in range(31):
        query(head=(fail, big[True][i % len(big[True])], W, ("mid", OVL_MODS[i % 4])),
              tail=(fail, big[False][(i + 5) % len(big[False])], W, ("mid", OVL_MODS[(i + 1) % 4])))
    query(head=("tight", 0, W, ("end", m)))
    # targets 0 .. 6: the ends ...
    ends = (m,) + LOC_EDGE_MS
    for t, L in enumerate(ends):
        spec = {}
        for d in (True, False):
            if L == m:
                spec[d] = ("tight", 0, t, ("end", m))
            else:
                spec[d] = (fail, below(d, L), t, ("end", L))
        query(head=spec[True], tail=spec[False])
    # ... and what lies between them
    mids = {d: [(k if reach[d] else "dear", f) for f in small[d] for k in ("blip", "fail")] for d in (True, False)}
    for d in (True, False):                                            # (rows above 32 the walk's target had no room for)
        on_w = {big[d][(i + (0 if d else 5)) % len(big[d])] for i in range(31)}
        mids[d] += [("fail", f) for f in big[d] if f and f not in on_w]
        mids[d] += [("indel", r) for r in OVL_INDEL_ROWS]
    if R == EDGE10_R and pat == MASK_PAT:
        mids[True].append(("edge10", 0))
    for i in range(max(len(mids[True]), len(mids[False]))):
        h = mids[True][i] if i < len(mids[True]) else None
        tl = mids[False][i] if i < len(mids[False]) else None
        query(head=h and (h[0], h[1], i % 7, ("mid", OVL_MODS[i % 4])), tail=tl and (tl[0], tl[1], (i + 3) % 7, ("mid", OVL_MODS[(i + 2) % 4])))
    for i, L in enumerate(LOC_EDGE_MS if reach[True] else ()):         # short queries: the probe's side is the clipped one
        query(head=("short", below(True, L), i, ("mid", OVL_MODS[i % 4])), short=L)
    nq = len(queries)
    texts, designed = list(queries), []
    for t, tg in enumerate(targets):
        buf = bytearray()
        places = []
        if tg["head"]:
            y = tg["head"]["y"]
            buf += y[::-1]
            places.append((tg["head"], len(y) - 16))
        buf += ar.rand_seq(rng, 40)
        for rec in tg["mids"]:
            buf += ar.rand_seq(rng, 8 + (rec["mod"] - len(buf) - 8) % 32)        # the place starts at a position = mod (32)
            places.append((rec, len(buf) if rec["fwd"] else len(buf) + len(rec["y"]) - 16))
            buf += rec["y"] if rec["fwd"] else rec["y"][::-1]
        L = len(tg["tail"]["y"]) if tg["tail"] else 0
        buf += ar.rand_seq(rng, 40)
        buf += ar.rand_seq(rng, (t % 2 - len(buf) - L) % 32)                     # the whole length = 0 or 1 (32)
        if tg["tail"]:
            places.append((tg["tail"], len(buf)))
            buf += tg["tail"]["y"]
        texts.append(bytes(buf))
        designed += [(nq + t, rec["q"], rec["fwd"], hit, rec["kind"], rec["f"]) for rec, hit in places]
    return texts, designed, nq, nq + W


def overlap_candidates(texts, pat: str, overlap_min: int = OVL_MIN, qtexts=None):
    """Every candidate of an all-vs-all call with one trial, by enumeration: [(target, query, forward, hit, a, b)] -- the
    query's head window (forward) or tail window (backward) found at a visited position of another read (0 .. len - 17 at these
    lengths: ref_seq's get_seedmap), past the OVERLAP_MIN gate; a, b: the two accessors' elements.  qtexts: the queries' bases
    where they are not the targets' (the reverse-complement pass of pba_overlap_strands), read for read."""
    out, n_match = [], 0
    for q, qt in enumerate(texts if qtexts is None else qtexts):
        if len(qt) < 16:
            continue
        for fwd in (True, False):
            win = qt[:16] if fwd else qt[-16:]
            assert any(win[k] != 65 for k, c in enumerate(pat) if c == "1")       # (a zero key is never looked up)
            for t, tt in enumerate(texts):
                if t == q:
                    continue
                for p in key_hits(tt, win, pat):
                    if p > len(tt) - 17:
                        continue
                    n_match += 1
                    if len(qt) >= overlap_min:
                        out.append((t, q, fwd, p, tt[p:] if fwd else tt[:p + 16][::-1], qt if fwd else qt[::-1]))
    return out, n_match


# ----------------------------------------------------------------------------- the walk's group edges
# The walk takes a target's sorted survivors 64 at a time (overlap.h: ovl_walk); a (target, query) run belongs to the group it
# starts in.  One target per situation, each run as (forward failures, forward success, backward success, backward failures):
# within a run the forward candidates come first, by position -- so the success at the target's tail is the last of them -- and
# the backward ones behind, the success at the target's head first.  FILL = a run of 16 that fails.
STRADDLE_FILL = (8, False, False, 8)
STRADDLE_RUNS = {
    # slots 48 .. 72: the run crosses 63 | 64, fails 24 times -- eight of them in the second group -- and succeeds at slot 72
    "a": (STRADDLE_FILL,) * 3 + ((24, True, False, 0), (10, False, True, 4)),
    # slots 48 .. 76: the first success at slot 63, another one at slot 64 that nobody may report
    "b": (STRADDLE_FILL,) * 3 + ((15, True, True, 12), STRADDLE_FILL),
    # slots 64 .. 74: the run starts with the second group
    "c": (STRADDLE_FILL,) * 4 + ((10, True, False, 0), (6, False, True, 5)),
}
STRADDLE_PLACE = 68      # elements of a failing place: the 64 rows and a few more


def _comp(x: bytes) -> bytes:
    return x.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


@functools.lru_cache(maxsize=None)
def straddle_case(R: float, pat: str = MASK_PAT):
    """_straddle_case from the first seed at which the three targets hold the designed candidates only"""
    for attempt in range(8):
        texts, designed, nq = _straddle_case(R, pat, attempt)
        found = {c[:4] for c in overlap_candidates(texts, pat)[0] if c[0] >= nq}
        if found == set(designed):
            return texts, designed, nq
    raise RuntimeError("no seed without a chance hit")


def _straddle_case(R: float, pat: str, attempt: int):
    """(texts, designed, n_queries): the queries (a head and a tail of 96 bases whose windows hit planted places only), then one
    target per entry of STRADDLE_RUNS, its runs in query order.  designed = {(target, query, forward, hit position)}.  Every
    failing place fails first at a reachable row of 33 .. 64 (it is listed by the scan, rows 33 .. 64 or the array fail it);
    a success is a tightrope that reaches the target's end."""
    rng = np.random.RandomState(9700 + int(R * 100) + 10000 * attempt)
    m = OVL_M
    big = {d: [f for f in reachable(R, pat, d) if f > 32] for d in (True, False)}
    queries, plans = [], []
    for name in sorted(STRADDLE_RUNS):
        plan = []
        for run in STRADDLE_RUNS[name]:
            xh, xt = base_side(rng, m), base_side(rng, m)
            plan.append((len(queries), xh, xt, run))
            queries.append(xh + ar.rand_seq(rng, 30) + xt[::-1])
        plans.append(plan)
    nq = len(queries)
    texts, designed, k = list(queries), [], 0
    for t, plan in enumerate(plans):
        head, tail, mids = None, None, []
        for q, xh, xt, (nf, f_ok, b_ok, nb) in plan:
            for d, x, n in ((True, xh, nf), (False, xt, nb)):
                for _ in range(n):
                    k += 1
                    mids.append((q, d, fail_first_at(rng, big[d][k % len(big[d])], R, pat, d, m, x=x)[1][:STRADDLE_PLACE]))
            if f_ok:
                assert tail is None
                tail = (q, tightrope(rng, R, m, pat, True, x=xh)[1])
            if b_ok:
                assert head is None
                head = (q, tightrope(rng, R, m, pat, False, x=xt)[1])
        buf = bytearray()
        if head:
            buf += head[1][::-1]
            designed.append((nq + t, head[0], False, len(buf) - 16))
        for q, d, y in mids:
            buf += ar.rand_seq(rng, int(rng.randint(8, 16)))
            designed.append((nq + t, q, d, len(buf) if d else len(buf) + len(y) - 16))
            buf += y if d else y[::-1]
        buf += ar.rand_seq(rng, int(rng.randint(8, 16)))
        if tail:
            designed.append((nq + t, tail[0], True, len(buf)))
            buf += tail[1]
        texts.append(bytes(buf))
    return texts, designed, nq


def straddle_views(R: float, NB: int = 1):
    """The two ways the case is run, as {name: (texts, qtexts)}: "forward" (pba_overlap_all: queries and targets from one set)
    and "rc" (the reverse-complement pass of pba_overlap_strands over the set whose QUERY reads were flipped: its queries' bases
    are the designed ones again).  NB = 2: behind an unrelated long read that sizes the plan."""
    texts, _, nq = straddle_case(R)
    if NB == 2:
        texts = texts + [ar.pilot(ar.row_of(2, 2)[0], R, seed=3)[0]]
    mixed = [_comp(x) if i < nq else x for i, x in enumerate(texts)]
    return {"forward": (texts, texts), "rc": (mixed, [_comp(x) for x in mixed])}, nq


def walk_composition(oracle, texts, qtexts, R: float, pat: str = MASK_PAT, overlap_min: int = OVL_MIN):
    """What the all-vs-all walk has to do, from the enumeration and the oracle's verdict per candidate alone.  Returns
    dict(slices = {target: its listed candidates in the order of the sorted slice, each with its verdict x}, n_match, n_pre,
    n_listed, rows = [(target, query, dir, ref_pos, cost, matlen_a, matlen_b)] and pairs of a plain walk of every candidate
    in that order: a run is tried until its first success, ref_seq.h:264-265)."""
    cands, n_match = overlap_candidates(texts, pat, overlap_min, qtexts)
    cands.sort(key=lambda c: (c[0], c[1], not c[2], c[3]))
    slices, rows, pairs, n_pre, done = {}, [], 0, 0, None
    for t, q, fwd, p, a, b in cands:
        x = oracle.align(a, b, R)
        ok = x["rc"] > 0 and x["matlen_a"] >= overlap_min
        if x["rc"] == -1 and 11 <= x["fail_row"] <= 32 and x["len_a"] >= 32 and x["len_b"] >= 32:
            n_pre += 1                                                    # settled by the scan's 32 rows: counted, never listed
        else:
            slices.setdefault(t, []).append(dict(q=q, fwd=fwd, p=p, x=x, ok=ok))
        if done == (t, q):
            continue
        pairs += 1
        if ok:
            done = (t, q)
            rows.append((t, q, 1 if fwd else -1, p, x["cost"], x["matlen_a"], x["matlen_b"]))
    return dict(slices=slices, n_match=n_match, n_pre=n_pre, n_listed=sum(len(v) for v in slices.values()), rows=rows, pairs=pairs)


def straddle_situations(slices):
    """which of the three situations each target of 65 .. 192 listed candidates shows at slots 63 | 64: {target: "a" / "b" / "c"}"""
    out = {}
    for t, L in slices.items():
        if not 65 <= len(L) <= 192:
            continue
        if L[63]["q"] != L[64]["q"]:
            out[t] = "c"                                                  # a run starts exactly at slot 64
            continue
        run = [i for i, c in enumerate(L) if c["q"] == L[63]["q"]]
        wins = [i for i in run if L[i]["ok"]]
        if wins and wins[0] >= 64 and any(L[i]["x"]["rc"] == -1 and 33 <= L[i]["x"]["fail_row"] <= 64 for i in range(64, wins[0])):
            out[t] = "a"                                                  # followed past the group's end, the array fails what lies before the success
        elif wins and wins[0] <= 63 and any(i >= 64 for i in wins):
            out[t] = "b"                                                  # done in the first group; a success behind the edge that must be skipped
    return out


def oracle_composition(oracle, texts, qtexts, R: float, pat: str = MASK_PAT, overlap_min: int = OVL_MIN):
    """(rows, pairs) of the oracle's locked spaced_seed round of every target against the file of the queries, one trial, the
    target's own read left out: rows as walk_composition's"""
    from pacbioassembly_amd import engine as eng
    file = b"".join(eng.text2bin(t) for t in qtexts)
    offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in qtexts[:-1]]).astype(np.uint64)
    mask = eng.mask_from_pattern(pat)
    want, pairs = [], 0
    for t in range(len(texts)):
        r = oracle.spaced_round(texts[t], mask, R, file, offs, 1, overlap_min, buggy=False, nthreads=8)
        pairs += int(r["n_pairs"].sum()) - int(r["n_pairs"][t])
        assert not r["j"][r["found"] == 1].any()
        want += [(t, q, int(r["dir"][q]), int(r["ref_pos"][q]), int(r["cost"][q]), int(r["matlen_a"][q]), int(r["matlen_b"][q]))
                 for q in range(len(texts)) if q != t and r["found"][q]]
    return want, pairs
