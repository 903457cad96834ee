"""Read sets that put the all-vs-all walk (overlap.h: k_ovl_walk<NB>, k_ovl_walk_rc<NB>) into a chosen ring, stage and parked-run
edge.  No GPU and no engine in here: test_walk_rings_cpu.py proves from overlap_ref.walk_composition, the oracle and the constants
of align_bitvec.h (align_rings.py) what every set is, test_gpu_walk_rings.py holds the kernels to the model on the same sets.

  A  collect_set      the lane-held one-hot of align_bitvec<NB, BAIL>: pairs whose first failing row sits at the first, second,
                      31st and last row of every block (diag_collect_inputs.py), each as a read and its copy, one probe per
                      read -- a pair is one head candidate in either order.  Rings >= 2 behind an unrelated filler read that
                      sizes the plan and is left out of the target range.
  B  stage_set        one set per plan row: reads of one length L whose cost is planted (the copy carries G / T where the read
                      has A / C: one edit each, whatever the path), at the first launch's window w1, one above it, at the middle
                      ring's window and one above that; a pair the narrow sweep gives up and the wider one fails; short pairs.
  C  parked_set       row (1, 2): one target, a list of short queries that are runs of one in query order, and planted-cost
                      queries placed among them by their index: the parked candidate at slot 0, 63, 64 of its target's list, as
                      a continuation past its item's end, in front of a candidate that would succeed narrowly, two in one item.

How the stages are derived (stages): a candidate whose window is its whole band is decided where it is tried; the others are
the planted ones, whose diagonal is known row by row -- given up where the condition of segment_done holds, parked where the
cost is above the window, failed where the reference fails them if the window certifies that row."""
import functools

import numpy as np

import align_rings as ar
import diag_collect_inputs as dc
import overlap_ref as orf
from conftest import MASK_PAT
from overlap_edge_inputs import Set, flipped_view

MASK = orf.mask_of(MASK_PAT)
WAVE = 64
AC, GT = np.frombuffer(b"AC", np.uint8), np.frombuffer(b"GT", np.uint8)


# ----------------------------------------------------------------------------- the oracle's answers, once per session
_ALIGNS = {}


class Cached:
    """oracle.align(a, b, R) answered once per (a, b, R) in a session, as align_rings.expected does; for sides of 512 rows
    and more the diagonal's cost at every 32nd row and at the last one is kept beside the answer (x["diag"]: {row: cost})."""

    def __init__(self, oracle):
        self.oracle = oracle

    def align(self, a, b, R):
        key = (a, b, R)
        if key not in _ALIGNS:
            x = self.oracle.align(a, b, R)
            m = min(x["len_a"], x["len_b"])
            if m >= 512:
                last = x["fail_row"] - 1 if x["rc"] == -1 and x["fail_row"] > 0 else m
                x["diag"] = {i: self.oracle.cell(i, i)[0] for i in sorted(set(range(32, last + 1, 32)) | {last})}
            _ALIGNS[key] = x
        return _ALIGNS[key]


def model(oracle, C, view="forward"):
    """overlap_ref.walk_composition of a case (dict: texts, queries, R, max_trial, overlap_min, t_lo, t_hi), with the case's
    fields beside it; view "rc": the reverse-complement pass over the set with its query reads flipped"""
    key = (C["name"], view)
    if key not in _MODELS:
        texts, qtexts = (C["texts"], C["texts"]) if view == "forward" else flipped_view(C["S"])
        W = orf.walk_composition(Cached(oracle), texts, qtexts, C["R"], MASK, C["max_trial"], C["overlap_min"], t_lo=C["t_lo"], t_hi=C["t_hi"])
        W.update(C, texts=texts, qtexts=qtexts, mask=MASK)
        _MODELS[key] = W
    return _MODELS[key]


_MODELS = {}


def case_of(S, name, R, max_trial, overlap_min, t_lo, t_hi, **more):
    return dict(S=S, name=name, texts=S.texts, R=R, max_trial=max_trial, overlap_min=overlap_min, t_lo=t_lo, t_hi=t_hi, **more)


def call_md(C):
    """the max_dst the call's plan is made from (overlap_table: the longest read of the set)"""
    return 1 + int(max(len(t) for t in C["texts"]) * C["R"])


def nb_mid_of(n1, n2):
    """ovl_walk: the widest instantiated ring between the narrow one and the reference band's (0: none)"""
    return max([nb for nb in ar.RINGS if n1 < nb < n2 and nb < ar.MAX_NB], default=0)


# ----------------------------------------------------------------------------- the walk's lists and stages
def listed(W):
    """{target: [candidate]} of what the walk's list holds: the candidates the scan did not settle, in try order; a
    candidate's place in it is its slot, slot // 64 its work item"""
    out = {}
    for c in W["cands"]:
        if not c["pre"]:
            out.setdefault(c["t"], []).append(c)
    return out


def items_of(W):
    """[(target, item)] in the order of the device's list: ceil(listed / 64) per target"""
    return [(t, g) for t, L in sorted(listed(W).items()) for g in range((len(L) + WAVE - 1) // WAVE)]


def gives_up(diag, m, w, upto, margin=1.0):
    """the rows (every 32nd from 1 024 on, and row m) up to `upto` at which segment_done's condition holds, in float32:
    (D - 4 sqrt(D)) m > i w; margin: ... holds by that factor (> 1), or fails by it (< 1)"""
    f32 = np.float32
    out = []
    for i in sorted(diag):
        if i >= 1024 and i <= upto and (i % 32 == 0 or i == m):
            end = f32(diag[i])
            if (end - f32(4.0) * np.sqrt(end)) * f32(m) > f32(i) * f32(w) * f32(margin):
                out.append(i)
    return out


def outcome(c, nb, full, R):
    """what one sweep of candidate c in ring nb says: "ok", "no" (decided, no success) or "park"; full: the reference band"""
    x = c["x"]
    md, m = x["max_dst"], min(x["len_a"], x["len_b"])
    w = md if full else ar.bv_pass1_w(md, nb)
    wl = ar.bv_full_wl(md) if full else ar.bv_pass1_wl(md, nb)
    assert wl + w <= ar.bv_max_span(nb), (nb, md)
    decided = "ok" if c["ok"] else "no"
    if m <= 10 or (w >= md and 2 * wl + 1 >= md):
        return decided
    assert "diag" in x, "a candidate in a narrow window that no builder planted"
    fr = x["fail_row"] if x["rc"] == -1 and x["fail_row"] > 0 else 0
    bail_w = w if not full and w < md else 0
    if bail_w and gives_up(x["diag"], m, bail_w, fr - 1 if fr else m):
        return "park"
    if fr:
        return "no" if 2 * wl + 2 > md or fr * R < 2 * wl + 2 else "park"
    assert x["rc"] >= 0
    return decided if x["cost"] <= w and x["cost"] <= 2 * wl + 1 else "park"


def stages(W, env=None):
    """The launches of ovl_walk for the call of W, from the model's candidates and outcome(): dict(launches = [(ring, form,
    work items)], parked = what the stats' n_redo counts, wide_first, rows, nb_first, n_first, nb_redo, n_redo = the ctx
    profile).  env: None, "wide" (PBA_OVL_WIDE=1) or "sample" (PBA_OVL_SAMPLE_MIN=1)."""
    md = call_md(W)
    n1, n2 = ar.nb1(md), ar.nb2(md)
    mid = nb_mid_of(n1, n2)
    L = listed(W)
    launches, rows = [], []

    def run_from(t, at, nb, full):
        """the run of L[t][at]'s query from slot `at` on; the slot it parks at, or None"""
        q = L[t][at]["q"]
        for s in range(at, len(L[t])):
            c = L[t][s]
            if c["q"] != q:
                break
            o = outcome(c, nb, full, W["R"])
            if o == "park":
                return s
            if o == "ok":
                x = c["x"]
                rows.append((t, q, c["jd"] >> 1, -1 if c["jd"] & 1 else 1, c["p"], x["cost"], x["matlen_a"], x["matlen_b"]))
                break
        return None

    def first_form(items, nb, full):
        launches.append((nb, "band" if full else "first", len(items)))
        parked = []
        for t, g in items:
            for s in range(WAVE * g, min(WAVE * g + WAVE, len(L[t]))):
                if s == 0 or L[t][s - 1]["q"] != L[t][s]["q"]:            # a run that starts in the item is the item's
                    at = run_from(t, s, nb, full)
                    if at is not None:
                        parked.append((t, at))
        return parked

    def redo_form(parked, nb, full):
        launches.append((nb, "redo_band" if full else "redo", len(parked)))
        return [(t, at) for t, s in parked for at in [run_from(t, s, nb, full)] if at is not None]

    def narrow_then_redo(items, nb):
        if not items:
            return 0
        p1 = first_form(items, nb, False)
        left = p1
        if left and mid > nb:
            left = redo_form(left, mid, False)
        if left:
            assert redo_form(left, n2, True) == []
        return len(p1)

    items = items_of(W)
    n_all = len(items)
    wide = 1 if env == "wide" else -1
    decided = wide >= 0 and env != "sample"
    n_sample = 0 if decided else n_all if env != "sample" else min(n_all, max(1, n_all // 32))
    parked = narrow_then_redo(items[:n_sample], n1)
    wide_first = 0
    if n_sample < n_all:
        wide_first = int(wide == 1 if decided else 2 * parked > len(rows))
        if wide_first and not mid:
            assert first_form(items[n_sample:], n2, True) == []
        else:
            parked += narrow_then_redo(items[n_sample:], mid if wide_first else n1)
    redo = [l for l in launches if l[1].startswith("redo")]
    return dict(launches=launches, parked=parked, wide_first=wide_first, rows=sorted(rows), nb_first=launches[0][0] if launches else 0,
                n_first=launches[0][2] if launches else 0, nb_redo=redo[-1][0] if redo else 0, n_redo=redo[-1][2] if redo else 0)


# ----------------------------------------------------------------------------- A: the lane-held one-hot
COLLECT_NBS = (1, 2, 3, 6)
COLLECT_MIN = 64
ROW_OF_RING = {1: (1, 1), 2: (2, 2), 3: (3, 4), 6: (6, 8)}
RING6_SUPERBLOCKS = (0, 1)


def collect_geometry(NB):
    """[(superblock, block, position)] of the rows of ring NB that the array judges (rows > 64: the others are the one-lane
    prefilters')"""
    sbs = RING6_SUPERBLOCKS if NB == 6 else dc.SUPERBLOCKS[NB]
    return [(s, b, p) for s in sbs for b in range(NB) for p in dc.POS if s * 32 * NB + 32 * b + p > 64]


def collect_rows(NB):
    return sorted(s * 32 * NB + 32 * b + p for s, b, p in collect_geometry(NB))


@functools.lru_cache(maxsize=None)
def collect_groups(NB):
    """[(R, rows)]: for rings 1 .. 3 the groups of test_gpu_diag_collect.py restricted to rows > 64; ring 6 over the part of the
    grid from 0.15 on (its filler has 9 632 / R bases, and the engine takes 65 000)"""
    if NB != 6:
        return [(R, [f for f in rows if f > 64]) for R, rows in dc.groups_of(NB) if any(f > 64 for f in rows)]
    left, out = collect_rows(6), []
    while left:
        R = max((k * 0.0005 for k in range(300, 600)), key=lambda R: (sum(dc.can_fail_first(f, R) for f in left), R))
        took = [f for f in left if dc.can_fail_first(f, R)]
        assert took
        out.append((R, took))
        left = [f for f in left if f not in took]
    return out


COLLECT_CASES = [(NB, g) for NB in COLLECT_NBS for g in range(len(collect_groups(NB)))]


def true_lengths(NB):
    """about one true pair per superblock: the diagonal ends on the first row of superblocks 1 .. 3, in the last block of
    superblock 2, and (rings 1 and 2) on the first row behind the ring wrap"""
    RB = 32 * NB
    ms = {RB + 1, 2 * RB + 1, 3 * RB - 1, 3 * RB + 1, 4 * RB + 1} | ({64 * RB + 1} if NB <= 2 else set())
    return sorted(m for m in ms if m > COLLECT_MIN)            # (shorter ones do not pass the gate)


@functools.lru_cache(maxsize=None)
def collect_set(NB, g):
    """The reads of group g of ring NB.  Every pair is a read x and its copy y + 16 unrelated bases (so that x is the shorter
    side: the copy as the target puts the target on the rows); planted[k] = dict(x, y: read indices, kind, f, m)."""
    R, rows = collect_groups(NB)[g]
    S = Set(12100 + 10 * NB + g)
    pairs = []

    def add(x, y, **meta):
        pairs.append(dict(x=S.add(x), y=S.add(y + S.rand(16)), **meta))

    for f in rows:
        for last in (True, False):
            m = f if last else f + dc.BEHIND
            add(*dc.hug_pair(S.rng, m, R, f, f), kind="fail", f=f, m=m)
    for m in (true_lengths(NB) if g == 0 else []):
        add(*dc.hug_pair(S.rng, m, R, 3 * 32 * NB), kind="true", f=0, m=m)
    t_hi = len(S.texts)
    if NB >= 2:                                   # the filler: the first max_dst of the ring's plan row, no target
        S.add(ar.pilot(ar.row_of(*ROW_OF_RING[NB])[0], R, seed=3)[0])
    return case_of(S, f"collect{NB}.{g}", R, 1, COLLECT_MIN, 0, t_hi, planted=pairs, NB=NB)


# ----------------------------------------------------------------------------- B: every plan row
# row -> (R, L): 1 + int(L R) lies in the row and (L + 1) (2 max_dst + 1) within the oracle's cell budget; (6, 8): L is that of
# its given-up pairs, which the reference fails at row 1 601 (the matrix is written as far as that row)
STAGE_ROWS = {(1, 1): (0.30, 1000), (1, 2): (0.90, 1540), (2, 2): (0.90, 2800), (2, 3): (0.90, 3300), (2, 4): (0.975, 4180),
              (3, 4): (0.975, 5000), (3, 6): (0.975, 5560), (4, 6): (0.975, 7500), (4, 8): (0.975, 8320), (6, 8): (0.975, 11000)}
STAGE_MIN = 64
STAGE_HEAD = 40
GIVEN_UP_ROWS = ((2, 4), (4, 8), (6, 8))
RC_ROWS = ((2, 4), (4, 8))
PARKS_FIRST = ((3, 6), (4, 8))              # rows whose first target is the "w1+1" read: a sample of one item then starts the rest wider


def planted_costs(row):
    """{name: cost} of the planted pairs of a plan row"""
    R, L = STAGE_ROWS[row]
    md = ar.max_dst_of(L, L, R)
    mid = nb_mid_of(*row)
    w1 = ar.bv_pass1_w(md, row[0])
    if row == (6, 8):
        return {}                                 # (no accepted cost at or above its window within the budget: align_rings.py)
    out = {"w1": w1 if w1 < md else md - 5}    # (a window that is the whole band: a few below the largest cost the band accepts)
    if w1 + 1 <= md - 1:
        out["w1+1"] = w1 + 1
    if mid:
        w_mid = ar.bv_pass1_w(md, mid)
        out["w_mid"] = w_mid
        if w_mid + 1 <= md - 1:
            out["w_mid+1"] = w_mid + 1
    return out


def two_letter(S, L):
    """a read of L bases: 40 random bases that begin with G, then A / C, the last 16 behind one G: neither probe of it has
    a key that the A / C text of another read holds"""
    return b"G" + S.rand(STAGE_HEAD - 1) + AC[S.rng.randint(0, 2, L - STAGE_HEAD - 16)].tobytes() + b"G" + AC[S.rng.randint(0, 2, 15)].tobytes()


def plant(x: bytes, cost: int, R: float, lo: int = STAGE_HEAD, tail: int = 0) -> bytes:
    """x with `cost` bases replaced by G / T (T where x has its G): the last one, and the others evenly over
    [lo, len - 1 - tail), so spaced that cost(i, i) <= i R at every row"""
    L = len(x)
    room = L - 1 - tail - lo
    assert 2 <= cost <= room + 1
    at = [lo + (k * room) // (cost - 1) for k in range(cost - 1)] + [L - 1]
    assert len(set(at)) == cost and all(k + 1 <= (i + 1) * R for k, i in enumerate(at))
    y = bytearray(x)
    for k, i in enumerate(at):
        assert y[i] in b"ACG"
        y[i] = b"T"[0] if y[i] == b"G"[0] else b"GT"[k & 1]
    return bytes(y)


def given_up(S, L):
    """a read and one that shares its 40-base head and no base behind it: cost(i, i) = i - 40"""
    x = two_letter(S, L)
    return x, x[:STAGE_HEAD] + GT[S.rng.randint(0, 2, L - STAGE_HEAD)].tobytes()


@functools.lru_cache(maxsize=None)
def stage_set(row):
    """The reads of a plan row: targets first -- the planted reads x, then the short reads -- and behind the target range the
    copies y, queries only.  long[name] = (x, y) read indices."""
    R, L = STAGE_ROWS[row]
    S = Set(12300 + 10 * row[0] + row[1])
    xs, long = [], {}
    for name, cost in planted_costs(row).items():
        x = two_letter(S, L)
        xs.append((name, x, plant(x, cost, R)))
    if row in GIVEN_UP_ROWS:
        for k in range(2 if row == (6, 8) else 1):
            xs.append((f"given_up{k}",) + given_up(S, L))
    if row in PARKS_FIRST:
        xs.sort(key=lambda e: e[0] != "w1+1")
    for name, x, _ in xs:
        long[name] = [S.add(x)]
    short = []
    for k, m in enumerate((100, 333, 590)):                   # short true pairs, both sides targets
        x = S.rand(m)
        short.append((S.add(x), S.add(ar.mutate(S.rng, x, 0.08) + S.rand(20 * k), query=True)))
    for m in (200, 450):                                      # ... and pairs that share a head and nothing else
        w = S.window()
        short.append((S.add(w + S.rand(m)), S.add(w + S.rand(m + 30), query=True)))
    t_hi = len(S.texts)
    for name, _, y in xs:
        long[name].append(S.add(y, query=True))
    return case_of(S, f"stage{row}", R, 1, STAGE_MIN, 0, t_hi, long={k: tuple(v) for k, v in long.items()}, short=short, row=row, L=L)


# ----------------------------------------------------------------------------- C: where a parked candidate sits
PARK_R, PARK_L, PARK_REGION = 0.90, 1800, 256
PARK_CASES = ("slot0", "slot63", "slot64", "straddle", "second_narrow", "two_in_item")


def park_cost():
    md = ar.max_dst_of(PARK_L, PARK_L, PARK_R)
    return ar.bv_pass1_w(md, 1) + 1


@functools.lru_cache(maxsize=None)
def parked_set(name):
    """One target T -- 256 random bases, then A / C -- and its queries in index order: `one` = T's 16 bases at a position
    of its own and nothing of T behind them (one candidate), `two` = 48 bases of T from a position of its own (with two
    trials its probe j = 1 is a second candidate), and planted copies of T (cost: one above ring 1's window), whose place
    in T's list is the number of candidates in front of them.  parked = the read indices of the planted copies."""
    S = Set(12500 + PARK_CASES.index(name))
    mt, om = (2, 32) if name == "straddle" else (1, 16 if name == "second_narrow" else 32)
    T = bytearray(b"G" + S.rand(PARK_REGION - 1) + AC[S.rng.randint(0, 2, PARK_L - PARK_REGION)].tobytes())
    lead = b""
    if name == "straddle":                        # T + T[0:15] once more, 20 bases before T's end: a candidate of 20 rows,
        lead = b"T"                               # (and no second copy of T[0:16] one base on)
        T[PARK_L - 20:PARK_L - 4] = lead + bytes(T[0:15])
        T[PARK_L - 4] = b"C"[0] if T[15] == b"A"[0] else b"A"[0]
    if name == "second_narrow":                   # T's head window once more there: the run's second candidate, decided at once
        T[PARK_L - 20:PARK_L - 4] = bytes(T[0:16])
    T = bytes(T)
    S.add(T, "T")
    nxt = [48]

    def short(kind, n=1):
        for _ in range(n):
            p = nxt[0]
            nxt[0] += 2
            if kind == "one":
                S.add(T[p:p + 16] + S.other(T[p + 16:p + 17]) + S.rand(47), query=True)
            else:
                S.add(T[p:p + 48] + S.rand(16), query=True)

    parked = []

    def copy():
        parked.append(S.add(lead + plant(T, park_cost() + len(parked), PARK_R, PARK_REGION, tail=24), query=True))

    if name == "slot0":
        copy(), short("two", 70)
    elif name in ("slot63", "slot64", "second_narrow"):
        short("two", 64 if name == "slot64" else 63), copy(), short("two", 10)
    elif name == "straddle":                      # 31 queries of two candidates and one of one: 63 slots
        short("two", 31), short("one"), copy(), short("two", 6)
    else:
        short("two", 10), copy(), short("two", 29), copy(), short("two", 20)
    return case_of(S, f"parked:{name}", PARK_R, mt, om, 0, 1, parked=parked)
