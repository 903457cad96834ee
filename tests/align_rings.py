"""The launch plan of the bit-vector aligner restated from the constants of align_bitvec.h, and deterministic inputs that put
a batch into a chosen ring size (NB, 32-row blocks per lane) and at the edges of its windows.  No GPU in here: the CPU file
(test_align_rings_cpu.py) proves every input's regime from the oracle and these constants, the GPU file
(test_gpu_align_rings.py) compares the kernels with the oracle on the same inputs.

How a ring is forced: make_plan (pba_host.h) sizes the ring from the LARGEST max_dst of a call and every pair of the launch
runs in it, so one "pilot" pair -- two unrelated sequences that fail the reference's check within the first rows -- puts a
few hundred short pairs through NB = 3, 4, 6.  Only the reference-band launch needs pairs that are long themselves."""
import os
import re

import numpy as np

from conftest import ROOT

HDR = os.path.join(ROOT, "pacbioassembly_amd", "csrc", "align_bitvec.h")
ALPHA = np.frombuffer(b"ACGT", np.uint8)
PBA_A_BACKWARD, PBA_B_BACKWARD = 1, 2


# ----------------------------------------------------------------------------- the header's constants
def _src() -> str:
    with open(HDR) as f:
        return f.read()


def _define(name: str) -> int:
    m = re.search(r"^#define[ \t]+%s[ \t]+(\d+)\b" % name, _src(), re.M)
    assert m, f"#define {name} <number> not found in align_bitvec.h: the plan of this file is computed from it"
    return int(m.group(1))


def _max_span():
    m = re.search(r"bv_max_span\(int nb\)\s*\{\s*return (\d+) \* nb \+ (\d+);", _src())
    assert m, "bv_max_span(int nb) { return A * nb + B; } not found in align_bitvec.h"
    return int(m.group(1)), int(m.group(2))


def _instantiated():
    """The ring sizes bv_nb_for_span can answer, from its own return expression (nb <= 4 ? nb : nb <= 6 ? 6 : nb <= 8 ? 8 : 0)
    and the divisor / offset of its `need`."""
    s = _src()
    m = re.search(r"bv_nb_for_span\(int span\)\s*\{\s*const int need = \(span - (\d+) \+ (\d+)\) / (\d+);", s)
    assert m, "bv_nb_for_span: const int need = (span - B + A-1) / A; not found in align_bitvec.h"
    off, rnd, div = map(int, m.groups())
    r = re.search(r"return nb <= (\d+) \? nb : ((?:\(nb <= \d+ \? \d+ : )+)0\)+;", s)
    assert r, "bv_nb_for_span: return nb <= K ? nb : (nb <= X ? X : ... 0); not found in align_bitvec.h"
    steps = [(int(a), int(b)) for a, b in re.findall(r"nb <= (\d+) \? (\d+)", r.group(2))]
    assert steps and all(a == b for a, b in steps), steps
    return list(range(1, int(r.group(1)) + 1)) + [b for _, b in steps], off, rnd, div


BAND_NUM = _define("PBA_BV_BAND_NUM")
BAND_DEN = _define("PBA_BV_BAND_DEN")
MAX_NB = _define("PBA_BV_MAX_NB")
SPAN_MUL, SPAN_ADD = _max_span()
RINGS, _NEED_OFF, _NEED_RND, _NEED_DIV = _instantiated()
assert (_NEED_OFF, _NEED_RND, _NEED_DIV) == (SPAN_ADD, SPAN_MUL - 1, SPAN_MUL), "bv_nb_for_span is not the inverse of bv_max_span"
assert RINGS[-1] == MAX_NB


def bv_max_span(nb):
    return SPAN_MUL * nb + SPAN_ADD


def bv_nb_for_span(span):
    need = max(1, (span - SPAN_ADD + SPAN_MUL - 1) // SPAN_MUL) if span > SPAN_ADD else 1
    for nb in RINGS:
        if nb >= need:
            return nb
    return 0


def bv_first_w(md):
    return min(md, max(md // 2, md * BAND_NUM // BAND_DEN) + 1)


def bv_first_wl(md):
    return min(md, bv_first_w(md) // 2 + 1)


def bv_full_wl(md):
    return md // 2 + 1 if md // 2 + 1 < md else md


def bv_pass1_w(md, nb):
    return min(md, max(bv_first_w(md), (bv_max_span(nb) - 4) * 2 // 3))


def bv_pass1_wl(md, nb):
    return min(md, bv_pass1_w(md, nb) // 2 + 1)


def bitvec_supports(md):
    return bv_nb_for_span(bv_full_wl(md) + md) != 0


def nb1(md):
    """ring of the narrow first launch of a batch whose largest max_dst is md (make_plan); 0: row sweep"""
    return bv_nb_for_span(bv_first_wl(md) + bv_first_w(md)) if bitvec_supports(md) else 0


def nb2(md):
    """ring of the reference-band re-run"""
    return bv_nb_for_span(bv_full_wl(md) + md) if bitvec_supports(md) else 0


def max_dst_of(la, lb, R):
    """text_clip (pba_host.h): the band of seq_aligner.h:94-102, same FP64 product and truncation"""
    return 1 + int((la if lb >= la else lb) * R)


def plan_rows():
    """[(md_lo, md_hi, nb1, nb2)] over max_dst = 1 .. the last supported one, from the constants alone."""
    rows, md = [], 1
    while bitvec_supports(md):
        key, lo = (nb1(md), nb2(md)), md
        while bitvec_supports(md + 1) and (nb1(md + 1), nb2(md + 1)) == key:
            md += 1
        rows.append((lo, md, key[0], key[1]))
        md += 1
    return rows


def row_of(n1, n2):
    for lo, hi, a, b in plan_rows():
        if (a, b) == (n1, n2):
            return lo, hi
    raise KeyError((n1, n2))


def first_window(md):
    """(w, wl) of the narrow launch of a batch whose largest max_dst is md, for a pair with that max_dst"""
    return bv_pass1_w(md, nb1(md)), bv_pass1_wl(md, nb1(md))


# ----------------------------------------------------------------------------- sequences
def rand_seq(rng, n):
    return ALPHA[rng.randint(0, 4, n)].tobytes()


def mutate(rng, x: bytes, e: float, head: int = 40) -> bytes:
    """a copy of x with substitutions, insertions and deletions at rate e in all, the first `head` bases clean"""
    out = bytearray(x[:head])
    u = rng.rand(len(x))
    for k in range(head, len(x)):
        if u[k] < e / 3:
            out += bytes([ALPHA[rng.randint(4)], x[k]])
        elif u[k] < 2 * e / 3:
            pass
        elif u[k] < e:
            out.append(ALPHA[(int(np.searchsorted(ALPHA, x[k])) + 1 + rng.randint(3)) % 4])
        else:
            out.append(x[k])
    return bytes(out)


def fit(rng, x: bytes, n: int) -> bytes:
    return x[:n] if len(x) >= n else x + rand_seq(rng, n - len(x))


class Batch:
    """Sequences of one set and pairs over it.  meta[q]: what pair q is (kind, m, tag, ...)."""

    def __init__(self):
        self.seqs, self.pairs, self.meta = [], [], []

    def add_seq(self, s: bytes) -> int:
        self.seqs.append(s)
        return len(self.seqs) - 1

    def place(self, rng, text: bytes, back: bool, mod: int):
        """text inside a sequence of its own, random flanks, the accessor's origin at pos % 32 == mod; (seq, pos, len)"""
        org = len(text) - 1 if back and text else 0
        left = (mod - org) % 32 + 32 * int(rng.randint(0, 2))
        s = self.add_seq(rand_seq(rng, left) + text + rand_seq(rng, int(rng.randint(0, 70))))
        return s, left + org, len(text)

    def add_pair(self, a, b, fa, fb, **meta):
        self.pairs.append((a[0], a[1], a[2], b[0], b[1], b[2], (PBA_A_BACKWARD if fa else 0) | (PBA_B_BACKWARD if fb else 0)))
        self.meta.append(meta)

    def elems(self, q):
        """the two accessors' elements in accessor order (a backward accessor reads towards lower addresses)"""
        sa, pa, la, sb, pb, lb, fl = self.pairs[q]
        a = self.seqs[sa][pa - la + 1:pa + 1][::-1] if fl & 1 and la else self.seqs[sa][pa:pa + la]
        b = self.seqs[sb][pb - lb + 1:pb + 1][::-1] if fl & 2 and lb else self.seqs[sb][pb:pb + lb]
        assert len(a) == la and len(b) == lb
        return a, b

    def with_pilot(self, pil):
        """a new batch: the pilot's two sequences inserted after sequence 0 (sequence 0 and the last one stay where they are),
        the pilot pair first"""
        o = Batch()
        o.seqs = self.seqs[:1] + [pil[0], pil[1]] + self.seqs[1:]
        sh = lambda s: s + 2 if s >= 1 else s
        o.pairs = [(1, 0, len(pil[0]), 2, 0, len(pil[1]), 0)] + [(sh(p[0]), p[1], p[2], sh(p[3]), p[4], p[5], p[6]) for p in self.pairs]
        o.meta = [dict(kind="pilot", tag="pilot")] + list(self.meta)
        return o

    def subset(self, keep):
        o = Batch()
        o.seqs = self.seqs
        o.pairs = [self.pairs[q] for q in keep]
        o.meta = [self.meta[q] for q in keep]
        return o


_ORACLE_CACHE = {}


def expected(oracle, batch: Batch, R: float):
    """the oracle's answers for a batch, computed once per (inputs, R) in a session and shared by every test"""
    out = []
    for q in range(len(batch.pairs)):
        a, b = batch.elems(q)
        key = (a, b, R)
        if key not in _ORACLE_CACHE:
            _ORACLE_CACHE[key] = oracle.align(a, b, R, want_ops=True)
        out.append(_ORACLE_CACHE[key])
    return out


# ----------------------------------------------------------------------------- pilot
def pilot(md_target: int, R: float, seed: int = 1):
    """two unrelated sequences of equal length whose max_dst is md_target: fails the reference's check within the first rows"""
    la = int(np.ceil((md_target - 1) / R))
    while max_dst_of(la, la, R) < md_target:
        la += 1
    while max_dst_of(la - 1, la - 1, R) >= md_target:
        la -= 1
    assert max_dst_of(la, la, R) == md_target and la <= 65000, (md_target, R, la)
    rng = np.random.RandomState(9000 + seed)
    return rand_seq(rng, la), rand_seq(rng, la)


# ----------------------------------------------------------------------------- short pairs at the edges of a ring
def edge_ms(NB):
    RB = 32 * NB
    return sorted({1, 10, 11, 12, 31, 32, 33, 63, 64, 65, RB - 1, RB, RB + 1, 2 * RB, 2 * RB + 1})


MODS = (0, 1, 31)


def edge_pairs(NB: int, R: float) -> Batch:
    """Short pairs (all under 600 bases) whose boundaries are those of ring NB (RB = 32 NB rows per superblock): every m of
    edge_ms, n - m in {0, 1, max_dst - 1, max_dst, max_dst + 40}, each as a true pair (a copy mutated at R / 2 behind a clean
    40-base head) and as an unrelated one; which side is longer, the four direction combinations and the origins' pos % 32
    in {0, 1, 31} are drawn per pair (the CPU test asserts that all occur).  Then the placements: a pair on sequence 0 with no
    left flank, backward accessors on sequence 0 whose first 32-element fetch reaches below base 0, a pair right after a
    zero-length sequence, and a pair on the last sequence of the set running to its last base."""
    assert R <= 0.45
    rng = np.random.RandomState(4100 + NB)
    B = Batch()
    head = rand_seq(rng, 70)                                # sequence 0: no flank on the left
    B.add_seq(head)
    for m in edge_ms(NB):
        md = 1 + int(m * R)
        for delta in sorted({0, 1, md - 1, md, md + 40}):
            for kind in ("true", "unrel"):
                x = rand_seq(rng, m)
                y = fit(rng, mutate(rng, x, R / 2), m + delta) if kind == "true" else rand_seq(rng, m + delta)
                a_longer = bool(rng.randint(2))
                a, b = (y, x) if a_longer else (x, y)
                fa, fb = bool(rng.randint(2)), bool(rng.randint(2))
                ma, mb = MODS[rng.randint(3)], MODS[rng.randint(3)]
                B.add_pair(B.place(rng, a[::-1] if fa else a, fa, ma), B.place(rng, b[::-1] if fb else b, fb, mb), fa, fb,
                           kind=kind, m=m, delta=delta, a_longer=a_longer, amod=ma, bmod=mb, tag=f"m{m}+{delta}:{kind}")
    # backward accessors from the first bases of sequence 0 (pos < 31: the 32-element fetch starts below base 0), forward from base 0
    for m in (1, 11, 12, 31, 33, 65):
        x = head[:m][::-1]                                  # the elements of a backward accessor at pos m - 1
        y = fit(rng, mutate(rng, x, R / 2), m + int(rng.randint(0, 3)))
        B.add_pair((0, m - 1, m), B.place(rng, y, False, MODS[m % 3]), True, False, kind="true", m=m, place="below0", tag=f"below0:m{m}")
        B.add_pair(B.place(rng, y[::-1], True, MODS[m % 3]), (0, m - 1, m), True, True, kind="true", m=m, place="below0", tag=f"below0:b:m{m}")
    y = fit(rng, mutate(rng, head[:65], R / 2), 70)
    B.add_pair((0, 0, 65), B.place(rng, y, False, 1), False, False, kind="true", m=65, place="first", tag="first:fwd")
    # after a zero-length sequence (its own accessors: length 0 at pos 0)
    z = B.add_seq(b"")
    x = rand_seq(rng, 64)
    s = B.add_seq(x)
    y = fit(rng, mutate(rng, x, R / 2), 66)
    B.add_pair((s, 0, 64), B.place(rng, y, False, 31), False, False, kind="true", m=64, place="after_empty", tag="after_empty:fwd")
    B.add_pair((s, 63, 64), B.place(rng, fit(rng, mutate(rng, x[::-1], R / 2), 64)[::-1], True, 0), True, True, kind="true", m=64,
               place="after_empty", tag="after_empty:back")
    B.add_pair((z, 0, 0), (s, 0, 12), False, False, kind="unrel", m=0, place="empty", tag="empty:a")
    # the last sequence of the set: forward to its last base (the fetches past it read the slack), backward from it
    x = rand_seq(rng, 97)
    ya = B.place(rng, fit(rng, mutate(rng, x, R / 2), 97 + 20), False, 0)
    yb = B.place(rng, fit(rng, mutate(rng, x[::-1], R / 2), 97)[::-1], True, 1)
    last = B.add_seq(x)
    B.add_pair(ya, (last, 0, 97), False, False, kind="true", m=97, place="last", tag="last:fwd")
    B.add_pair((last, 96, 97), yb, True, True, kind="true", m=97, place="last", tag="last:back")
    B.add_pair((last, 64, 33), (last, 32, 33), False, True, kind="unrel", m=33, place="last", tag="last:tail")
    assert last == len(B.seqs) - 1 and max(len(s) for s in B.seqs) < 600 + 64 + 70
    assert all(p[2] < 600 and p[5] < 600 for p in B.pairs)
    return B


# ----------------------------------------------------------------------------- rows past 64 superblocks
WRAP_EXTRA = (-1, 0, 1, 33)


def wrap_pairs(NB: int, R: float = 0.30) -> Batch:
    """True pairs whose longer side has 64 RB - 1, 64 RB, 64 RB + 1 and 64 RB + 33 rows (RB = 32 NB): at 64 RB + 1 lane 0 takes
    its second superblock.  The shorter side is 24 bases shorter, so the clip (shorter + max_dst) leaves the row count alone;
    the last one is swapped so that `a` is the longer side, and one runs backward.  (The wrap does not depend on R; 0.30 keeps
    the pilot that forces rings 2 .. 6 within the engine's sequence limit.)"""
    rng = np.random.RandomState(5200 + NB)
    B = Batch()
    for k, extra in enumerate(WRAP_EXTRA):
        n = 64 * 32 * NB + extra
        x = rand_seq(rng, n - 24)
        y = fit(rng, mutate(rng, x, 0.06), n)
        back = k == 1
        a, b = (y, x) if k == 3 else (x, y)
        B.add_pair(B.place(rng, a[::-1] if back else a, back, MODS[k % 3]), B.place(rng, b[::-1] if back else b, back, MODS[(k + 1) % 3]),
                   back, back, kind="true", rows=n, a_longer=k == 3, tag=f"wrap{NB}:{extra:+d}")
    return B


# ----------------------------------------------------------------------------- the certificate's adversaries
EXC_R = 0.30


def excursion_ds(w, wl):
    return [wl - 1, wl, wl + 1, wl + 40, w - 1, w, w + 1]


def excursion_pairs(md: int, w: int, wl: int) -> Batch:
    """Pairs whose cheapest path leaves the diagonal by d and (where the reference can still accept that) returns: the columns
    of the sweep are the shorter sequence, the rows the longer one, and row i sees the columns [i - w, i + wl].

    side "wl" (columns ahead of rows): the ROW sequence lacks a block of d bases at p1 and carries d random bases at p2; the
             path runs d columns ahead between the two and pays 2 d, so the reference accepts it only while 2 d <= m R:
             d in {wl - 1, wl, wl + 1, wl + 40}.  (d around w cannot return: 2 (w - 1) > m R in this plan row.)
    side "w"  (rows ahead of columns, towards the free end): the COLUMN sequence lacks the block.  d in {wl - 1 .. wl + 40}
             returns at p2 like the other side; d in {w - 1, w, w + 1} stays out and ends at the free end (m + d, m), cost d.
    Each one in both orders of the pair (a = rows, a = columns), once as the reference accepts it and once ("late") with a
    tail that shares no base with the other side's, so that the reference fails at a row fr with fr R >= 2 wl + 2.  md: the max_dst every pair is to have
    (shorter side m = the first length with that max_dst); p1 is late enough for the diagonal cells inside the excursion to
    pass cost(i,i) <= i R (they cost min(2 d, ~0.55 (i - p1)))."""
    R = EXC_R
    m = int(np.ceil((md - 1) / R))
    while max_dst_of(m, m + 1, R) < md:
        m += 1
    assert max_dst_of(m, m + 1, R) == md
    rng = np.random.RandomState(6300)
    B = Batch()
    for side in ("wl", "w"):
        for d in excursion_ds(w, wl):
            returns = 2 * d + 160 <= int(m * R)
            if side == "wl" and not returns:
                continue
            assert d < md
            for late in (False, True):
                for a_rows in (False, True):
                    if returns:
                        # block out at p1, d random bases in at p2; the stretch between costs more on the diagonal than 2 d
                        # (... and more than p2 R: a sweep that cannot follow the path out fails its own diagonal check in between)
                        p2 = m - 260 if not late else m - 1800
                        p1 = p2 - max(4 * d, int(0.62 * p2))
                        assert p1 > 2000, (d, p1)
                        x = rand_seq(rng, m + 30)
                        if late:                                        # from 60 bases past the return on: no base in common
                            k = len(x) - p2 - 60
                            x = x[:p2 + 60] + np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, k)].tobytes()
                        y = x[:p1] + x[p1 + d:p2] + rand_seq(rng, d) + x[p2:]
                        if late:
                            y = y[:p2 + 60] + np.frombuffer(b"GT", np.uint8)[rng.randint(0, 2, k)].tobytes()
                        lack, full = y, x
                        # the sequence that lacks the block is the rows for side wl, the columns for side w
                        rows, cols = (lack, full[:m]) if side == "wl" else (full, lack[:m])
                    else:
                        # side w only: the columns lack d bases at p1 and never get them back; ends at the free end
                        p1 = int(m / 1.8) if not late else int(m / 2.6)
                        x = rand_seq(rng, m + md + 30)
                        rows, cols = x, x[:p1] + x[p1 + d:m + d]
                    assert len(cols) == m and len(rows) > m
                    a, b = (rows, cols) if a_rows else (cols, rows)
                    B.add_pair(B.place(rng, a, False, MODS[d % 3]), B.place(rng, b, False, MODS[(d + 1) % 3]), False, False,
                               kind="late" if late else "accept", side=side, d=d, returns=returns, a_rows=a_rows,
                               tag=f"exc:{side}:d{d}:{'late' if late else 'ok'}:{'a' if a_rows else 'b'}rows")
    return B


def script_excursion(ops, a_rows: bool):
    """(max of columns - rows, max of rows - columns) along an edit script of the reference (1 MATCH, 2 INSERT: b advances,
    3 DELETE: a advances); rows are a if a_rows else b"""
    ops = np.asarray(ops, np.int64)
    step = np.where(ops == 2, 1, np.where(ops == 3, -1, 0))            # j - i in (a, b) coordinates
    off = np.cumsum(step if a_rows else -step)                        # columns - rows
    return int(max(off.max(initial=0), 0)), int(max(-off.min(initial=0), 0))


# ----------------------------------------------------------------------------- pairs for the reference-band launch
# One entry per plan row with nb2 in {3, 4, 6, 8}: (nb1, nb2) -> (R, m, divergences of its pairs, two_letter).  A pair is a
# (m bases) against a mutated copy behind a clean head, with tail enough for the clip; the oracle's matrix is
# (m + 1) (2 max_dst + 1) cells, held to that of the suite's 15 kb pairs at R = 0.30 (15 001 x 9 003).  R and m put max_dst
# into the row, the divergence puts the cost above the row's first-pass w.  Copies mutated with indels level off near 0.4
# edits per base, so the rows whose w is beyond that for any m within the matrix limit (w = 5 416) are two_letter: a over
# {A, C}, its copy mutated at 0.10 with indels and then a share e of its bases replaced by G / T, which cost one edit each
# whatever the path does.  Row (6, 8) has no entry: a cost above its w = 8 104 needs m > 8 104 at max_dst >= 9 632, a matrix
# 16 % over the limit; ring 8 as the re-run is the same instantiation under row (4, 8), whose pairs also have the
# 64 * 256 + 1 rows of a second superblock for lane 0.
WIDE = {
    (2, 3): (0.40, 9000, (0.44, 0.47), False),
    (2, 4): (0.42, 10000, (0.38, 0.42), False),
    (3, 4): (0.42, 12000, (0.46, 0.48), False),
    (3, 6): (0.48, 11500, (0.48, 0.52), False),
    (4, 6): (0.90, 8200, (0.66, 0.70), True),
    (4, 8): (0.975, 8320, (0.66, 0.70), True),
}
ORACLE_CELL_BUDGET = 15001 * 9003


def wide_pairs(row) -> tuple:
    """(batch, R) for a plan row (nb1, nb2): pairs the reference accepts with cost above the row's first-pass w; the second
    one has `a` as the longer side."""
    R, m, es, two_letter = WIDE[row]
    md = max_dst_of(m, m + 1, R)
    lo, hi = row_of(*row)
    assert lo <= md <= hi, (row, md, lo, hi)
    assert (m + 1) * (2 * md + 1) <= ORACLE_CELL_BUDGET, (row, (m + 1) * (2 * md + 1))
    rng = np.random.RandomState(7400 + 10 * row[0] + row[1])
    B = Batch()
    for k, e in enumerate(es):
        if two_letter:
            x = np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, m)].tobytes()
            y = bytearray(mutate(rng, x, 0.10))
            u = rng.rand(len(y))
            for i in range(40, len(y)):
                if u[i] < e:
                    y[i] = b"GT"[rng.randint(2)]
            y = bytes(y)
        else:
            x = rand_seq(rng, m)
            y = mutate(rng, x, e)
        y = (y + rand_seq(rng, md + 50))[:m + md + 40]
        a, b = (y, x) if k == 1 and not big_as_a(m, md) else (x, y)
        B.add_pair(B.place(rng, a, False, MODS[k % 3]), B.place(rng, b, False, MODS[(k + 1) % 3]), False, False,
                   kind="wide", rows=m + md, tag=f"wide{row}:e{e}")
    return B, R


def big_as_a(m, md):
    """with the longer side as a the reference's matrix has m + max_dst + 1 rows: over the limit?"""
    return (m + md + 1) * (2 * md + 1) > ORACLE_CELL_BUDGET
