"""Hand-built inputs for the vote-box core (csrc/consensus.h: k_cons_elect, VoteSink, cons_yield, cons_bump, k_cons_evolve;
csrc/pba_pileup.hip: pile_block_count / pile_block_write), each one placed on an edge of that code: the 1 024-box chunk of
evolve counted from `pre`, the 64-op chunk of elect, the 64-vote gather of VoteSink, the 256-box step and the 64-lane ballot
of the pile-up write, the strict majority of cons_yield and the 16-bit counters.  No GPU in here: test_votebox_inputs_cpu.py
proves from the oracle what each input is, test_gpu_votebox.py runs the kernels on them, tests/golden/make_golden.py runs
the reference itself on those the reference is defined on.

A State is a reference text (a part of it prepended / appended with weight 1, the rest given to the constructor with
`weight`) and a list of edit scripts.  Box indices are counted from `pre`; a script's pos is counted from `beg`, as elect
takes it.  Evolve states are planted with one-op scripts:
    forward  [MATCH x]  at a box:  sel[x]++, tot++
    forward  [DELETE]   at a box:  tot++
    backward [INSERT x] at a box:  sup[x]++ on that box and nothing else
A plain model of elect and evolve (model_boxes, model_evolve) says what every state holds and which output absorbs which
deleted box; the CPU test holds the oracle to it, so the regime a state is named for is asserted, not assumed."""
import functools
import hashlib
from collections import namedtuple
from dataclasses import dataclass, field

import numpy as np

from cons_scenarios import votes_digest
from map_ref import rand_text
from pacbioassembly_amd import engine as eng

MATCH, INSERT, DELETE = 1, 2, 3
CHUNK = 1024            # boxes per sweep step of k_cons_evolve
WAVE = 64               # ops per ballot of k_cons_elect, votes per gather of VoteSink
STEP = 256              # boxes per step of pile_block_write
PRE = 37                # boxes prepended in the prepended form of an evolve state: the chunk grid starts at pre, not at beg
MAX_LEN = 8192          # of every consensus object: above every box count here, so the evolved text fits (3 * max_len arrays)
R = 0.30
OVERLAP_MIN = 64

Script = namedtuple("Script", "pos fwd ops vals nedit")     # ops / vals fill the script's slot; the first nedit of them count


def script(pos, fwd, ops, vals, slot=None):
    ops = np.asarray(ops, np.uint8)
    vals = bytes(vals)
    assert len(vals) == ops.size
    return Script(int(pos), bool(fwd), ops, vals, ops.size if slot is None else int(slot))


@dataclass
class State:
    name: str
    base: bytes                 # the constructor's text, boxes of `weight`
    weight: int = 1
    pre: bytes = b""            # prepended / appended before the scripts vote: boxes of weight 1
    app: bytes = b""
    scripts: list = field(default_factory=list)
    marks: dict = field(default_factory=dict)      # what the state is named for (test_votebox_inputs_cpu.py asserts it)
    max_len: int = MAX_LEN

    @property
    def text(self) -> bytes:
        return self.pre + self.base + self.app

    @property
    def n(self) -> int:
        return len(self.pre) + len(self.base) + len(self.app)

    @property
    def ref_safe(self) -> bool:
        """The reference itself is defined on this state: every vote inside [pre, post) (that covers a forward INSERT on
        the first box, which targets pre - 1) and no counter beyond 16 bits."""
        return all(((t >= 0) & (t < self.n)).all() for t in (vote_targets(self, s) for s in self.scripts))


# ----------------------------------------------------------------------------- the model
def vote_targets(st: State, sc: Script) -> np.ndarray:
    """The box (counted from pre, not clipped) each of the script's nedit ops votes on (apply_edits, ref_seq.h:25-41)."""
    ops = sc.ops[:sc.nedit]
    adv = (ops == MATCH) | (ops == DELETE)
    before = np.cumsum(adv) - adv                             # advancing ops before op k
    it = sc.pos + len(st.pre) + (before if sc.fwd else -before)
    return np.where((ops == INSERT) & sc.fwd, it - 1, it).astype(np.int64)


def advancing_per_chunk(sc: Script):
    """MATCH + DELETE ops in each run of 64 ops: what k_cons_elect's ballot counts and carries in `done`."""
    ops = sc.ops[:sc.nedit]
    adv = (ops == MATCH) | (ops == DELETE)
    return [int(adv[k:k + WAVE].sum()) for k in range(0, ops.size, WAVE)]


def initial_boxes(st: State):
    n = st.n
    sel = np.zeros((n, 4), np.int64); sup = np.zeros((n, 4), np.int64); tot = np.ones(n, np.int64)
    w = np.ones(n, np.int64)
    w[len(st.pre):len(st.pre) + len(st.base)] = st.weight
    code = np.frombuffer(st.text.translate(bytes.maketrans(b"ACGT", bytes(range(4)))), np.uint8)
    sel[np.arange(n), code] = w
    return sel, sup, tot


def model_boxes(st: State):
    """(sel, sup, tot) after every script of the state has voted, votes outside [0, n) dropped."""
    sel, sup, tot = initial_boxes(st)
    for sc in st.scripts:
        for k, at in enumerate(vote_targets(st, sc)):
            if not 0 <= at < st.n:
                continue
            op = int(sc.ops[k])
            if op == MATCH:
                sel[at, b"ACGT".index(sc.vals[k])] += 1; tot[at] += 1
            elif op == DELETE:
                tot[at] += 1
            else:
                sup[at, b"ACGT".index(sc.vals[k])] += 1
    return sel, sup, tot


def model_evolve(sel, sup, tot):
    """ref_seq::evolve (ref_seq.h:317-349) in plain steps.  Returns (sel, sup, tot, text, src, absorbed): src[k] = (input
    box, 0: the box itself / 1: the box split from its suppliment) of output k; absorbed[box] = the output that took a
    deleted box's selection, or -1 where it was dropped."""
    out, src, absorbed, text = [], [], {}, bytearray()
    for i in range(len(tot)):
        S = 2 * int(sup[i].max()) > int(tot[i])
        V = 2 * int(sel[i].max()) > int(tot[i])
        if V:
            out.append([sel[i].copy(), np.zeros(4, np.int64) if S else sup[i].copy(), int(tot[i])])
            src.append((i, 0)); text.append(b"ACGT"[int(np.argmax(sel[i]))])
        else:
            absorbed[i] = len(out) - 1
            if out:
                out[-1][1] = out[-1][1] + sel[i]
        if S:
            out.append([sup[i].copy(), np.zeros(4, np.int64), int(tot[i])])
            src.append((i, 1)); text.append(b"ACGT"[int(np.argmax(sup[i]))])
    n = len(out)
    s2 = np.array([o[0] for o in out], np.int64).reshape(n, 4)
    p2 = np.array([o[1] for o in out], np.int64).reshape(n, 4)
    t2 = np.array([o[2] for o in out], np.int64)
    return s2, p2, t2, bytes(text), src, absorbed


# ----------------------------------------------------------------------------- driving a consensus object
def build(make, st: State):
    """make(base, weight, max_len) -> an object with prepend / append (OracleCons, RefCons, eng.Consensus)."""
    c = make(st.base, st.weight, st.max_len)
    if st.pre:
        c.prepend(st.pre)
    if st.app:
        c.append(st.app)
    return c


def elect_loop(c, st: State):
    """one script per call (the oracle and the reference take them that way)"""
    for sc in st.scripts:
        c.elect(sc.pos, sc.fwd, sc.ops[:sc.nedit], sc.vals[:sc.nedit])


def elect_batch(c, scripts):
    """Every script in ONE pba_cons_elect call, each in a slot of its own that may be longer than its nedit."""
    import ctypes as C
    n = len(scripts)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([s.ops.size for s in scripts])
    ops = np.concatenate([s.ops for s in scripts] + [np.zeros(1, np.uint8)])
    vals = np.frombuffer(b"".join(s.vals for s in scripts) + b"\0", np.uint8)
    ne = np.array([s.nedit for s in scripts], np.int32)
    pos = np.array([s.pos for s in scripts], np.int32)
    fw = np.array([s.fwd for s in scripts], np.uint8)
    p = lambda a: C.c_void_p(a.ctypes.data)
    c.ctx.check(c.ctx.lib.pba_cons_elect(c.ctx.h, c.h, n, p(pos), p(fw), p(ops), p(vals), p(off), p(ne)), "cons_elect")


def snap(c, cap: int):
    """(sel, sup, tot, extent, text) of any consensus object as it stands"""
    if isinstance(c, eng.Consensus):
        sel, sup, tot, ext = c.dump()
        return sel, sup, tot, list(ext), c.text()
    sel, sup, tot, ext = c.dump(cap)
    return sel, sup, tot, list(ext), c.text(cap)


def stages(c, st: State, rounds: int = 2):
    """The object after its votes and after each of `rounds` evolves in a row (no votes in between: what the first evolve
    absorbed is all the second one finds in those suppliments)."""
    cap = 2 * st.n + 2 * CHUNK + 8
    out = [snap(c, cap)]
    for _ in range(rounds):
        c.evolve()
        cap = 2 * len(out[-1][2]) + 2 * CHUNK + 8
        out.append(snap(c, cap))
    return out


def same_stage(a, b) -> bool:
    return all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3] and a[4] == b[4]


def record(stgs):
    """What tests/golden/votebox.json keeps of a state: extent and digest of the boxes per stage, the text or its hash."""
    def text(t):
        return t.decode() if len(t) <= 48 else "sha256:" + hashlib.sha256(t).hexdigest()[:32]
    return [{"extent": s[3], "votes": votes_digest(s[0], s[1], s[2]), "text": text(s[4])} for s in stgs]


# ----------------------------------------------------------------------------- the planter
class Planter:
    """Puts chosen counters on chosen boxes of a text with one-op scripts, keeping count of what every box holds."""

    def __init__(self, name: str, text: bytes, weight: int = 1, pre_len: int = 0, app_len: int = 0):
        self.st = State(name, text[pre_len:len(text) - app_len], weight, text[:pre_len], text[len(text) - app_len:] if app_len else b"")
        self.sel, self.sup, self.tot = initial_boxes(self.st)
        self.P = pre_len

    def _one(self, box, fwd, op, base):
        self.st.scripts.append(script(box - self.P, fwd, [op], bytes([base])))

    def own(self, box) -> int:
        return self.st.text[box]

    def match(self, box, base=None, times=1):
        base = self.own(box) if base is None else base
        for _ in range(times):
            self._one(box, True, MATCH, base)
        self.sel[box, b"ACGT".index(base)] += times; self.tot[box] += times

    def ignore(self, box, times=1):
        for _ in range(times):
            self._one(box, True, DELETE, 0)
        self.tot[box] += times

    def supply(self, box, base, times=1):
        for _ in range(times):
            self._one(box, False, INSERT, base)
        self.sup[box, b"ACGT".index(base)] += times

    def kill(self, box):
        """ignores until the selection is no majority: the box is deleted"""
        while 2 * self.sel[box].max() > self.tot[box]:
            self.ignore(box)

    def split(self, box, base=ord("T")):
        """supplies of one base until they are a majority: a box splits off"""
        while not 2 * self.sup[box].max() > self.tot[box]:
            self.supply(box, base)

    def mark(self, kind, box, what):
        self.st.marks.setdefault(kind, {})[int(box)] = what


def _text(seed: int, n: int, fixed=()) -> bytes:
    t = bytearray(rand_text(np.random.default_rng(seed), n))
    for at, s in fixed:
        t[at:at + len(s)] = s
    return bytes(t)


FORMS = ("plain", "prepended")
BIG = 2100


def _planter(name, form, n, weight=1, seed=0, fixed=()):
    return Planter(f"{name}/{form}", _text(900 + seed, n, fixed), weight, PRE if form == "prepended" else 0)


def _evolve_states_of(form):
    out = []

    def done(p):
        out.append(p.st)

    # lengths: a split box at the very end, a deleted one at the very start, a few of each in between
    for n in (1, 1023, 1024, 1025, 2048, BIG):
        if n == 1 and form == "prepended":
            continue                                        # one box has no part to prepend
        p = _planter(f"len_{n}", form, n, seed=n)
        rng = np.random.default_rng(n)
        p.split(n - 1); p.mark("yield", n - 1, 2)
        if n > 1:
            p.kill(0); p.mark("yield", 0, 0); p.mark("absorb", 0, None)
            picks = rng.choice(np.arange(1, n - 1), 16, replace=False)
            for b in picks[:8]:
                p.kill(b); p.mark("yield", b, 0)
            for b in picks[8:]:
                p.split(b, b"ACGT"[int(rng.integers(4))]); p.mark("yield", b, 2)
        done(p)
    if form == "plain":
        p = _planter("len_1_deleted", form, 1, seed=77)     # evolves to the empty reference, and that evolves again
        p.kill(0); p.mark("yield", 0, 0); p.mark("absorb", 0, None)
        done(p)
    # a kept-and-split box on either side of a chunk edge: its second output is the first box of the next chunk's range
    for b in (1022, 1023, 1024, 2047):
        p = _planter(f"split_at_{b}", form, BIG, seed=b)
        p.split(b); p.mark("yield", b, 2)
        done(p)
    # a deleted box as the first of a chunk: the output that absorbs it was written by the chunk before
    p = _planter("del_behind_kept", form, BIG, seed=1)
    p.kill(1024); p.mark("yield", 1023, 1); p.mark("yield", 1024, 0); p.mark("absorb", 1024, (1023, 0))
    done(p)
    p = _planter("del_behind_split", form, BIG, seed=2)
    p.split(1023); p.kill(1024)
    p.mark("yield", 1023, 2); p.mark("yield", 1024, 0); p.mark("absorb", 1024, (1023, 1))
    done(p)
    # a deleted box whose own suppliment is a majority: only the box split from it survives, its selection goes to the
    # output before it (none at box 0)
    for b in (0, 1023, 1024):
        p = _planter(f"del_with_supply_at_{b}", form, BIG, seed=10 + b)
        p.kill(b); p.split(b, ord("G"))
        p.mark("yield", b, "split_only"); p.mark("absorb", b, (b - 1, 0) if b else None)
        done(p)
    # twelve deleted boxes across the chunk edge, every base among them: one output absorbs all four counters
    p = _planter("del_run_across_edge", form, BIG, seed=3, fixed=[(1019, b"ACGTTGCAACGT")])
    for b in range(1019, 1031):
        p.kill(b); p.mark("yield", b, 0); p.mark("absorb", b, (1018, 0))
    p.mark("yield", 1018, 1)
    done(p)
    p = _planter("del_run_at_start", form, BIG, seed=4, fixed=[(0, b"ACGTGT")])
    for b in range(6):
        p.kill(b); p.mark("yield", b, 0); p.mark("absorb", b, None)
    done(p)
    # a whole chunk that yields nothing: the carry stands still, and the box behind it is absorbed two chunks back
    p = _planter("chunk_all_deleted", form, BIG, seed=5)
    for b in range(1024, 2049):
        p.kill(b); p.mark("absorb", b, (1023, 0))
    p.mark("yield", 1023, 1); p.mark("yield", 2048, 0); p.mark("yield", 2049, 1)
    done(p)
    p = _planter("chunk0_all_deleted", form, BIG, seed=6)   # ... and with nothing before it to absorb
    for b in range(0, 1025):
        p.kill(b); p.mark("absorb", b, None)
    p.mark("yield", 0, 0); p.mark("yield", 1024, 0); p.mark("yield", 1025, 1)
    done(p)
    # majority ties.  rel 0: 2 * max == tot (not kept / not split), rel 1: 2 * max == tot + 1 (kept / split)
    for w in (1, 3):
        p = _planter(f"ties_w{w}", form, BIG, weight=w, seed=20 + w)
        at = iter(range(100, 400, 3))                       # every case once early in the first chunk, once around its end
        for m, d in ((0, 2 * w - 1), (1, 2 * w), (1, 2 * w - 1), (2, 2 * w), (0, 2 * w - 2), (3, 2 * w + 1)):
            for far in (0, 900):
                b = next(at) + far
                p.match(b, times=m); p.ignore(b, times=d)   # sel = w + m, tot = 1 + m + d
                rel = 2 * (w + m) - (1 + m + d)
                assert rel in (0, 1)
                p.mark("tie", b, ("sel", rel)); p.mark("yield", b, rel)
        for m, s in ((1, 1), (2, 2), (3, 2), (4, 3), (5, 3), (0, 1)):
            for far in (0, 900):
                b = next(at) + far
                p.match(b, times=m); p.supply(b, ord("C"), times=s)   # tot = 1 + m, sup = s
                rel = 2 * s - (1 + m)
                assert rel in (0, 1), (m, s)
                p.mark("tie", b, ("sup", rel)); p.mark("yield", b, 1 + rel)
        if w == 3:                                          # four ignores leave a weight-3 box alive, five delete it
            p.ignore(700, times=4); p.mark("tie", 700, ("sel", 1)); p.mark("yield", 700, 1)
            p.ignore(703, times=5); p.mark("tie", 703, ("sel", 0)); p.mark("yield", 703, 0)
        done(p)
    # weight 0: an unvoted box dies; what evolves is what was voted in
    p = _planter("weight_0", form, 1100, weight=0, seed=30)
    for b in (40, 1023, 1024, 1099):
        p.match(b, times=2); p.mark("yield", b, 1)          # sel 2 of tot 3
    p.match(50); p.mark("yield", 50, 0)                     # sel 1 of tot 2: a tie, dies
    p.supply(60, ord("A")); p.mark("yield", 60, "split_only")
    done(p)
    # winner ties: equal maxima go to the first in ACGT order, T wins only alone (weight 3, so that 3 + 3 votes of tot 4 hold)
    fixed = [(200, b"A"), (203, b"C"), (206, b"G"), (209, b"T"), (1023, b"A"), (1024, b"G")]
    p = _planter("winner_ties_w3", form, BIG, weight=3, seed=31, fixed=fixed)
    for b, other, win in ((200, b"C", b"A"), (203, b"G", b"C"), (206, b"T", b"G"), (1023, b"C", b"A"), (1024, b"T", b"G")):
        p.match(b, other[0], times=3); p.mark("winner", b, ("sel", win)); p.mark("yield", b, 1)
    p.match(209, ord("A"), times=2); p.mark("winner", 209, ("sel", b"T"))
    for b, pair, win in ((300, b"AC", b"A"), (303, b"CG", b"C"), (306, b"GT", b"G"), (309, b"T", b"T"), (1022, b"GT", b"G")):
        for x in pair:
            p.supply(b, x)
        p.mark("winner", b, ("sup", win)); p.mark("yield", b, 2)
    done(p)
    # two evolves in a row: what a kept box absorbed in the first is all its suppliment holds, and splits it in the second
    fixed = [(300, b"ACCC"), (400, b"AGG"), (1023, b"TAAA")]
    p = _planter("two_evolves", form, BIG, seed=32, fixed=fixed)
    p.match(300, times=4)                                   # tot 5: three absorbed C are a majority ...
    for b in (301, 302, 303):
        p.kill(b); p.mark("absorb", b, (300, 0))
    p.match(400, times=4)                                   # ... two absorbed G are not
    for b in (401, 402):
        p.kill(b); p.mark("absorb", b, (400, 0))
    for b in (1024, 1025, 1026):                            # tot 1: absorbed across the chunk edge
        p.kill(b); p.mark("absorb", b, (1023, 0))
    p.st.marks["second_split"] = {300: b"C", 1023: b"A"}
    p.st.marks["second_kept_whole"] = {400: True}
    done(p)
    return out


@functools.lru_cache(maxsize=None)
def evolve_states():
    return tuple(s for form in FORMS for s in _evolve_states_of(form))


# ----------------------------------------------------------------------------- elect scripts
ELECT_PRE, ELECT_BASE, ELECT_APP = 50, 400, 50
ELECT_N = ELECT_PRE + ELECT_BASE + ELECT_APP
ELECT_LENS = (63, 64, 65, 127, 128, 129, 200)


def _elect_state(name, scripts, weight=1):
    t = _text(1500, ELECT_N)
    return State("elect/" + name, t[ELECT_PRE:ELECT_PRE + ELECT_BASE], weight, t[:ELECT_PRE], t[ELECT_PRE + ELECT_BASE:], scripts)


def mixed_script(rng, box, fwd, length, first=MATCH, heads=None):
    """A script of `length` ops, half MATCH, a quarter INSERT, a quarter DELETE; `heads`: the op at index 64 and 128."""
    ops = rng.choice(np.array([MATCH, MATCH, INSERT, DELETE], np.uint8), length)
    if length:
        ops[0] = first
    for k in (WAVE, 2 * WAVE):
        if heads is not None and k < length:
            ops[k] = heads
    vals = np.where(ops == DELETE, 0, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)]).astype(np.uint8)
    return script(box - ELECT_PRE, fwd, ops, vals.tobytes())


@functools.lru_cache(maxsize=None)
def elect_states():
    rng = np.random.default_rng(4242)
    out = []
    # every length around the 64-op chunks, the first op of the second and third chunk a MATCH, a DELETE, an INSERT
    sc = [mixed_script(rng, 60 if fwd else 440, fwd, L, heads=h)
          for L in ELECT_LENS for h in (MATCH, DELETE, INSERT) for fwd in (True, False)]
    out.append(_elect_state("chunks", sc))
    # tails past post, and backward past pre, are dropped
    sc = [mixed_script(rng, ELECT_N - 20 if fwd else 19, fwd, L, heads=h)
          for L in (63, 65, 129, 200) for h in (MATCH, INSERT) for fwd in (True, False)]
    out.append(_elect_state("tails", sc))
    # single INSERTs at the ends of the range
    out.append(_elect_state("insert_dropped", [script(-ELECT_PRE, True, [INSERT], b"G"),                  # targets pre - 1
                                               script(-ELECT_PRE, True, [INSERT, MATCH, INSERT], b"GCT")]))
    out.append(_elect_state("insert_kept", [script(ELECT_N - 1 - ELECT_PRE, False, [INSERT], b"G"),       # post - 1 itself
                                            script(1 - ELECT_PRE, True, [INSERT], b"C"),                  # the box before: pre
                                            script(-ELECT_PRE, True, [MATCH, INSERT], b"AT"),
                                            script(ELECT_N - 1 - ELECT_PRE, True, [MATCH, INSERT], b"AT")]))
    # nedit == 0, and slots longer than nedit whose tail would vote if it were read
    sc = [script(0, True, [], b""), script(10, False, [], b"")]
    for fwd in (True, False):
        for ne in (0, 1, 4, 63, 64, 65):
            s = mixed_script(rng, 250, fwd, ne + 70)
            sc.append(s._replace(nedit=ne))
    out.append(_elect_state("slots", sc))
    # five hundred scripts on the same three boxes
    sc = []
    for k in range(500):
        fwd = bool(k & 1)
        ops = rng.choice(np.array([MATCH, MATCH, DELETE], np.uint8), 3)
        ops = np.insert(ops, int(rng.integers(1, 3)), INSERT)          # an INSERT between them: forward or backward it stays on 200 .. 202
        vals = np.where(ops == DELETE, 0, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 4)]).astype(np.uint8)
        sc.append(script((200 if fwd else 202) - ELECT_PRE, fwd, ops, vals.tobytes()))
    out.append(_elect_state("hammer", sc, weight=2))
    # fuzz: inside the range by the choice of position; anywhere
    sc = []
    for _ in range(200):
        L, fwd = int(rng.integers(0, 301)), bool(rng.integers(2))
        box = int(rng.integers(1, ELECT_N - L)) if fwd else int(rng.integers(L, ELECT_N))
        sc.append(mixed_script(rng, box, fwd, L, first=int(rng.integers(1, 4))))
    out.append(_elect_state("fuzz_inside", sc, weight=3))
    sc = []
    for _ in range(200):
        L, fwd = int(rng.integers(0, 301)), bool(rng.integers(2))
        sc.append(mixed_script(rng, int(rng.integers(0, ELECT_N)), fwd, L, first=int(rng.integers(1, 4))))
    out.append(_elect_state("fuzz_any", sc, weight=3))
    # counter limits: weight 65 534 plus one MATCH of the box's own base reads 65 535 and leaves its neighbours alone
    lim = State("elect/limits", b"GAGCAGATA", 65534)
    lim.scripts = [script(b, True, [MATCH], lim.base[b:b + 1]) for b in LIMIT_BOXES]
    out.append(lim)
    return tuple(out)


LIMIT_BOXES = (1, 3, 5, 7)          # bases A, C, G, T of elect/limits


def all_states():
    return evolve_states() + elect_states()


def state(name: str) -> State:
    return {s.name: s for s in all_states()}[name]


# ----------------------------------------------------------------------------- the VoteSink phase sweep
SWEEP_N, SWEEP_L = 700, 300
SWEEP_D = range(20, 150)            # 130 consecutive distances of the planted edit from the read's start
SWEEP_KINDS = ("sub", "ins", "del")


@functools.lru_cache(maxsize=None)
def sweep_case():
    """(text, reads, pairs, meta): reads are exact 300-base copies of a slice of the text with one edit at distance d from
    their start, each as a forward pair (flags 0) and a backward pair (flags 3) of reference sequence 1; a few unedited
    reads (pure runs, one of 650 bases) and three of 50 bases that the matlen_a >= 64 gate keeps from voting.
    meta[q] = (kind, d, forward)."""
    rng = np.random.default_rng(5151)
    code = np.cumsum(rng.integers(1, 4, SWEEP_N)) % 4          # random, but no base equals its neighbour: a lost base and
    text = np.frombuffer(b"ACGT", np.uint8)[code].tobytes()    # an inserted one have one place each in the cheapest alignment
    reads, pairs, meta = [], [], []

    def add(seg, s, e, kind, d):
        r = len(reads)
        reads.append(seg)
        pairs.append((1, s, len(text) - s, r, 0, len(seg), 0)); meta.append((kind, d, True))
        pairs.append((1, e - 1, e, r, len(seg) - 1, len(seg), 3)); meta.append((kind, d, False))

    for d in SWEEP_D:
        s = (3 * d) % 300
        src = text[s:s + SWEEP_L]
        other = bytes([b"ACGT"[(b"ACGT".index(src[d]) + 1 + d % 3) % 4]])
        add(src[:d] + other + src[d + 1:], s, s + SWEEP_L, "sub", d)
        new = bytes([next(x for x in b"ACGT" if x not in (src[d - 1], src[d]))])
        add(src[:d] + new + src[d:], s, s + SWEEP_L, "ins", d)         # differs from both neighbours: one place for it
        add(src[:d] + src[d + 1:], s, s + SWEEP_L, "del", d)
    for s, L in ((0, 300), (111, 300), (399, 300), (25, 650), (5, 64), (300, 50), (301, 50), (17, 50)):
        add(text[s:s + L], s, s + L, "run", L)
    return text, tuple(reads), np.array(pairs, eng.PAIR_DTYPE), tuple(meta)


_SWEEP_EXP = {}


def sweep_expectation(oracle):
    """(OracleCons with every gated script of the oracle's own aligner elected, [align result per pair])"""
    if "v" not in _SWEEP_EXP:
        text, reads, pairs, _ = sweep_case()
        cons = oracle.consensus(text, 1, MAX_LEN)
        res = []
        for pr in pairs:
            fwd = int(pr["flags"]) == 0
            seg = reads[int(pr["b_seq"])]
            a = text[int(pr["a_pos"]):] if fwd else text[:int(pr["a_pos"]) + 1]
            out = oracle.align(a, seg, R, fwd, fwd, want_ops=True)
            res.append(out)
            if out["rc"] >= 0 and out["matlen_a"] >= OVERLAP_MIN:
                cons.elect(int(pr["a_pos"]), fwd, out["ops"], eng.script_vals(out["ops"], seg, fwd))
        _SWEEP_EXP["v"] = (cons, res)
    return _SWEEP_EXP["v"]


def edit_phase(a: bytes, b: bytes, ops: np.ndarray):
    """Indices of the ops of a script that are not a MATCH of equal elements (a, b: the accessors' elements in walk order)."""
    i = j = 0
    out = []
    for k, op in enumerate(ops):
        if op == MATCH:
            if a[i] != b[j]:
                out.append(k)
            i += 1; j += 1
        elif op == INSERT:
            out.append(k); j += 1
        else:
            out.append(k); i += 1
    return out


# ----------------------------------------------------------------------------- the per-target pile-up case
PILE_LENS = (300, 12000, 500)       # the planted contig is the second of three: its boxes do not start at 0
PILE_C = 1
PILE_INS = (256 * 8 - 1, 256 * 15 + 63)               # an inserted base after thread 255 of a step; after lane 63 of wave 0
PILE_DEL = ((256 * 22 - 1, 256 * 22), (256 * 29 + 64,))   # lost: the last box of a step and the first of the next; lane 0 of wave 1
PILE_TIE = 256 * 36 - 1                               # four of seven voters carry an insertion: 2 * 4 == tot, no split
PILE_VOTERS = 6


@functools.lru_cache(maxsize=None)
def pile_case():
    """(contigs, reads, rows): exact 900-base copies of the middle contig apart from one plant, six per site (seven at the
    tie site, three of them unedited), starting 400 - 500 bases before it; sites at least 1 500 bases apart.  The contig
    reads ACGT around every site and an inserted base is a T between the C and the G, so that the cheapest alignment is
    unique and puts the edit on the planted box (polish_helpers.edge_case).  rows: the map rows of the reads, by hand."""
    rng = np.random.default_rng(6161)
    contigs = [bytearray(rand_text(rng, n)) for n in PILE_LENS]
    T = contigs[PILE_C]
    for site in PILE_INS + (PILE_TIE,):
        T[site - 1:site + 3] = b"ACGT"
    for dels in PILE_DEL:
        T[dels[0] - 1:dels[0] + 3] = b"ACGT" if len(dels) == 2 else b"ACGA"
    T = bytes(T)
    contigs = [bytes(c) for c in contigs]
    contigs[PILE_C] = T
    reads, starts = [], []
    plants = [(s, 0, PILE_VOTERS) for s in PILE_INS] + [(d[0], len(d), PILE_VOTERS) for d in PILE_DEL] + [(PILE_TIE, 0, 4), (PILE_TIE, -1, 3)]
    for site, lost, voters in plants:
        for k in range(voters):
            s = site - 400 - 17 * k - (5 if lost < 0 else 0)
            seg = bytearray(T[s:s + 900])
            at = site - s
            if lost > 0:
                del seg[at:at + lost]
            elif lost == 0:
                seg.insert(at + 1, ord("T"))
            reads.append(bytes(seg)); starts.append(s)
    rows = np.zeros(len(reads), eng.MAP_ROW_DTYPE)
    rows["read"] = np.arange(len(reads)); rows["found"] = 1; rows["strand"] = 1; rows["contig"] = PILE_C
    rows["j"] = 0; rows["pos"] = starts
    return contigs, reads, rows


# Boxes of the planted contig that yield no character although nothing was planted on them.  A read with an inserted base
# is one base longer than its slice, and the aligner ends a base further on the contig and pays a DELETE for it: the box 500
# behind the site, where the farthest-reaching read of the site ends and is the only voter (sel 1 of tot 2).
PILE_EXTRA_NONE = (2547, 4403, 9715)
PILE_EXTRA_TWO = ()

NOVOTE_LENS = (63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
NOVOTE_WEIGHTS = (1, 65535)


@functools.lru_cache(maxsize=None)
def novote_texts():
    rng = np.random.default_rng(7171)
    return tuple(rand_text(rng, n) for n in NOVOTE_LENS)


# ----------------------------------------------------------------------------- the two forms of the pile-up kernels
# (the default of PBA_PILE_LONG_SEG in csrc/pba_pileup.hip, restated: the library does not expose it)
FORM_LONG_SEG = 65536       # a pile-up runs the per-target kernels while no segment is longer than this, else the tiled ones
FORM_SWITCH_LEN = FORM_LONG_SEG + 1     # the shortest sequence that, appended to a set, switches all of it to the tiled kernels
FORM_EDGE_LEN = 20000       # polish_helpers.edge_case in a contig the per-target kernels serve: every plant and read below 16 900


@functools.lru_cache(maxsize=None)
def form_switch_text():
    return rand_text(np.random.default_rng(8181), FORM_SWITCH_LEN)
