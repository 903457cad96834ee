"""Hand-made read sets for the bookkeeping of the all-vs-all scan (overlap.h): the run lists of a round (PBA_OVL_COMPACT and
the slot-to-run `locate` of k_ovl_scan), the head / tail visiting order inside the overlapper (HeadTail, TargetWalk), the
candidates behind a success (k_ovl_after), the probe entries (k_probe_emit) and a census that misses.  No GPU in here:
test_overlap_edges_cpu.py proves from overlap_ref.py and the oracle what every set is, test_gpu_overlap_edges.py runs both forms
of the kernels on them.

How a set is made.  A target is random text with 16-base windows planted in it.  A BUCKET of N entries is N queries that share
one window W as their head (forward probe j = 0) or as their tail (backward probe j = 0); W planted at a target position is a
run of N there.  A SINGLE is a query whose window is the target's own at one position: a run of one, so that the slot of a
candidate inside its round is its position's rank (the order inside a bucket is the table's fill order and nobody's to choose).
A member survives the scan's 32 rows where its body copies the target behind (forward) or before (backward) the plant; the
others carry random bodies and the oracle says what becomes of them.  A seed is taken only if enumeration finds exact 16-base
copies of probe windows and nothing else (is_clean: a chance hit agrees at the mask's care positions only)."""
import functools

import numpy as np

import align_rings as ar
import index_ref as ir
import overlap_ref as orf
import prefilter_inputs as pi
from conftest import MASK_PAT

RUN_R, RUN_MIN = 0.30, 20
HT_R, HT_MIN = 0.15, 20
HT_LENS = (20015, 20016, 20017, 20036, 40015, 40016, 40017, 50000)
AFTER_R = 0.15
AFTER_TRIALS = (1, 2, 33, 63)
AFTER_MINS = (10, 30)
LAST_MODS = (0, 1, 15)
SHORT_LENS = (0, 15, 16, 17, 31, 32)
CENSUS_READS, CENSUS_TARGET, CENSUS_PLANTS = 1040, 1, 72


class Set:
    """reads in order, the index of every named one, and which of them are queries only (flipped_view)"""

    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        self.texts, self.idx, self.queries = [], {}, []

    def rand(self, n):
        return ar.rand_seq(self.rng, n)

    def window(self):
        while True:
            w = self.rand(16)
            if w[0] != 65 and w[15] != 65:
                return w

    def add(self, text, name=None, query=False):
        self.texts.append(bytes(text))
        if name is not None:
            self.idx[name] = len(self.texts) - 1
        if query:
            self.queries.append(len(self.texts) - 1)
        return len(self.texts) - 1

    def target(self, name, length, plants=()):
        buf = bytearray(self.rand(length))
        buf[:16] = b"A" * 16                        # a zero key: the target's own head probe does not exist, position 0 holds no run
        for pos, w in plants:
            assert 0 <= pos and pos + len(w) <= length
            buf[pos:pos + len(w)] = w
        self.add(buf, name)
        return bytes(buf)

    def other(self, base: bytes) -> bytes:
        return b"ACGT"[(b"ACGT".index(base) + 1 + self.rng.randint(3)) % 4:][:1]

    def fwd(self, w, T=None, p=None, n=64, name=None):
        """a query of n bases with head window w; T, p: its body copies the target behind the plant at p"""
        body = T[p + 16:p + n - 16] if T is not None else b""
        body += self.rand(n - 32 - len(body))
        return self.add(w + body + self.rand(16), name, query=True)

    def bwd(self, w, T=None, p=None, n=64, name=None):
        body = T[max(0, p - (n - 32)):p] if T is not None else b""
        body = self.rand(n - 32 - len(body)) + body
        return self.add(self.rand(16) + body + w, name, query=True)

    def bucket(self, N, w, T=None, p=None, survivors=(), fwd=True):
        return [(self.fwd if fwd else self.bwd)(w, T if i in survivors else None, p) for i in range(N)]


def is_clean(texts, qtexts, mask, max_trial, overlap_min):
    """every seed match is an exact copy of the probe's 16 bases"""
    qtexts = texts if qtexts is None else qtexts
    cands, _ = orf.candidates(texts, qtexts, mask, max_trial, 0)
    for t, q, jd, _, p in cands:
        j, slen = jd >> 1, len(qtexts[q])
        pos = slen - j - 16 if jd & 1 else j
        if texts[t][p:p + 16] != qtexts[q][pos:pos + 16]:
            return False
    return True


def first_clean(make, mask, max_trial, overlap_min, tries=24):
    for attempt in range(tries):
        S = make(attempt)
        if is_clean(S.texts, None, mask, max_trial, overlap_min) and is_clean(*flipped_view(S), mask, max_trial, overlap_min):
            return S                                # (clean forward and in the reverse-complement pass's view)
    raise RuntimeError("no seed without a chance hit")


def round_positions(step, wave, half, lanes, ks=range(orf.HALF)):
    """positions of one round in slot order: lanes of the wavefront, ks of the half"""
    return [16 * (256 * step + 64 * wave + lane) + orf.HALF * half + k for lane in lanes for k in ks]


def find_collision(rng, mask):
    """two windows whose masked keys differ and fall into one bucket of the hashed table"""
    text = ar.rand_seq(rng, 60015)
    ws = [text[i:i + 16] for i in range(60000)]
    keys = (ir.np_keys(text)[:60000] & np.uint32(mask)).astype(np.uint64)
    b = ((keys * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - orf.PT_MAX_BITS)
    order = np.argsort(b, kind="stable")
    for i, k in zip(order, order[1:]):
        if b[i] == b[k] and keys[i] != keys[k] and keys[i] and keys[k] and 65 not in (ws[i][0], ws[i][15], ws[k][0], ws[k][15]):
            return ws[i], ws[k]
    raise RuntimeError("no collision among 60 000 windows")


# ----------------------------------------------------------------------------- the run lists
# Chance hits grow with probes x positions / 2^24 under MASK_PAT, so the run-list inputs are several small sets, not one.
RUN_SETS = ("b_small", "b128", "b200", "b520", "shapes", "groups", "full", "misc")
BUCKETS = {"b_small": (1, 63, 64, 65), "b128": (128, 129), "b200": (200,), "b520": (520,)}
SHAPES = {"r64_5": [(32, 64), (48, 5)], "r60_4_5": [(32, 60), (48, 4), (64, 5)], "tot_small": [(32, 3), (34, 1), (48, 2)],
          "ones64_5": [(p, 1) for p in round_positions(0, 0, 0, range(2, 10))] + [(160, 5)],
          "ones65": [(p, 1) for p in round_positions(0, 0, 0, range(2, 10))] + [(160, 1)]}
GROUP_POS = round_positions(0, 0, 0, range(4, 28))
GROUP_LANES = (0, 31, 32, 63)
FULL_POS = round_positions(0, 0, 1, range(64))
LAYOUT_POS = [16 * 67 + 1, 16 * 137 + 12, 16 * 252 + 3, 16 * 257 + 5]
LAYOUT_LANE = [16 * 5 + 2, 16 * 5 + 10]          # singles: both halves of one lane
LAYOUT_LEN, LAYOUT_LAST = 16 * 261 + 9, 16 * 260 + 5


@functools.lru_cache(maxsize=None)
def runlist_set(name: str, pat: str = MASK_PAT):
    return first_clean(lambda a: _runlist_set(name, pat, a), orf.mask_of(pat), 1, RUN_MIN)


def _runlist_set(name, pat, attempt):
    """One target per situation (test_overlap_edges_cpu.py says what each must show), one trial, queries of 64 bases (40 in
    "full")."""
    S = Set(9900 + 100 * RUN_SETS.index(name) + 1000 * (pat != MASK_PAT) + 10000 * attempt)
    S.facts = {}
    if name in BUCKETS:                         # a bucket of N at position 40: one run of N alone in its round
        for N in BUCKETS[name]:
            w = S.window()
            T = S.target(f"b{N}", 200, [(40, w)])
            # forward, every member holds W at its own position 0: a run of N there too, its own entry inside (N * N candidates).
            # Above 512 backward: W is a member's last window, which a short target does not visit.
            for i in range(N):
                (S.fwd if N < 512 else S.bwd)(w, T if i in (0, N // 2, N - 1) else None, 40)
    if name == "shapes":                        # (position, bucket size) of one round in slot order; size 1 = a single
        for tname, runs in SHAPES.items():
            ws = {p: S.window() for p, n in runs if n > 1}
            T = S.target(tname, 260, list(ws.items()))
            for i, (p, n) in enumerate(runs):
                if n > 1:
                    S.bucket(n, ws[p], T, p, {0, n - 1})
                else:
                    S.fwd(T[p:p + 16], T if i % 3 == 0 else None, p)
    if name == "groups":                        # three slot groups of runs of one, forward and backward alternating
        T = S.target("groups", 16 * 28 + 80)
        for s, p in enumerate(GROUP_POS):
            q = (S.fwd if s % 2 == 0 else S.bwd)(T[p:p + 16], T if s % 64 in GROUP_LANES else None, p)
            S.facts[q] = (s, p)
    if name == "full":                          # all 512 positions of half 1 of wavefront 0; the queries' tails fall into half 0
        T = S.target("full", 16 * 64 + 48)
        for p in FULL_POS:
            S.add(T[p:p + 40], query=True)
    if name == "misc":
        _misc_targets(S)
    return S


def _misc_targets(S):
    # layout: both halves of one lane, every wavefront, step 1, the last live chunk (261 chunks: lanes 5 .. 63 of step 1 dead)
    w = S.window()
    T = S.target("layout", LAYOUT_LEN, [(p, w) for p in LAYOUT_POS])
    S.bucket(3, w, T, LAYOUT_POS[0], {0})
    for p in LAYOUT_LANE:
        S.fwd(T[p:p + 16], T, p)
    S.fwd(T[LAYOUT_LAST:LAYOUT_LAST + 16])
    S.bwd(T[LAYOUT_LAST:LAYOUT_LAST + 16], T, LAYOUT_LAST)
    # the last window: W at len - 16 is not visited, at len - 17 it is; and a W cut by the end of a read
    for m in LAST_MODS:
        w, L = S.window(), 160 + m
        S.target(f"last16_{m}", L, [(L - 16, w)])
        T = S.target(f"last17_{m}", L, [(L - 17, w)])
        S.target(f"cut_{m}", L, [(L - 9, w[:9])])
        S.add(w[9:] + S.rand(57), f"cutnext_{m}")
        S.bucket(2, w, T, L - 17, {0})
    # short reads behind one head window, as queries of a target and as targets of a query
    w = S.window()
    T = S.target("short_t", 200, [(40, w)])
    for L in SHORT_LENS:
        S.add((w + T[56:72])[:L] if L >= 16 else S.rand(L), f"short{L}", query=True)
    S.fwd(w, T, 40, name="short_q")
    # the target's own probes: its head window is a bucket's, and planted once more; and a read identical to it
    w = S.window()
    T = S.target("own_t", 200, [(0, w), (80, w)])
    S.bucket(3, w, T, 80, {1})
    S.add(T, "own_twin")
    # two keys in one bucket of the hashed table
    w1, w2 = find_collision(S.rng, orf.mask_of(pi.HEAVY_PAT))
    T = S.target("col_t", 200, [(40, w1), (104, w2)])
    S.bucket(3, w1, T, 40, {0})
    S.bucket(2, w2, T, 104, {1})
    S.facts["collide"] = (w1, w2)


# ----------------------------------------------------------------------------- head and tail
def head_tail(L: int):
    """(nhead, tail_lo, tail_top) of ref_seq::get_seedmap: positions 0 .. nhead - 1 ascending, then tail_top .. tail_lo descending"""
    nh, nt = max(0, min(L - 16, 20000)), max(0, min(L - 20016, 20000))
    return nh, L - 16 - nt + 1, L - 16


def ht_positions(L: int):
    nh, lo, top = head_tail(L)
    return sorted({p for p in (nh - 1, 19999, 20000, lo - 1, lo, top) if 0 <= p <= L - 16})


def ht_order(L: int):
    """two head and two tail positions of the two windows that show the try order (targets with room for them in the tail)"""
    lo = head_tail(L)[1]
    return dict(a=[1000, 3000, lo + 500, lo + 2500], b=[1200, 3200, lo + 700, lo + 2700]) if L >= 40015 else None


@functools.lru_cache(maxsize=None)
def headtail_set(L: int):
    return first_clean(lambda a: _headtail_set(L, a), orf.mask_of(MASK_PAT), 1, HT_MIN)


def _headtail_set(L, attempt):
    """One target of L bases; at each of ht_positions an exact copy read forward (from the plant on) and one read backward (up
    to the plant's last base, behind one base that is not the target's); the first 15 bases of a window at tail_top + 1, completed by the next read; from 40 015 bases on
    one window at two head and two tail positions with the same 48 bases behind all four (the first in try order wins: the
    lower head position), and one whose copies succeed in the tail only (the higher tail position wins)."""
    S = Set(9950 + L + 100000 * attempt)
    order = ht_order(L)
    wcut = S.window()
    plants = [(L - 15, wcut[:15])]
    if order:
        wa, wb, sa, sb = S.window(), S.window(), S.rand(48), S.rand(48)
        plants += [(p, wa + sa) for p in order["a"]] + [(p, wb) for p in order["b"][:2]] + [(p, wb + sb) for p in order["b"][2:]]
    T = S.target("T", L, plants)
    S.add(wcut[15:] + S.rand(63), "next")
    S.facts = dict(q={})
    for p in ht_positions(L):
        # (the backward copy behind one other base: its head window finds nothing, so the backward probe is the one reported)
        S.facts["q"][p] = (S.add(T[p:p + 64], query=True), S.add(S.other(T[p - 49:p - 48]) + T[p - 48:p + 16], query=True))
    if order:
        S.facts["qa"] = S.add(wa + sa, query=True)
        S.facts["qb"] = S.add(wb + sb, query=True)
    return S


# ----------------------------------------------------------------------------- behind a success
AFTER_SETS = ("main", "own")


@functools.lru_cache(maxsize=None)
def after_set(name: str):
    return first_clean(lambda a: _after_set(name, a), orf.mask_of(MASK_PAT), max(AFTER_TRIALS), min(AFTER_MINS), tries=40)


def _after_set(name, attempt):
    """Queries of 80 bases (40: "short") cut from their targets so that every probe is an exact copy and the first candidate
    of most runs succeeds; what lies behind it is what k_ovl_after has to count (after_situations names it)."""
    S = Set(9970 + (name == "own") + 10000 * attempt)
    if name == "own":
        wk, wl = S.window(), S.window()
        body_k, body_l = S.rand(64), S.rand(64)
        S.target("T3", 20100, [(500, wk + body_k), (1500, wk), (20030, wk), (600, wl), (1600, wl + body_l), (20050, wl)])
        S.add(wk + body_k, "own_first", query=True)                 # success at 500; its key again at 1 500 (head) and 20 030 (tail)
        S.add(wl + body_l, "own_second", query=True)                # fails at 600, success at 1 600; behind it the tail's 20 050 only
        return S
    unit = S.rand(21)
    while len(set(unit)) < 4:
        unit = S.rand(21)
    T1 = bytearray(S.rand(620))
    T1[200:216] = b"A" * 16
    T1[199:200], T1[216:217] = b"C", b"G"
    T1[300:426] = unit * 6
    T1 = bytes(T1)
    S.add(T1, "T1")
    S.add(T1[50:130], "plain", query=True)                      # forward success at j = 0, its backward probe and every later one behind
    S.add(T1[195:275], "zero", query=True)                      # the forward probe at j = 5 is sixteen A
    S.add(T1[300:380], "periodic", query=True)                  # period 21: later probes with the success's key, and with one another's
    x = b"ACGT"[(b"ACGT".index(T1[449:450]) + 1) % 4:][:1]
    S.add(x + T1[450:529], "back", query=True)                  # no forward hit at j = 0; backward success, forward j = 1 behind
    S.add(T1[540:580], "short", query=True)                     # 40 bases: probes behind j = 24 do not exist
    T2 = bytearray(S.rand(400))
    T2[20:36] = T2[100:116]                                     # a decoy before the copy: the success is the run's second candidate
    T2[300:316] = T2[240:256] = T2[200:216]                     # two decoys before the copy at 300, whose tail is not the target's
    T2 = bytes(T2)
    S.add(T2, "T2")
    S.add(T2[100:180], "middle", query=True)
    S.add(T2[300:372] + S.rand(8), "last", query=True)
    return S


def after_situations(W, texts, mask, max_trial, overlap_min):
    """what lies behind every success of a model run W: {(target, query): set of names}"""
    out = {}
    keyset = {}
    for c in W["cands"]:
        keyset.setdefault((c["t"], c["q"]), []).append(c)
    for t, q, j, d, p, *_ in W["rows"]:
        run = keyset[(t, q)]
        jd0 = 2 * j + (d < 0)
        at = [i for i, c in enumerate(run) if c["jd"] == jd0 and c["p"] == p][0]
        names = {"first" if at == 0 else "last" if at == len(run) - 1 else "middle"}
        qt, slen = texts[q], len(texts[q])
        keys = ir.np_keys(qt) & np.uint32(mask)
        pos0 = slen - j - 16 if d < 0 else j
        later = {}
        for jd in range(jd0 + 1, 2 * max_trial):
            jj = jd >> 1
            pos = slen - jj - 16 if jd & 1 else jj
            if pos < 0 or pos + 16 > slen:
                if slen - jj >= overlap_min:
                    names.add("nonexistent_past_gate")
                continue
            if not keys[pos]:
                names.add("zero_key")
                continue
            if slen - jj == overlap_min - 1:
                names.add("gate_minus_1")
            if slen - jj < overlap_min:
                continue
            later[int(keys[pos])] = later.get(int(keys[pos]), 0) + 1
            if jd == jd0 + 1 and d > 0:
                names.add("fwd_then_bwd_of_j")
            if jd == jd0 + 1 and d < 0:
                names.add("bwd_then_fwd_of_j_plus_1")
        if int(keys[pos0]) in later:
            names.add("own_key_repeats")
        if 3 in later.values():
            names.add("multiplicity_3")
        own = [c for c in run[at + 1:] if c["jd"] == jd0]
        if any(c["p"] < 20000 for c in own) and any(c["p"] > 20000 for c in own):
            names.add("own_key_head_and_tail_behind")
        if any(c["jd"] == jd0 for c in run[:at]):
            names.add("own_key_before")
        out[(t, q)] = names
    return out


AFTER_NAMES = {"first", "middle", "last", "nonexistent_past_gate", "zero_key", "gate_minus_1", "fwd_then_bwd_of_j", "bwd_then_fwd_of_j_plus_1",
               "own_key_repeats", "multiplicity_3", "own_key_head_and_tail_behind", "own_key_before"}


# ----------------------------------------------------------------------------- a census that misses
@functools.lru_cache(maxsize=None)
def census_set():
    return first_clean(_census_set, orf.mask_of(MASK_PAT), 1, RUN_MIN, tries=60)


def _census_set(attempt):
    """1 040 reads: read 1 holds CENSUS_PLANTS places 40 bases apart, reads 2 .. are their exact copies (each survives forward,
    and backward through its tail), the rest are fillers of 17 bases.  A range of 1 040 targets is sized from every 16th: those
    have no candidate at all, and read 1 needs more room than they ask for."""
    S = Set(9990 + 10000 * attempt)
    S.add(S.rand(17))
    T = S.target("dense", 40 * (CENSUS_PLANTS + 2))
    for i in range(CENSUS_PLANTS):
        S.add(T[40 * (i + 1):40 * (i + 2)], query=True)
    while len(S.texts) < CENSUS_READS:
        S.add(S.rand(17))
    return S


# ----------------------------------------------------------------------------- short masks: the probe table's small scan
# Masks of six and of seven care bases: 4 096 and 16 384 buckets, either side of the one-workgroup scan of the probe table's
# bucket counts (PBA_SCAN_SMALL_MAX).  Such masks hit by chance all over -- no input is clean under them, and none has to be.
SHORT_PATS = ("1**1*1**1**1***1", "1**1*1**1*11***1")
SHORT_R, SHORT_MIN, SHORT_TRIALS = 0.15, 40, 3


@functools.lru_cache(maxsize=None)
def short_mask_set():
    """twelve reads of 300 bases, 100 bases apart on a 1 400-base text (neighbours overlap by 200 and by 100), every third with
    a few substitutions"""
    S = Set(4242)
    G = S.rand(1400)
    for i in range(12):
        r = bytearray(G[100 * i:100 * i + 300])
        if i % 3 == 1:
            for at in S.rng.randint(20, 280, 4):
                r[at:at + 1] = S.other(bytes(r[at:at + 1]))
        S.add(r, query=True)
    return S


def flipped_view(S):
    """(texts, qtexts) of the reverse-complement pass over the set whose query reads were flipped: the pass's queries are the
    designed bases again (prefilter_inputs.straddle_views)"""
    qs = set(S.queries)
    mixed = [orf.comp(x) if i in qs else x for i, x in enumerate(S.texts)]
    return mixed, [orf.comp(x) for x in mixed]


# ----------------------------------------------------------------------------- what the kernels are held to
CASES = ([("run", name, pat) for pat in (MASK_PAT, pi.HEAVY_PAT) for name in RUN_SETS] + [("ht", L) for L in HT_LENS]
         + [("after", name, mt, om) for name in AFTER_SETS for mt in AFTER_TRIALS for om in AFTER_MINS])
VIEW_CASES = [("run", "b_small", MASK_PAT), ("run", "shapes", MASK_PAT), ("run", "groups", MASK_PAT), ("run", "full", MASK_PAT),
              ("run", "misc", pi.HEAVY_PAT), ("ht", 40017)]
SHORT_CASES = [("short", pat) for pat in SHORT_PATS]


def case_id(case):
    return "-".join("heavy" if c == pi.HEAVY_PAT else "plain" if c == MASK_PAT else str(c) for c in case)


def case_params(case):
    """(set, R, mask pattern, max_trial, overlap_min)"""
    if case[0] == "run":
        return runlist_set(case[1], case[2]), RUN_R, case[2], 1, RUN_MIN
    if case[0] == "ht":
        return headtail_set(case[1]), HT_R, MASK_PAT, 1, HT_MIN
    if case[0] == "after":
        return after_set(case[1]), AFTER_R, MASK_PAT, case[2], case[3]
    if case[0] == "short":
        return short_mask_set(), SHORT_R, case[1], SHORT_TRIALS, SHORT_MIN
    return census_set(), RUN_R, MASK_PAT, 1, RUN_MIN


_MODEL, _ALIGNS = {}, {}


def expected(oracle, case, view="forward"):
    """the model's answer for a case, once per session: overlap_ref.walk_composition's dict with texts, qtexts, mask and the
    call's parameters beside it.  view "rc": the reverse-complement pass over the set with its query reads flipped."""
    key = (case, view)
    if key not in _MODEL:
        S, R, pat, mt, om = case_params(case)
        texts, qtexts = (S.texts, S.texts) if view == "forward" else flipped_view(S)
        mask = orf.mask_of(pat)
        W = orf.walk_composition(oracle, texts, qtexts, R, mask, mt, om, cache=_ALIGNS.setdefault((case[:2], view, pat), {}))
        W.update(S=S, texts=texts, qtexts=qtexts, mask=mask, R=R, max_trial=mt, overlap_min=om)
        _MODEL[key] = W
    return _MODEL[key]
