"""Planted inputs for the unlocked round (pba_cons_round over k_spaced_round / ss_try) and for ss_try's own gates in the
locked round (pba_spaced_round).  Nothing here needs a GPU or the oracle, and importing it computes nothing.

The unlocked round re-states a serial loop (spaced_seed.cpp:420-446: every success votes and may grow the text, the
reads after it see the grown text) as device batches, under one dependency rule: a candidate's outcome can depend on where
the text ends only while its reference accessor is shorter than len_b + max_dst (seq_aligner.h:94-102), so ss_try flags
such a read as `touching` that end, and the host defers a read once an earlier read of the batch has grown, or been put
back for, an end it touches.  Every case below places exact (or lightly edited) copies of a random genome G around the
ends of a text G[P0:P0+L] so that the rows themselves tell whether that rule was followed:

    D    the length of the reference accessor of a read's first candidate: from its first seed hit to the post end
         (forward), from the end of its last seed hit back to the pre end (backward)
    thr  s_len + 1 + int(s_len * R): at D >= thr the clip no longer looks at the accessor's own length

A case is the tuple (text, weight, reads, pool, max_trial, overlap_min, meta); meta names what the case stands on."""
from typing import NamedTuple

import numpy as np

PATTERN = "111*11*11*1*1111"
R = 0.30
GENOME_SEED, GENOME_LEN = 20261, 24000
P0, L = 9000, 3000               # the text is G[P0:P0+L]
N = 1000                         # read length of the unlocked cases
D_GROW = 750                     # the grower: N (1 - R) <= D < N
D_FOLLOW = 600
D_CHAIN = (750, 600, 450)
GATE_MIN, D_GATE_CHAIN = 400, (750, 200, 100)      # a chain of found / not found under overlap_min = 400
HEAD_JUNK = 48
SHORT_L = 1500                   # < s_len + thr: one read can touch both ends


class Case(NamedTuple):
    text: bytes
    weight: int
    reads: list
    pool: list
    max_trial: int
    overlap_min: int
    meta: dict


def thr_of(s_len: int, r: float = R) -> int:
    """the touch threshold of ss_try: len_b + max_dst of seq_aligner.h:94-102, same FP64 product and truncation"""
    return s_len + 1 + int(s_len * r)


_G = {}


def genome(seed: int = GENOME_SEED, n: int = GENOME_LEN) -> bytes:
    if (seed, n) not in _G:
        _G[(seed, n)] = np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(seed).randint(0, 4, n)].tobytes()
    return _G[(seed, n)]


def _junk(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(seed).randint(0, 4, n)].tobytes()


def text_of(length: int = L) -> bytes:
    return genome()[P0:P0 + length]


def read_at(side: str, d: int, n: int = N, length: int = L) -> bytes:
    """An exact read whose first candidate has a reference accessor of d bases on `side`: it starts d bases before the
    post end, or ends d bases behind the pre end (d >= 17: the index holds positions 0 .. length - 17)."""
    g = genome()
    if side == "post":
        return g[P0 + length - d:P0 + length - d + n]
    rd = g[P0 + d - n:P0 + d]
    if d > n - HEAD_JUNK:            # its head lies inside the text: junk there, so that no forward probe finds it first
        rd = _junk(HEAD_JUNK, d) + rd[HEAD_JUNK:]
    return rd


def interior(start: int, n: int = N) -> bytes:
    return genome()[P0 + start:P0 + start + n]


def other(ch: int) -> int:
    return b"ACGT"[(b"ACGT".index(ch) + 1) % 4]


def records(reads):
    """(file, rec_offs): the binary read file of spaced_seed (4-byte length + 2 bits per base) and its record offsets"""
    from pacbioassembly_amd import engine as eng
    file = b"".join(eng.text2bin(t) for t in reads)
    offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in reads[:-1]]).astype(np.uint64) if reads else np.zeros(0, np.uint64)
    return file, offs


def ring_read_len(nb: int, r: float = R) -> int:
    """The shortest read length whose call plans ring nb for its narrow launch: make_plan sees 1 + int(max_len * R)."""
    import align_rings as ar
    n = 64
    while ar.nb1(1 + int(n * r)) < nb:
        n += 1
    return n


def _case(name, reads, pool, line, text=None, weight=1, max_trial=4, overlap_min=64, **meta):
    meta.update(name=name, line=line, R=R)
    meta.setdefault("pool2", list(reversed(pool)))
    return Case(text_of() if text is None else text, weight, reads, pool, max_trial, overlap_min, meta)


SIDES = ("post", "pre")
_END = {"post": "ss_try: touch |= 1 (forward accessor ref_len - hit); pba_cons_round: dirty_post, deferred",
        "pre": "ss_try: touch |= 2 (backward accessor hit + 16, hit counted from ref_org); pba_cons_round: dirty_pre, org = beg - pre"}


# ------------------------------------------------------------------------------------------------ one end
def follower_cases():
    """A grower A and a follower B whose accessor is longer behind A's growth: [A, B] and [B, A] give other matlens."""
    out = []
    for side in SIDES:
        reads = [read_at(side, D_GROW), read_at(side, D_FOLLOW)]
        for pool in ([0, 1], [1, 0]):
            out.append(_case(f"follower_{side}_{pool[0]}{pool[1]}", reads, pool, _END[side], differs=("matlen_a", "matlen_b"),
                             twin=f"follower_{side}_{pool[1]}{pool[0]}"))
    return out


def ring2_cases():
    """The follower pair with a grower long enough that the call plans ring 2 (make_plan on reads->max_len)."""
    out = []
    n2 = ring_read_len(2)
    for side in SIDES:
        reads = [read_at(side, D_GROW, n2), read_at(side, D_FOLLOW)]
        for pool in ([0, 1], [1, 0]):
            out.append(_case(f"ring2_{side}_{pool[0]}{pool[1]}", reads, pool, "spaced_round_subset: make_plan ring of the narrow launch; " + _END[side],
                             differs=("matlen_a", "matlen_b"), twin=f"ring2_{side}_{pool[1]}{pool[0]}", ring=2))
    return out


def threshold_cases():
    """A follower at D = thr - 1, thr, thr + 1 behind a grower: same rows either way; below thr it must be re-walked, above
    it must not be, at thr the choice is the implementation's."""
    out = []
    for side in SIDES:
        for d in (-1, 0, 1):
            reads = [read_at(side, D_GROW), read_at(side, thr_of(N) + d)]
            out.append(_case(f"thr_{side}_{'m1' if d < 0 else 'p%d' % d}", reads, [0, 1],
                             "ss_try: my_rlen <= s_len + 1 + (int)(s_len * R); " + _END[side], thr_delta=d, one_batch=d > 0, rows_only=d == 0))
    return out


def flip_cases():
    """A follower at D = overlap_min - 1 is found only behind the growth (ref_seq.h:265 matlen_a gate); at D = overlap_min
    it is found both ways."""
    out = []
    for side in SIDES:
        for d in (63, 64):
            reads = [read_at(side, D_GROW), read_at(side, d)]
            for pool in ([0, 1], [1, 0]):
                found = d >= 64 or pool == [0, 1]
                out.append(_case(f"flip_{side}_{d}_{pool[0]}{pool[1]}", reads, pool, "ss_try: o.matlen_a < overlap_min -> continue; " + _END[side],
                                 follower_found=found, max_trial=4))
    return out


def chain_cases():
    """A, B, C each with a longer accessor behind the one before: three batches.  `chain` changes matlens, `gatechain`
    (overlap_min 400) changes found / not found."""
    out = []
    for side in SIDES:
        for name, ds, omin in (("chain", D_CHAIN, 64), ("gatechain", D_GATE_CHAIN, GATE_MIN)):
            reads = [read_at(side, d) for d in ds]
            for tag, pool in (("fwd", [0, 1, 2]), ("rev", [2, 1, 0])):
                out.append(_case(f"{name}_{side}_{tag}", reads, pool, "pba_cons_round: pending.swap(deferred), one growth per end and batch; " + _END[side],
                                 overlap_min=omin, depth=3 if tag == "fwd" else (2 if name == "chain" else 1), ds=ds))
    return out


# ------------------------------------------------------------------------------------------------ both ends
def both_ends_reads():
    return [read_at("post", D_GROW), read_at("pre", D_GROW), read_at("post", D_FOLLOW), read_at("pre", D_FOLLOW)]


def both_ends_cases():
    out = []
    reads = both_ends_reads()
    for tag, pool in (("fwd", [0, 1, 2, 3]), ("rev", [3, 2, 1, 0])):
        out.append(_case(f"both_{tag}", reads, pool, "pba_cons_round: dirty_post / dirty_pre kept apart, both growths applied after the votes"))
    # a forward read found in a batch after a prepend: [A', B', F] -- B' is put back for the pre end, which dirties both
    # ends, so the forward follower F is re-walked at ref_org > 0 and its ref_pos must stay relative to beg
    reads = [read_at("pre", D_GROW), read_at("pre", D_FOLLOW), read_at("post", D_FOLLOW), interior(1200)]
    out.append(_case("fwd_after_prepend", reads, [0, 1, 2, 3], "ss_try: myhit = ix_pos + ref_org, st.ref_pos = hit - ref_org; row_accessors(org)",
                     depth=2))
    # a follower that touches only the end that did not grow is taken in the first batch
    for side, oth in (("post", "pre"), ("pre", "post")):
        reads = [read_at(side, D_GROW), read_at(oth, 1100)]
        out.append(_case(f"other_end_{side}", reads, [0, 1], "pba_cons_round: (touch & 1) && dirty_post || (touch & 2) && dirty_pre", one_batch=True))
    # a short text: the forward candidate of T touches the post end and fails, its backward one touches the pre end
    g = genome()
    t = read_at("post", 600, 40, SHORT_L) + g[200:460] + read_at("pre", 800, 700, SHORT_L)
    for side in SIDES:
        reads = [read_at(side, D_GROW, N, SHORT_L), t]
        out.append(_case(f"short_text_{side}", reads, [0, 1], "ss_try: touch bits of every visited candidate, failed ones included",
                         text=text_of(SHORT_L)))
    return out


def interior_cases():
    """Reads with D > thr on both sides are never deferred."""
    ins = [interior(400), interior(900), interior(1500)]
    grow = [read_at("post", D_GROW), read_at("pre", D_GROW)]
    foll = [read_at("post", D_FOLLOW), read_at("pre", D_FOLLOW)]
    out = [_case("interior_growers", [ins[0], grow[0], ins[1], grow[1], ins[2]], [0, 1, 2, 3, 4],
                 "ss_try: touch stays 0 above thr; pba_cons_round: one batch", one_batch=True)]
    reads = [ins[0], grow[0], ins[1], foll[0], ins[2], grow[1], interior(600), foll[1]]
    out.append(_case("interior_interleaved", reads, list(range(8)), "pba_cons_round: interior rows accepted behind a deferral",
                     interior=[0, 2, 4, 6]))
    return out


# ------------------------------------------------------------------------------------------------ votes at the seam
def _edit(side, kind):
    """The grower with one planted edit at the seam: the last reference base (post) or the first (pre)."""
    rd = bytearray(read_at(side, D_GROW))
    k = D_GROW - 1 if side == "post" else N - D_GROW          # the read's copy of that base
    if kind == "sub":
        rd[k] = other(rd[k])
    elif kind == "ins":                                     # a base directly behind (post) / in front of (pre) it
        at = k + 1 if side == "post" else k
        rd[at:at] = bytes([other(rd[k])])
    else:
        del rd[k]
    return bytes(rd)


def vote_cases():
    """Growers with an edit at the seam, a clean follower that is deferred and votes over the appended boxes."""
    out = []
    for side in SIDES:
        for kind in ("sub", "ins", "del"):
            for weight in (1, 3):
                reads = [_edit(side, kind), read_at(side, D_FOLLOW), read_at(side, 900)]
                out.append(_case(f"vote_{side}_{kind}_w{weight}", reads, [0, 1, 2],
                                 "pba_cons_round: votes against the batch's text (vote_into(c->pre)), growths after them", weight=weight))
    return out


# ------------------------------------------------------------------------------------------------ pool forms
def pool_cases():
    reads = [interior(100), read_at("post", D_FOLLOW), interior(700), interior(1300), read_at("pre", D_GROW), interior(1900),
             read_at("post", D_GROW), read_at("pre", D_FOLLOW)]
    out = [_case("subset_pool", reads, [6, 1, 4, 2], "spaced_round_subset: rows[subset[k]] only", outside=[0, 3, 5, 7], pool2=[7, 5, 0])]
    for n in (0, 10, 15):
        out.append(_case(f"tiny_text_{n}", both_ends_reads(), [2, 0, 3], "pba_cons_round: an index without entries", text=text_of(n), one_batch=True))
    return out


def toolong_cases():
    """A growth past the buffer (post + add > 3 max_len, pre - add < 0): PBA_E_TOOLONG on either end."""
    out = []
    for side in SIDES:
        out.append(_case(f"toolong_{side}", [read_at(side, 150, N, 200)], [0], "pba_cons_append / pba_cons_prepend: PBA_E_TOOLONG",
                         text=text_of(200), max_len=200))
    return out


def unlocked_cases():
    return (follower_cases() + ring2_cases() + threshold_cases() + flip_cases() + chain_cases() + both_ends_cases() + interior_cases() +
            vote_cases() + pool_cases())


# ------------------------------------------------------------------------------------------------ locked-round gates
LOCK_SEED, LOCK_LEN = 20262, 12000
N_PLANTS, PLANT_AT, PLANT_STEP = 130, 100, 40
PLANT_READS = (0, 63, 64, 65, 128, 129)
LOCK_N = 600
SHORT_LENS = (15, 16, 17, 63, 64, 65, 79, 80)


def locked_ref() -> bytes:
    """A random reference with one 16-mer planted 130 times 40 apart (long hit lists), and, at its very start, a copy
    of the 63 bases that end a later 16-mer (a first candidate with matlen_a = overlap_min - 1)."""
    g = bytearray(genome(LOCK_SEED, LOCK_LEN))
    k = bytes(g[50:66])
    for i in range(N_PLANTS):
        g[PLANT_AT + PLANT_STEP * i:PLANT_AT + PLANT_STEP * i + 16] = k
    g[0:63] = g[SHORT_HIT_END - 63:SHORT_HIT_END]
    return bytes(g)


SHORT_HIT_END = 8016             # the later 16-mer sits at 8000


SHORT_AT = 7001                  # where the short reads are copied from (see skipped_probes)
SPACER, SPACER_AT, JUNK_SEED = 200, 50399, 40


def locked_reads(ring: int = 1):
    """(reads, names, n_checked): reads [0, n_checked) are compared in both seed placements; the fillers behind them keep
    the reference's seed_at (a byte offset where pos % 4 == 0, dna_seq.h:64) inside the set for every compared read.

    A probe with pos < 0 or pos + 16 > slen is skipped by ss_try without a trial.  The reference has no such gate (it
    keeps no read below 500 bases) and reads the neighbouring records' bytes there, so each short read lies between
    spacers from a foreign genome, and SHORT_AT is chosen so that none of those windows is a key of the index
    (skipped_probes lists them; the CPU suite looks each one up): the gate is then the only thing the rows can show."""
    ref = locked_ref()
    foreign = genome(LOCK_SEED + 1, 60000)
    reads, names = [], []
    for i in PLANT_READS:                                            # long hit lists: n_pairs = i + 1
        p = PLANT_AT + PLANT_STEP * i
        reads.append(ref[p:p + LOCK_N]); names.append(f"plant_{i}")
    reads.append(b"A" * 20 + ref[9000:9000 + LOCK_N - 20]); names.append("poly_a")      # key 0 at the forward probe j = 0
    # the backward probe j = 0 meets position 47 first (accessor 63 bases, an exact match: matlen_a = 63), then 8000
    reads.append(_junk(40, 3) + ref[SHORT_HIT_END - LOCK_N + 40:SHORT_HIT_END]); names.append("short_first_hit")
    reads.append(ref[10000:10000 + LOCK_N]); names.append("both_dirs")                    # found forward at j = 0 ...
    reads.append(_junk(16, 5) + ref[10016:10000 + LOCK_N]); names.append("both_dirs_bwd")  # ... and backward at j = 0 too
    if ring == 2:
        n2 = ring_read_len(2)
        reads.append(ref[1000:1000 + n2]); names.append("ring2")
    k = 0
    for n in SHORT_LENS:                                             # pos + 16 > slen, s_len < overlap_min
        for nm, rd in ((f"short_{n}", ref[SHORT_AT:SHORT_AT + n]),
                       (f"short_tail_{n}", _junk(min(16, n), JUNK_SEED + n) + ref[SHORT_AT + 16:SHORT_AT + n])):
            reads.append(foreign[SPACER_AT + SPACER * k:SPACER_AT + SPACER * (k + 1)]); names.append(f"spacer_{k}"); k += 1
            reads.append(rd); names.append(nm)
    n_checked = len(reads)
    for i in range(max(len(r) for r in reads) // 250 + 2):        # a byte offset up to the longest read's length stays inside
        reads.append(foreign[1000 * i:1000 * i + 1000]); names.append(f"filler_{i}")
    return reads, names, n_checked


def skipped_probes(slen: int, max_trial: int = 32):
    """[(pos, dir)] of the probes of spaced_seed.cpp:424-426 that ss_try's first gate skips for a read of slen bases"""
    out = []
    for j in range(max_trial):
        for pos, d in ((j, 1), (slen - j - 16, -1)):
            if pos < 0 or pos + 16 > slen:
                out.append((pos, d))
    return out


LOCK_MAX_TRIAL, LOCK_OVERLAP_MIN = 32, 64
PLANT_PAIRS = {f"plant_{i}": i + 1 for i in PLANT_READS}
