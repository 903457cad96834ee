"""The clip rule of DESIGN §5.8 (include/pba.h: pba_clip_*) restated in plain Python -- the expectation the device is held to,
exactly (tests/test_gpu_clip.py), pinned by hand without a GPU (tests/test_clip_cpu.py) -- and the inputs both tests share:
cases computed by hand, and a read set with planted chimeras and junk tails.

The rule is a deterministic function of the overlap rows and exactly as good as they are: it sees a junction only where the
alignments really break there."""
import numpy as np

from layout_ref import ACGT, make_rows, rc  # noqa: F401  (make_rows: [(target, query, strand, cost, t_beg, t_end, q_beg, q_end)])

DROPPED, WHOLE, CUT = 0, 1, 2
TARGETS, QUERIES, KEEP_UNSEEN = 1, 2, 4
STEP = 1024                                                   # csrc/clip.h: CLIP_STEP, the positions a workgroup sweeps per step
ROW_FIELDS = ("read", "state", "beg", "end", "n_iv", "n_runs", "max_cov", "n_covered")
COUNTERS = ("n_rows", "n_iv", "n_iv_short", "n_whole", "n_cut", "n_dropped", "n_multi_run", "n_unseen", "n_bases_in", "n_bases_out")


def entries(L):
    """int32 entries of a read's difference arena: L + 1 (with margin 0 a -1 lands on entry L), rounded up to a multiple of 4"""
    return (L + 1 + 3) // 4 * 4


def n_chunks(lens, max_bases):
    """consecutive ranges of reads whose entries fit max_bases, one read at least per range"""
    k, room = 0, 0
    for L in lens:
        if k == 0 or room + entries(L) > max_bases:
            k, room = k + 1, 0
        room += entries(L)
    return k


def coverage(lens, rows, margin, flags):
    """(cov of every read, n_iv of every read, counted intervals that were too short to cover anything)"""
    cov = [np.zeros(int(L), np.int64) for L in lens]
    n_iv = [0] * len(lens)
    n_short = 0
    for r in rows:
        for role, who, b, e in ((TARGETS, "target", "t_beg", "t_end"), (QUERIES, "query", "q_beg", "q_end")):
            if not flags & role:
                continue
            x, b, e = int(r[who]), int(r[b]), int(r[e])
            n_iv[x] += 1
            if e - b <= 2 * margin:
                n_short += 1
                continue
            cov[x][b + margin:e - margin] += 1                # every p in [b + margin, e - margin)
    return cov, n_iv, n_short


def runs_of(cov, c):
    """maximal [s, e) with cov >= c throughout, in order"""
    out, s = [], None
    for p, v in enumerate(cov.tolist() if hasattr(cov, "tolist") else cov):
        if v >= c and s is None:
            s = p
        if v < c and s is not None:
            out.append((s, p))
            s = None
    if s is not None:
        out.append((s, len(cov)))
    return out


def clip_ref(lens, rows, margin, min_cov, min_len=0, flags=TARGETS | QUERIES, texts=None):
    """{"table": one ROW_FIELDS tuple per read, "stats": the COUNTERS, "cov": per read, "texts": the sliced texts if given}"""
    cov, n_iv, n_short = coverage(lens, rows, margin, flags)
    table = []
    st = dict.fromkeys(COUNTERS, 0)
    st["n_rows"], st["n_iv"], st["n_iv_short"] = len(rows), sum(n_iv), n_short
    for x, L in enumerate(int(v) for v in lens):
        runs = runs_of(cov[x], min_cov)
        state, beg, end = DROPPED, 0, 0
        if flags & KEEP_UNSEEN and n_iv[x] == 0:
            state, beg, end = WHOLE, 0, L
            st["n_unseen"] += 1
        elif runs:
            s, e = max(runs, key=lambda r: (r[1] - r[0], -r[0]))            # the longest, then the smallest start
            kb, ke = max(s - margin, 0), min(e + margin, L)
            if ke - kb >= min_len:
                state, beg, end = (WHOLE if (kb, ke) == (0, L) else CUT), kb, ke
        st[("n_dropped", "n_whole", "n_cut")[state]] += 1
        st["n_multi_run"] += len(runs) >= 2
        st["n_bases_in"] += L
        st["n_bases_out"] += end - beg
        table.append((x, state, beg, end, n_iv[x], len(runs), int(cov[x].max()) if L else 0, sum(e - s for s, e in runs)))
    out = {"table": table, "stats": st, "cov": [v.tolist() for v in cov]}
    if texts is not None:
        out["texts"] = [t[row[2]:row[3]] for t, row in zip(texts, table)]
    return out


def _st(n_rows, **kw):
    out = dict.fromkeys(COUNTERS, 0)
    out["n_rows"] = n_rows
    out.update(kw)
    return out


_TWO = [(0, 1, 1, 0, 0, 60, 0, 60), (0, 1, -1, 0, 20, 100, 0, 80)]
_SHORT = [(0, 1, 1, 0, 0, 60, 0, 60), (0, 1, -1, 0, 20, 81, 0, 61)]
HAND_CASES = [
    dict(name="two_targets_one_run", lens=[100, 80], rows=_TWO, margin=10, min_cov=2, min_len=0, flags=TARGETS,
         # read 0: [0, 60) -> [10, 50), [20, 100) -> [30, 90): cov 1 on [10, 30), 2 on [30, 50), 1 on [50, 90); one run [30, 50),
         # kept [20, 60).  Read 1: nothing counted (targets only), no run
         table=[(0, CUT, 20, 60, 2, 1, 2, 20), (1, DROPPED, 0, 0, 0, 0, 0, 0)],
         stats=_st(2, n_iv=2, n_cut=1, n_dropped=1, n_bases_in=180, n_bases_out=40)),
    dict(name="both_roles_strand_minus_as_given", lens=[100, 80], rows=_TWO, margin=10, min_cov=2, min_len=0, flags=TARGETS | QUERIES,
         # read 1: [0, 60) -> [10, 50) and, from the strand -1 row AS GIVEN, [0, 80) -> [10, 70): cov 2 on [10, 50), 1 on
         # [50, 70); run [10, 50), kept [0, 60)
         table=[(0, CUT, 20, 60, 2, 1, 2, 20), (1, CUT, 0, 60, 2, 1, 2, 40)],
         stats=_st(2, n_iv=4, n_cut=2, n_bases_in=180, n_bases_out=100)),
    dict(name="queries_only", lens=[100, 80], rows=_TWO, margin=10, min_cov=1, min_len=0, flags=QUERIES,
         # read 1 at min_cov 1: cov >= 1 on [10, 70), kept [0, 80): whole.  Read 0: nothing counted
         table=[(0, DROPPED, 0, 0, 0, 0, 0, 0), (1, WHOLE, 0, 80, 2, 1, 2, 60)],
         stats=_st(2, n_iv=2, n_whole=1, n_dropped=1, n_bases_in=180, n_bases_out=80)),
    dict(name="chimera_two_equal_runs", lens=[200, 100, 100, 100, 100], margin=10, min_cov=1, min_len=0, flags=TARGETS,
         rows=[(0, 1, 1, 0, 0, 90, 0, 90), (0, 2, 1, 0, 0, 100, 0, 100), (0, 3, 1, 0, 100, 200, 0, 100), (0, 4, -1, 0, 120, 200, 0, 80)],
         # read 0: [10, 80), [10, 90), [110, 190), [130, 190): runs [10, 90) and [110, 190), 80 each: the smaller start wins,
         # kept [0, 100) -- the extension stops at the junction 100; max cov 2, 160 covered
         table=[(0, CUT, 0, 100, 4, 2, 2, 160)] + [(k, DROPPED, 0, 0, 0, 0, 0, 0) for k in (1, 2, 3, 4)],
         stats=_st(4, n_iv=4, n_cut=1, n_dropped=4, n_multi_run=1, n_bases_in=600, n_bases_out=100)),
    dict(name="margin_zero_keep_unseen", lens=[60, 60, 10], rows=[(0, 1, 1, 0, 0, 60, 0, 60)], margin=0, min_cov=1, min_len=20,
         flags=TARGETS | QUERIES | KEEP_UNSEEN,
         # margin 0: [0, 60) covers the whole read (its -1 lands on entry L = 60).  Read 2 is unseen and shorter than
         # min_len: the flag leaves it alone
         table=[(0, WHOLE, 0, 60, 1, 1, 1, 60), (1, WHOLE, 0, 60, 1, 1, 1, 60), (2, WHOLE, 0, 10, 0, 0, 0, 0)],
         stats=_st(1, n_iv=2, n_whole=3, n_unseen=1, n_bases_in=130, n_bases_out=130)),
    dict(name="margin_zero_unseen_dropped", lens=[60, 60, 10], rows=[(0, 1, 1, 0, 0, 60, 0, 60)], margin=0, min_cov=1, min_len=20,
         flags=TARGETS | QUERIES,
         table=[(0, WHOLE, 0, 60, 1, 1, 1, 60), (1, WHOLE, 0, 60, 1, 1, 1, 60), (2, DROPPED, 0, 0, 0, 0, 0, 0)],
         stats=_st(1, n_iv=2, n_whole=2, n_dropped=1, n_bases_in=130, n_bases_out=120)),
    dict(name="interval_of_2m_and_2m_plus_1_min_len_met", lens=[100, 100], rows=_SHORT, margin=30, min_cov=1, min_len=61, flags=TARGETS,
         # [0, 60): exactly 2m, covers nothing.  [20, 81): 2m + 1, covers position 50 alone; kept [20, 81), 61 bases = min_len
         table=[(0, CUT, 20, 81, 2, 1, 1, 1), (1, DROPPED, 0, 0, 0, 0, 0, 0)],
         stats=_st(2, n_iv=2, n_iv_short=1, n_cut=1, n_dropped=1, n_bases_in=200, n_bases_out=61)),
    dict(name="min_len_missed_by_one", lens=[100, 100], rows=_SHORT, margin=30, min_cov=1, min_len=62, flags=TARGETS,
         # the run is still reported (n_runs 1, 1 covered): only the kept interval is refused
         table=[(0, DROPPED, 0, 0, 2, 1, 1, 1), (1, DROPPED, 0, 0, 0, 0, 0, 0)],
         stats=_st(2, n_iv=2, n_iv_short=1, n_dropped=2, n_bases_in=200, n_bases_out=0)),
]


def hand_texts(case, seed=0):
    """Texts for a hand case (the rows are not real overlaps of them: the rule never looks at a base before apply)."""
    rng = np.random.default_rng(2000 + seed)
    return [rng.choice(ACGT, n).tobytes() for n in case["lens"]]


# ---- the planted input: reads with chimeric joins and junk tails, where the alignments really break
PLANTED = dict(n=208, rl=1500, glen=19000, seed_g=811, seed_r=812, seed_p=813, every=20, margin=50, min_cov=2, R=0.30)


def planted_reads(P=PLANTED):
    """P["n"] reads of a synthetic genome at the generator's 15 % default error, about 16x.  Every P["every"]-th read
    (from read 3) is replaced by a chimera of two PIECES THE SET DOES NOT HOLD (further reads of the same generator: a
    piece copied from a read of the set would align to its source without an error, and R's unused budget would carry that
    row across the junction): the head of one, then the head of one that starts at least two read lengths away,
    reverse-complemented by a seeded draw; the junction is drawn from the middle third.  Every P["every"]-th (from read 13)
    carries a random tail of a fifth of the read length.  Then every second read (seeded) is reverse-complemented as a whole.
    Returns (texts, chimeras {read: junction}, junk {read: (first, last + 1) of the junk}), in the final coordinates."""
    from pacbioassembly_amd import engine as eng
    n, rl = P["n"], P["rl"]
    g = eng.synth_genome(P["seed_g"], P["glen"])
    reads, offs, starts = eng.synth_reads(P["seed_r"], g, 2 * n, rl)        # reads n .. 2n - 1: the pool of pieces
    rng = np.random.default_rng(P["seed_p"])
    src = [reads[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(2 * n)]
    texts, chim, junk = src[:n], {}, {}
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
        elif i % P["every"] == 13:
            texts[i] = src[i] + rng.choice(ACGT, rl // 5).tobytes()
            junk[i] = (rl, len(texts[i]))
    for i in range(n):
        if rng.integers(0, 2):
            L = len(texts[i])
            texts[i] = rc(texts[i])
            if i in chim:
                chim[i] = L - chim[i]
            if i in junk:
                junk[i] = (L - junk[i][1], L - junk[i][0])
    return texts, chim, junk


# Of the 11 planted chimeras, how many may keep both J - margin and J + margin: a sixth, rounded up (an alignment may swallow
# a junction that lies within R's unused budget of a read end: the rule does not see those).  Observed with the oracle's rows
# (872 of them): 1 -- chimera 3, junction 997, kept [6, 1184) -- and none WHOLE; 1 of the 11 shows two runs, 8 are cut on one
# side of the junction, 1 is dropped.  Of the 10 junk-tailed reads none is WHOLE and 281 of 3 000 junk bases are kept (one
# tail is swallowed); 75 of 187 clean reads stay whole (reported only: the overlapper's recall on 1.5 kb reads is low).
PLANTED_CHIMERAS_SPANNED_MAX = 2


def planted_report(table, chim, junk, margin):
    """What the clip table did to the planted reads.  The CONDITIONS the tests assert: no chimera is WHOLE, and at most
    PLANTED_CHIMERAS_SPANNED_MAX chimeras keep both J - margin and J + margin.  The rest is reported, not asserted."""
    rows = {t[0]: t for t in table}
    spans = lambda t, lo, hi: t[1] != DROPPED and t[2] <= lo and t[3] >= hi
    rep = dict(
        chimeras=len(chim), chimeras_whole=sum(rows[i][1] == WHOLE for i in chim),
        chimeras_spanned=sum(spans(rows[i], J - margin, J + margin) for i, J in chim.items()),
        chimeras_multi_run=sum(rows[i][5] >= 2 for i in chim),
        chimeras_cut_near=sum(rows[i][1] == CUT and (abs(rows[i][2] - J) <= margin or abs(rows[i][3] - J) <= margin) for i, J in chim.items()),
        junk=len(junk), junk_whole=sum(rows[i][1] == WHOLE for i in junk),
        junk_kept_bases=sum(max(0, min(rows[i][3], hi) - max(rows[i][2], lo)) for i, (lo, hi) in junk.items()),
        clean=len(table) - len(chim) - len(junk),
        clean_whole=sum(t[1] == WHOLE for t in table if t[0] not in chim and t[0] not in junk))
    return rep
