"""A plain model of the all-vs-all loop (overlap.h) for any max_trial, in Python and numpy: independent of the engine, the
seedmap from index_ref.np_index, the verdict of every candidate from Oracle.align.  tests/test_overlap_edges_cpu.py holds it to
Oracle.spaced_round target by target on every input of overlap_edge_inputs.py and to prefilter_inputs.overlap_candidates on that
file's cases; tests/test_gpu_overlap_edges.py holds both forms of the scan and the walk to it.

  probes        spaced_seed.cpp:426: probe jd = 2 j + backward of a read of slen bases looks at pos = j (forward) or slen - j - 16
                (backward); it exists if pos >= 0 and pos + 16 <= slen, and a zero masked key is never looked up
  candidates    of a target, in the order the reference tries them: (query, j, forward before backward, the seedmap's list
                order); the target's own probes left out; n_match counts before the gate slen - j >= overlap_min
  the walk      a (target, query) run is tried until its first success (ref_seq.h:264-265); n_pre = candidates with both clipped
                lengths >= 32 whose first failing row is one of 11 .. 32 (what the scan settles on the spot), the rest is listed
  rounds        which (step, wavefront, half) round of k_ovl_scan / k_ovl_fill a position of a target belongs to, and what the
                round's run lists look like: R runs, Tot slots, every run's first slot
"""
import numpy as np

import index_ref as ir

PPT, HALF, WAVES, WAVE = 16, 8, 4, 64          # PBA_OVL_PPT, PBA_OVL_HALF, PBA_OVL_WAVES, PBA_WAVE
PT_MAX_BITS = 26                               # PBA_PT_MAX_BITS: masks with more care bits take the hashed table
PRE_ROWS = 32


def comp(x: bytes) -> bytes:
    return x.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1]


def mask_of(pat: str) -> int:
    """dna_seq.h's key layout (index_ref.np_keys): base k of the window in byte k // 4, bits 7 - 2 (k % 4) and 6 - 2 (k % 4)"""
    m = 0
    for k, c in enumerate(pat):
        if c == "1":
            m |= 3 << (8 * (k // 4) + 6 - 2 * (k % 4))
    return m


def hashed(mask: int) -> bool:
    return bin(mask).count("1") > PT_MAX_BITS


def bucket_of(key, mask: int):
    """the probe table's bucket of a masked key: the key itself (its care bits gathered: one bucket per key) or the hash"""
    if not hashed(mask):
        return np.asarray(key, np.uint64)
    return ((np.asarray(key, np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - PT_MAX_BITS)


# ----------------------------------------------------------------------------- probes
def probes(text: bytes, mask: int, max_trial: int):
    """[(jd, pos, key)] of the probes of one read that exist and have a key, jd ascending"""
    slen = len(text)
    if slen < 16:
        return []
    keys = ir.np_keys(text) & np.uint32(mask)
    out = []
    for jd in range(2 * max_trial):
        j = jd >> 1
        pos = slen - j - 16 if jd & 1 else j
        if pos >= 0 and pos + 16 <= slen and keys[pos]:
            out.append((jd, pos, int(keys[pos])))
    return out


def probe_entries(qtexts, mask: int, max_trial: int, q_lo: int = 0, q_hi=None) -> np.ndarray:
    """the multiset of probe entries key << 32 | (q t2 + jd) of queries [q_lo, q_hi), sorted"""
    t2 = 2 * max_trial
    q_hi = len(qtexts) if q_hi is None else q_hi
    e = [(key << 32) | (q * t2 + jd) for q in range(q_lo, q_hi) for jd, _, key in probes(qtexts[q], mask, max_trial)]
    return np.sort(np.array(e, np.uint64))


class ProbeTable:
    """every probe of every query by key, and the size of every bucket of the device's table"""

    def __init__(self, qtexts, mask: int, max_trial: int):
        self.mask, self.max_trial = mask, max_trial
        self.by_key = {}
        for q, text in enumerate(qtexts):
            for jd, _, key in probes(text, mask, max_trial):
                self.by_key.setdefault(key, []).append((q, jd))
        self.n_entries = sum(len(v) for v in self.by_key.values())
        self.bucket_size = {}
        for key, v in self.by_key.items():
            b = int(bucket_of(key, mask))
            self.bucket_size[b] = self.bucket_size.get(b, 0) + len(v)


# ----------------------------------------------------------------------------- a target's seedmap and candidates
def seedmap(text: bytes, mask: int):
    """(keys ascending, positions in list order inside a key) of ref_seq::get_seedmap -- index_ref's restatement, no third one"""
    keys, pos, _ = ir.np_index(text, mask, "head_tail")
    return keys, pos


def candidates(texts, qtexts, mask: int, max_trial: int, overlap_min: int, table=None, t_lo: int = 0, t_hi=None):
    """([(target, query, jd, k, pos)] in try order -- k: the position's place in its key's list --, n_match) of the targets
    [t_lo, t_hi); the queries are the whole set, the target's own read left out by its index in the set"""
    qtexts = texts if qtexts is None else qtexts
    table = table or ProbeTable(qtexts, mask, max_trial)
    pkeys = np.array(sorted(table.by_key), np.uint32)
    out, n_match = [], 0
    for t in range(t_lo, len(texts) if t_hi is None else t_hi):
        text = texts[t]
        keys, pos = seedmap(text, mask)
        if not keys.size or not pkeys.size:
            continue
        for key in np.intersect1d(keys, pkeys):
            lo, hi = np.searchsorted(keys, key, "left"), np.searchsorted(keys, key, "right")
            for q, jd in table.by_key[int(key)]:
                if q == t:
                    continue
                n_match += hi - lo
                if len(qtexts[q]) - (jd >> 1) >= overlap_min:
                    out += [(t, q, jd, k, int(pos[lo + k])) for k in range(hi - lo)]
    out.sort()
    return out, int(n_match)


def sides(text: bytes, qtext: bytes, jd: int, p: int):
    """the two accessors' elements of a candidate (spaced_seed.cpp:274-286, ref_seq.h:282-286)"""
    j = jd >> 1
    if jd & 1:
        return text[:p + 16][::-1], qtext[:len(qtext) - j][::-1]
    return text[p:], qtext[j:]


def walk_composition(oracle, texts, qtexts, R: float, mask: int, max_trial: int, overlap_min: int, cache=None, t_lo: int = 0,
                     t_hi=None):
    """What the all-vs-all call has to answer, from the enumeration and the oracle's verdict per candidate alone:
    dict(n_match, n_gate, n_pre, n_listed, rows = [(target, query, j, dir, ref_pos, cost, matlen_a, matlen_b)], pairs,
    pairs_by = {(target, query): pairs}, cands = [dict(t, q, jd, k, p, x, ok, pre, tried)] in try order, probes = entries).
    t_lo, t_hi: the call's target range (the probe table is that of every query whatever the range)."""
    qtexts = texts if qtexts is None else qtexts
    table = ProbeTable(qtexts, mask, max_trial)
    cands, n_match = candidates(texts, qtexts, mask, max_trial, overlap_min, table, t_lo, t_hi)
    cache = {} if cache is None else cache
    rows, pairs_by, out, n_pre, done = [], {}, [], 0, None
    for t, q, jd, k, p in cands:
        x = cache.get((t, q, jd, p))
        if x is None:
            a, b = sides(texts[t], qtexts[q], jd, p)
            x = cache[(t, q, jd, p)] = oracle.align(a, b, R)
        ok = x["rc"] > 0 and x["matlen_a"] >= overlap_min
        pre = x["rc"] == -1 and 11 <= x["fail_row"] <= PRE_ROWS and x["len_a"] >= PRE_ROWS and x["len_b"] >= PRE_ROWS
        n_pre += pre
        tried = done != (t, q)
        out.append(dict(t=t, q=q, jd=jd, k=k, p=p, x=x, ok=ok, pre=pre, tried=tried))
        if not tried:
            continue
        pairs_by[(t, q)] = pairs_by.get((t, q), 0) + 1
        if ok:
            done = (t, q)
            rows.append((t, q, jd >> 1, -1 if jd & 1 else 1, p, x["cost"], x["matlen_a"], x["matlen_b"]))
    return dict(n_match=n_match, n_gate=len(cands), n_pre=int(n_pre), n_listed=len(cands) - int(n_pre), rows=rows,
                pairs=sum(pairs_by.values()), pairs_by=pairs_by, cands=out, n_probe_entries=table.n_entries)


def oracle_composition(oracle, texts, qtexts, R: float, mask: int, max_trial: int, overlap_min: int, text2bin, t_lo: int = 0,
                       t_hi=None):
    """(rows, pairs_by) of the oracle's locked spaced_seed round of every target of [t_lo, t_hi) against the file of the
    queries, the target's own read left out: rows and pairs_by as walk_composition's"""
    qtexts = texts if qtexts is None else qtexts
    file = b"".join(text2bin(t) for t in qtexts)
    offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in qtexts[:-1]]).astype(np.uint64)
    rows, pairs_by = [], {}
    for t in range(t_lo, len(texts) if t_hi is None else t_hi):
        r = oracle.spaced_round(texts[t], mask, R, file, offs, max_trial, overlap_min, buggy=False, nthreads=8)
        for q in range(len(qtexts)):
            if q == t:
                continue
            if r["n_pairs"][q]:
                pairs_by[(t, q)] = int(r["n_pairs"][q])
            if r["found"][q]:
                rows.append((t, q, int(r["j"][q]), int(r["dir"][q]), int(r["ref_pos"][q]), int(r["cost"][q]), int(r["matlen_a"][q]),
                             int(r["matlen_b"][q])))
    return rows, pairs_by


# ----------------------------------------------------------------------------- the scan's rounds
def round_of(pos: int):
    """(step, wavefront, half): thread x of step st takes chunk c = 256 st + x, positions 16 c .. 16 c + 15, and the runs of
    each half of a wavefront's 64 chunks are compacted together; inside a round the runs stand in position order"""
    c = pos >> 4
    return c // (WAVE * WAVES), c % (WAVE * WAVES) // WAVE, (pos & (PPT - 1)) // HALF


def n_chunks(tlen: int) -> int:
    """chunks a workgroup walks: positions 0 .. len - 16 of a read that visits anything"""
    return ((tlen - 16) >> 4) + 1 if tlen > 16 else 0


def rounds(text: bytes, table: ProbeTable):
    """{round: [(pos, entries of the bucket its key reaches)]} of one target, positions ascending: the runs of every round that
    has any (a run counts every entry of its bucket: the target's own and, hashed, those of another key among them).
    Shape of a round L: R = len(L), Tot = sum of the entries, run r starts at slot sum of the entries before it."""
    keys, pos = seedmap(text, table.mask)
    out = {}
    for b, p in sorted(zip(bucket_of(keys, table.mask).tolist(), pos.tolist()), key=lambda e: e[1]):
        n = table.bucket_size.get(int(b), 0)
        if n:
            out.setdefault(round_of(p), []).append((p, n))
    return out


def run_starts(L):
    return [int(s) for s in np.cumsum([0] + [n for _, n in L])]
