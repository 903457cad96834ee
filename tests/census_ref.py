"""The seed-key census (pba_census_*) as plain numpy, independent of the engine: which positions are visited and
what a window's key is come from index_ref (np_index, np_keys, visit_order) -- there is no second restatement of keys here --,
the probes, the candidates and the first-success loop from overlap_ref, the verdict of a candidate from Oracle.align.
tests/test_census_cpu.py pins it by hand and proves the conditions of the planted set; tests/test_gpu_census.py holds the
device to it exactly.

  census        count[key] = sum over the sequences of the length of key's list in np_index(text, mask, mode); a zero key is
                never counted; n_visited = n_counted + n_zero_keys
  histogram     hist[0] = 2^bits - n_distinct, hist[v] = keys with count v, hist[cap - 1] = keys with count >= cap - 1
  cutoff        the smallest c in [max(floor, 1), cap - 2] with at most int(fraction * n_distinct) distinct keys above it
  masking       a probe entry whose key has count > max_occ is taken out; the probe table is built from the rest
"""
import numpy as np

import index_ref as ir
import overlap_ref as orf

ACGT = np.frombuffer(b"ACGT", np.uint8)
U32_MAX = 0xFFFFFFFF
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits_of(mask: int) -> int:
    return bin(mask).count("1")


def visited(n: int, mode: str) -> np.ndarray:
    """the positions a sequence of n bases has visited, in visiting order (index_ref.visit_order; its second value is what
    get_seedmap returns, which wraps for n < 16 and is not used here)"""
    return ir.visit_order(n, mode)[0]


def census(texts, mask: int, mode: str) -> dict:
    """dict(count = {key: occurrences}, n_visited, n_counted, n_zero_keys, n_seqs) of the texts under (mask, mode)"""
    parts, n_visited = [], 0
    for t in texts:
        keys, _, _ = ir.np_index(t, mask, mode)
        parts.append(keys)
        n_visited += int(visited(len(t), mode).size)
    keys = np.concatenate(parts) if parts else np.zeros(0, np.uint32)
    k, c = np.unique(keys, return_counts=True)
    return dict(count=dict(zip(k.tolist(), c.tolist())), n_visited=n_visited, n_counted=int(keys.size),
                n_zero_keys=n_visited - int(keys.size), n_seqs=len(texts))


def merged(a: dict, b: dict) -> dict:
    """the census of two sets added into the same counters"""
    count = dict(a["count"])
    for k, v in b["count"].items():
        count[k] = count.get(k, 0) + v
    return dict(count=count, **{f: a[f] + b[f] for f in ("n_visited", "n_counted", "n_zero_keys", "n_seqs")})


def lookup(cen: dict, keys, mask: int) -> np.ndarray:
    return np.array([cen["count"].get(int(k) & mask, 0) if int(k) & mask else 0 for k in keys], np.uint32)


def histogram(cen: dict, mask: int, cap: int):
    """(hist u64[cap], n_distinct, max_count)"""
    assert cap >= 2
    c = np.array(list(cen["count"].values()), np.int64)
    hist = np.bincount(np.minimum(c, cap - 1), minlength=cap).astype(np.uint64)
    hist[0] = (1 << bits_of(mask)) - c.size
    return hist, int(c.size), int(c.max()) if c.size else 0


def cutoff(hist, fraction: float, floor: int = 1):
    """the occurrence cutoff, or None where the device answers PBA_E_TOOLONG"""
    hist = [int(x) for x in hist]
    cap = len(hist)
    n_distinct = sum(hist[1:])
    budget = int(fraction * n_distinct)                       # FP64 product, truncated
    above = n_distinct                                        # distinct keys with count > c, c = 0
    for c in range(1, cap - 1):                               # c <= cap - 2: the keys above c are counted exactly
        above -= hist[c]
        if c >= floor and above <= budget:
            return c
    return None


def read_repeats(cen: dict, texts, mask: int, mode: str, max_occ: int):
    """(n_over, n_visited) per text: visited positions whose key is nonzero with count > max_occ, visited positions"""
    over, vis = [], []
    for t in texts:
        pos = visited(len(t), mode)
        keys = (ir.np_keys(t)[pos] & np.uint32(mask)).tolist() if pos.size else []
        over.append(sum(1 for k in keys if k and cen["count"].get(k, 0) > max_occ))
        vis.append(int(pos.size))
    return np.array(over, np.uint32), np.array(vis, np.uint32)


def masked_entries(entries: np.ndarray, cen: dict, max_occ: int):
    """(the probe entries key << 32 | probe id that stay, sorted; how many were taken out): an entry goes when its key has
    count > max_occ; all-ones slots are padding and neither stay nor count"""
    entries = np.asarray(entries, np.uint64)
    entries = entries[entries != ALL_ONES]
    keep = np.array([cen["count"].get(int(e) >> 32, 0) <= max_occ for e in entries], bool)
    return np.sort(entries[keep]), int((~keep).sum())


def masked_composition(oracle, texts, qtexts, R: float, mask: int, max_trial: int, overlap_min: int, cen: dict, max_occ: int,
                       cache=None, t_lo: int = 0, t_hi=None):
    """What pba_overlap_strands_masked has to answer for one strand (qtexts: the query texts of that strand, None = texts):
    the probe table with the over-frequent keys' probes removed, overlap_ref.candidates over it, and walk_composition's
    first-success loop over the oracle's verdicts (a candidate behind its run's first success is never aligned, as there).
    dict(rows = [(target, query, j, dir, ref_pos, cost, matlen_a, matlen_b)], n_match, pairs, pairs_by, n_probe_entries,
    n_masked)."""
    qtexts = texts if qtexts is None else qtexts
    table = orf.ProbeTable(qtexts, mask, max_trial)
    before = table.n_entries
    table.by_key = {k: v for k, v in table.by_key.items() if cen["count"].get(k, 0) <= max_occ}
    table.n_entries = sum(len(v) for v in table.by_key.values())
    cands, n_match = orf.candidates(texts, qtexts, mask, max_trial, overlap_min, table, t_lo, t_hi)
    cache = {} if cache is None else cache
    rows, pairs_by, done = [], {}, None
    for t, q, jd, k, p in cands:
        if done == (t, q):
            continue
        x = cache.get((t, qtexts[q], jd, p))
        if x is None:
            a, b = orf.sides(texts[t], qtexts[q], jd, p)
            x = cache[(t, qtexts[q], jd, p)] = oracle.align(a, b, R)
        pairs_by[(t, q)] = pairs_by.get((t, q), 0) + 1
        if x["rc"] > 0 and x["matlen_a"] >= overlap_min:
            done = (t, q)
            rows.append((t, q, jd >> 1, -1 if jd & 1 else 1, p, x["cost"], x["matlen_a"], x["matlen_b"]))
    return dict(rows=rows, n_match=n_match, pairs=sum(pairs_by.values()), pairs_by=pairs_by, n_probe_entries=table.n_entries,
                n_masked=before - table.n_entries)


# ----------------------------------------------------------------------------- inputs: the edges of the count kernel
def edge_lengths():
    """the chunk (16 positions), wavefront (1 024), workgroup pass (4 096) and tile (16 384 visited positions: 16 399 bases
    head_tail) edges of the walk, and the head / tail / middle edges of get_seedmap (20 016, 40 016)"""
    return [0, 1, 15, 16, 17, 31, 32, 33, 1023, 1024, 1025, 4095, 4096, 4097, 16399, 20015, 20016, 20017, 20032, 40015, 40016,
            40017, 40100]


SHAPES = ("random", "all_t", "all_a", "period2", "period7")


def edge_texts(shape: str, seed: int = 7):
    """one text per edge length: random bases, all T (every key is the mask itself), all A (only zero keys, but for the padded
    windows at the end in mode "all"), period 2 and period 7 (two and seven keys, counted many times each)"""
    rng = np.random.default_rng(seed)
    out = []
    for n in edge_lengths():
        if shape == "random":
            out.append(rng.choice(ACGT, n).tobytes())
        elif shape == "all_t":
            out.append(b"T" * n)
        elif shape == "all_a":
            out.append(b"A" * n)
        elif shape == "period2":
            out.append((b"GT" * (n // 2 + 1))[:n])
        else:
            out.append((b"ACGGTCA" * (n // 7 + 1))[:n])
    return out


W13_PAT = "111*11*1111*1111"
MASKS = {"w1": orf.mask_of("*****1**********"), "w2": orf.mask_of("***1********1***"), "w12": orf.mask_of("111*11*11*1*1111"),
         "w13": orf.mask_of(W13_PAT)}
MASK_27_BITS = MASKS["w13"] | 1 << 10           # one more bit of a don't-care base: one care bit too many for direct addressing
assert [bits_of(m) for m in MASKS.values()] == [2, 4, 24, 26] and bits_of(MASK_27_BITS) == 27


# ----------------------------------------------------------------------------- inputs: a read set with planted repeats
PLANTED = dict(R=0.2, max_trial=8, overlap_min=64, max_occ=3)
ELEMENT_AT, ELEMENT_LEN = (700, 2600, 4700, 6900), 300
SATELLITE_AT, SATELLITE_LEN = 3600, 200


def repeat_intervals():
    return [(a, a + ELEMENT_LEN) for a in ELEMENT_AT] + [(SATELLITE_AT, SATELLITE_AT + SATELLITE_LEN)]


def planted_reads(seed: int = 2024):
    """(texts, meta) -- meta[i] = (genome start, genome end, strand).  An 8 kb random genome with one 300-base element at four
    loci and a 200-base satellite of period 5; 40 reads of 500 .. 1 200 bases at about 8 % error (3 % substitutions, 2.5 %
    deletions, 2.5 % insertions), every second one reverse-complemented; 32 of them on a grid of starts, 8 placed so that they
    start or end inside a copy of the element or inside the satellite."""
    rng = np.random.default_rng(seed)
    G = rng.choice(ACGT, 8000)
    elem = rng.choice(ACGT, ELEMENT_LEN)
    for a in ELEMENT_AT:
        G[a:a + ELEMENT_LEN] = elem
    G[SATELLITE_AT:SATELLITE_AT + SATELLITE_LEN] = np.tile(np.frombuffer(b"ACGAT", np.uint8), SATELLITE_LEN // 5)
    spans = []
    for i in range(32):
        s = int(i * 225 + rng.integers(0, 60))
        spans.append((s, min(8000, s + int(rng.integers(500, 1201)))))
    spans += [(760, 1500), (2750, 3400), (3650, 4400), (3700, 4600),          # start inside a copy / inside the satellite
              (100, 850), (1900, 2800), (2900, 3720), (6000, 7100)]           # end inside one
    texts, meta = [], []
    for i, (s, e) in enumerate(spans):
        out = []
        for b in G[s:e].tolist():
            u = rng.random()
            if u < 0.03:
                out.append(int(ACGT[(int(np.flatnonzero(ACGT == b)[0]) + int(rng.integers(1, 4))) % 4]))
            elif u < 0.055:
                continue
            elif u < 0.08:
                out += [b, int(rng.choice(ACGT))]
            else:
                out.append(b)
        t = bytes(out)
        strand = -1 if i & 1 else 1
        texts.append(orf.comp(t) if strand < 0 else t)
        meta.append((s, e, strand))
    return texts, meta


def unique_overlap(ma, mb) -> int:
    """bases two reads share on the genome outside every planted copy"""
    lo, hi = max(ma[0], mb[0]), min(ma[1], mb[1])
    if hi <= lo:
        return 0
    return (hi - lo) - sum(max(0, min(hi, e) - max(lo, s)) for s, e in repeat_intervals())


def planted_compositions(oracle, max_occ=None, cache=None):
    """{strand: (unmasked composition, masked composition)} of the planted set at PLANTED (max_occ: another cutoff), and the census"""
    P = PLANTED
    texts, _ = planted_reads()
    mask = MASKS["w12"]
    cen = census(texts, mask, "head_tail")
    rc_texts = [orf.comp(t) for t in texts]
    cache = {} if cache is None else cache
    out = {}
    for strand, q in ((1, None), (-1, rc_texts)):
        args = (oracle, texts, q, P["R"], mask, P["max_trial"], P["overlap_min"], cen)
        out[strand] = (masked_composition(*args, U32_MAX, cache), masked_composition(*args, P["max_occ"] if max_occ is None else max_occ, cache))
    return out, cen


def strand_rows(comps, which: int):
    """[(target, query, strand, j, dir, ref_pos, cost, matlen_a, matlen_b)] sorted by (target, query, strand), +1 before -1:
    the order of pba_overlap_strands; which: 0 unmasked, 1 masked"""
    rows = [(r[0], r[1], s) + tuple(r[2:]) for s in (1, -1) if s in comps for r in comps[s][which]["rows"]]
    return sorted(rows, key=lambda r: (r[0], r[1], -r[2]))
