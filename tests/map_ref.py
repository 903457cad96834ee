"""pba_map_reads as plain Python over the C oracle's pieces, independent of the engine.

map_reads_ref restates locator.cpp:70-92 for a target of many contigs and both strands of the reads.  Per read and strand:
for j < min(trials, len), the key is Oracle.encode of the window at j padded with code 3 (a 'T'), & mask; key 0 is skipped
(locator.cpp:64); the hits are the per-contig Oracle.index(contig, mask, "all") lists concatenated in contig order; each is
handed to Oracle.align(read[j:], contig[pos:], R); the walk stops at the first rc > 0.  strands == 3 walks every read on +,
then the reads with len >= min_len that found nothing again as their reverse complement; the first success is the row and
n_pairs is summed.  tests/test_map_ref_cpu.py pins it to Oracle.locator on one contig.

Also here: the interval arithmetic of pba_map_row (intervals), the merge of two one-strand answers (merge_strands) and the
builders of the inputs tests/test_gpu_map.py uses, so that their seeds can be chosen on the CPU.
"""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")

MAP_REF_DTYPE = np.dtype([(n, "<i4") for n in
                          ("read", "nseq", "found", "strand", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b",
                           "n_pairs", "r_beg", "r_end", "c_beg", "c_end")])
STAT_KEYS = ("n_reads_kept", "n_probe_hits", "n_pairs", "n_located", "n_cells")


def rc(x: bytes) -> bytes:
    return x.translate(_COMP)[::-1]


def intervals(strand: int, found: int, j: int, pos: int, matlen_a: int, matlen_b: int, read_len: int):
    """(r_beg, r_end, c_beg, c_end) of a pba_map_row: half-open, forward strand of the read / of the contig; zeros when
    nothing was found.  a = the read from j, b = the contig from pos."""
    if not found:
        return 0, 0, 0, 0
    if strand > 0:
        return j, j + matlen_a, pos, pos + matlen_b
    return read_len - j - matlen_a, read_len - j, pos, pos + matlen_b


class SetIndex:
    """The per-contig Oracle.index(..., "all") lists; hits(key) concatenates them in contig order."""

    def __init__(self, oracle, contigs, mask):
        self.per = []
        for c in contigs:
            if len(c) == 0:
                self.per.append((np.zeros(0, np.uint32), np.zeros(0, np.int32)))
            else:
                keys, pos, _, _ = oracle.index(c, mask, "all")
                self.per.append((keys, pos))

    def hits(self, key: int):
        """[(contig, pos), ...] in list order."""
        out = []
        for c, (keys, pos) in enumerate(self.per):
            lo, hi = np.searchsorted(keys, key, "left"), np.searchsorted(keys, key, "right")
            out.extend((c, int(p)) for p in pos[lo:hi])
        return out


def walk_one(oracle, six, contigs, read: bytes, mask: int, R: float, trials: int):
    """One read on the strand it is given.  Returns a dict: found, contig, j, pos, cost, seglen, matlen_a, matlen_b, n_pairs,
    n_probe_hits, n_cells, and -- for a success -- rank (the hit's place in its key's list) and first_contig (the first
    contig holding that key)."""
    out = dict(found=0, contig=-1, j=-1, pos=-1, cost=-1, seglen=0, matlen_a=0, matlen_b=0, n_pairs=0, n_probe_hits=0, n_cells=0,
               rank=-1, first_contig=-1)
    n = len(read)
    for j in range(min(trials, n)):
        key = oracle.encode(read[j:j + 16].ljust(16, b"T")) & mask
        if key == 0:
            continue
        hits = six.hits(key)
        if not hits:
            continue
        out["n_probe_hits"] += 1
        for rank, (c, pos) in enumerate(hits):
            res = oracle.align(read[j:], contigs[c][pos:], R)
            out["n_pairs"] += 1
            out["n_cells"] += res["cells"]
            if res["rc"] > 0:
                out.update(found=1, contig=c, j=j, pos=pos, cost=res["cost"], seglen=n - j, matlen_a=res["matlen_a"],
                           matlen_b=res["matlen_b"], rank=rank, first_contig=hits[0][0])
                return out
    return out


def map_reads_ref(oracle, contigs, reads, mask: int, R: float, trials: int = 50, min_len: int = 500, strands: int = 3):
    """(rows of MAP_REF_DTYPE, [stats of the + walk, of the - walk], walks): walks[r] = {+1: dict, -1: dict} of walk_one
    for the strands read r was walked on."""
    six = SetIndex(oracle, contigs, mask)
    rows = np.zeros(len(reads), MAP_REF_DTYPE)
    stats = [dict.fromkeys(STAT_KEYS, 0) for _ in range(2)]
    walks = []
    nseq = 0
    for r, text in enumerate(reads):
        kept = len(text) >= min_len
        mine = {}
        if kept and strands & 1:
            mine[1] = walk_one(oracle, six, contigs, text, mask, R, trials)
        if kept and strands & 2 and not (mine.get(1) or {}).get("found"):
            mine[-1] = walk_one(oracle, six, contigs, rc(text), mask, R, trials)
        walks.append(mine)
        for k, s in ((0, 1), (1, -1)):
            if s in mine:
                w = mine[s]
                stats[k]["n_reads_kept"] += 1
                stats[k]["n_probe_hits"] += w["n_probe_hits"]; stats[k]["n_pairs"] += w["n_pairs"]
                stats[k]["n_located"] += w["found"]; stats[k]["n_cells"] += w["n_cells"]
        win_s = next((s for s in (1, -1) if s in mine and mine[s]["found"]), 0)
        row = rows[r]
        row["read"] = r
        row["nseq"] = nseq if kept else -1
        nseq += kept
        w = mine[win_s] if win_s else dict(found=0, contig=-1, j=-1, pos=-1, cost=-1, seglen=0, matlen_a=0, matlen_b=0)
        for k in ("found", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b"):
            row[k] = w[k]
        row["strand"] = win_s
        row["n_pairs"] = sum(x["n_pairs"] for x in mine.values())
        row["r_beg"], row["r_end"], row["c_beg"], row["c_end"] = intervals(win_s, w["found"], w["j"], w["pos"], w["matlen_a"],
                                                                           w["matlen_b"], len(text))
    return rows, stats, walks


def merge_strands(plus, minus, read_lens, contig: int = 0):
    """One-contig rows of Oracle.locator on the reads (plus) and on their reverse complements (minus), merged as
    pba_map_reads(strands = 3) merges its walks: the + row if found, else the - row; n_pairs summed -- a read found on + is
    not walked on -, so its - pairs do not count."""
    rows = np.zeros(len(plus), MAP_REF_DTYPE)
    for r in range(len(plus)):
        p, m = plus[r], minus[r]
        s = 1 if p["found"] else (-1 if m["found"] else 0)
        w = p if s >= 0 else m
        row = rows[r]
        row["read"], row["nseq"], row["found"], row["strand"] = r, p["nseq"], w["found"], s
        row["contig"] = contig if s else -1
        for k in ("j", "pos", "cost", "seglen", "matlen_a", "matlen_b"):
            row[k] = w[k]
        row["n_pairs"] = int(p["n_pairs"]) + (0 if p["found"] else int(m["n_pairs"]))
        row["r_beg"], row["r_end"], row["c_beg"], row["c_end"] = intervals(s, int(w["found"]), int(w["j"]), int(w["pos"]),
                                                                           int(w["matlen_a"]), int(w["matlen_b"]), int(read_lens[r]))
    return rows


# ----------------------------------------------------------------------------- inputs
def rand_text(rng, n: int) -> bytes:
    return ACGT[rng.integers(0, 4, n)].tobytes()


def mutate(rng, text: bytes, p: float, keep: int = 0) -> bytes:
    """text with per-base substitution / insertion / deletion at p / 3 each; the first `keep` bases stay as they are."""
    out = bytearray()
    u = rng.random(len(text))
    ins = rng.integers(0, 4, len(text))
    for i, ch in enumerate(text):
        if i < keep or u[i] >= p:
            out.append(ch)
        elif u[i] < p / 3:
            out.append(b"ACGT"[(b"ACGT".index(ch) + 1 + ins[i] % 3) % 4])      # substitution: another base
        elif u[i] < 2 * p / 3:
            out.append(ch); out.append(b"ACGT"[ins[i]])                       # insertion
        # else: deletion
    return bytes(out)


MANY_LENS = [40000, 0, 3000, 12, 17000, 9000, 25000, 5000]     # 8 contigs of 3 - 40 kb, one empty, one of 12 bases


def many_contig_case(seed: int, n_reads: int = 400, err: float = 0.12, trials: int = 50, min_len: int = 500):
    """(contigs, reads, flipped): MANY_LENS contigs and n_reads reads of 600 - 2 000 bases at `err` error.  For every
    non-degenerate contig: reads that start at its position 0 and within `trials` bases of it (first 20 bases kept exact),
    and reads whose segment ends on its last base (some with a random overhang, so that the read's remainder is longer than
    the contig's).  20 reads are found nowhere (10 random, 10 random behind an exact 40-base prefix of a contig: hits that
    fail), 10 are below min_len.  Every second read, by a seeded draw, is reverse-complemented."""
    rng = np.random.default_rng(seed)
    contigs = [rand_text(rng, n) for n in MANY_LENS]
    real = [c for c, n in enumerate(MANY_LENS) if n >= 600]
    reads = []
    for c in real:
        T = contigs[c]
        for s in (0, 0, 7, 33, trials - 1):
            L = int(rng.integers(600, min(2000, len(T) - s) + 1))
            reads.append(mutate(rng, T[s:s + L], err, keep=20))
        for over in (0, 0, 0, 30):
            L = int(rng.integers(600, min(2000, len(T)) + 1))
            reads.append(mutate(rng, T[len(T) - L:], err, keep=20) + rand_text(rng, over))
    for k in range(20):
        x = rand_text(rng, int(rng.integers(600, 2001)))
        if k >= 10:
            T = contigs[real[k % len(real)]]
            s = int(rng.integers(0, len(T) - 40))
            x = T[s:s + 40] + x[40:]
        reads.append(x)
    for _ in range(10):
        T = contigs[real[int(rng.integers(0, len(real)))]]
        L = int(rng.integers(100, min_len))
        s = int(rng.integers(0, len(T) - L))
        reads.append(mutate(rng, T[s:s + L], err))
    w = np.array([len(contigs[c]) for c in real], float)
    while len(reads) < n_reads:
        T = contigs[real[int(rng.choice(len(real), p=w / w.sum()))]]
        L = int(rng.integers(600, min(2000, len(T)) + 1))
        s = int(rng.integers(0, len(T) - L + 1))
        reads.append(mutate(rng, T[s:s + L], err))
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    flipped = rng.integers(0, 2, len(reads)).astype(bool)
    reads = [rc(x) if f else x for x, f in zip(reads, flipped)]
    return contigs, reads, flipped


def repeat_case(seed: int, n_reads: int = 50, copies: int = 100, n_contigs: int = 5, seg_len: int = 300, err: float = 0.08):
    """(contigs, reads, copy_of): one seg_len-base segment planted `copies` times, spread evenly over n_contigs contigs with
    random spacers of 100 - 300 bases between the copies; read k starts inside copy copy_of[k] (chosen evenly over all the
    copies, so that some lie in the last contigs and behind more than 64 earlier copies) and runs 700 bases on, through the
    spacers and copies that follow, with its first 20 bases kept exact."""
    rng = np.random.default_rng(seed)
    seg = rand_text(rng, seg_len)
    contigs, where = [], []
    per = copies // n_contigs
    for c in range(n_contigs):
        t = bytearray(rand_text(rng, 200))
        for _ in range(per):
            where.append((c, len(t)))
            t += seg
            t += rand_text(rng, int(rng.integers(100, 301)))
        t += rand_text(rng, 900)
        contigs.append(bytes(t))
    copy_of = np.linspace(0, copies - 1, n_reads).astype(int)
    reads = []
    for k in copy_of:
        c, at = where[k]
        off = int(rng.integers(0, seg_len - 40))
        reads.append(mutate(rng, contigs[c][at + off:at + off + 700], err, keep=20))
    return contigs, reads, copy_of
