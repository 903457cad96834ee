"""The site rule and the per-row allele records of DESIGN §5.13 (include/pba.h: pba_pileup_sites, pba_sites_*,
pba_*_rows_alleles) restated in plain numpy and Python, independent of the engine -- the expectation the device is held to,
exactly (tests/test_gpu_sites.py), pinned by hand without a GPU (tests/test_sites_cpu.py) -- and the planted diploid input
both share.

A box is (sel[4], sup[4], tot) as Pileup.dump gives it, before evolve.  N = tot - 1 + weight; the five allele counts are the
four sel counters (the target's own base carries weight) and DEL = N - their sum; major is the first maximal allele in the
order A, C, G, T, DEL, minor the first maximal among the other four.  A script is the reference's: 1 MATCH (a and b advance),
2 INSERT (b advances), 3 DELETE (a advances), origin-first; a is the target."""
import numpy as np

SEL, SUP, DEL = 1, 2, 4
LETTERS = "ACGT-"
SITE = np.dtype([("target", "<i4"), ("pos", "<i4"), ("kind", "u1"), ("own", "u1"), ("major", "u1"), ("minor", "u1"), ("n", "<u4"),
                 ("n_major", "<u4"), ("n_minor", "<u4")])
SUM_FIELDS = ("n_sites", "n_own", "n_major", "n_minor", "n_other")
_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}


def code(ch: int) -> int:
    return _CODE[ch]


def passes(n: int, alt: int, th) -> bool:
    min_depth, min_alt, min_permille = th
    return n >= min_depth and alt >= min_alt and alt * 1000 >= min_permille * n


def box_call(sel, sup, tot, weight):
    """(N, five counts, major, minor, winning sup base, its counter) of one box"""
    c = [int(v) for v in sel]
    n = int(tot) - 1 + weight
    c.append(max(n - sum(c), 0))
    major = c.index(max(c))
    rest = [k for k in range(5) if k != major]
    minor = max(rest, key=lambda k: (c[k], -k))             # the first maximal among the others
    s = [int(v) for v in sup]
    return n, c, major, minor, s.index(max(s)), max(s)


def sites_of(sel, sup, tot, own_text: bytes, weight: int, thresholds, target: int = 0) -> np.ndarray:
    """the records of one target's boxes, sorted by (pos, kind): SEL before SUP where a box is both"""
    out = []
    for i in range(len(tot)):
        n, c, major, minor, sw, sv = box_call(sel[i], sup[i], tot[i], weight)
        own = code(own_text[i])
        if passes(n, c[minor], thresholds):
            out.append((target, i, SEL, own, major, minor, n, c[major], c[minor]))
        if passes(n, sv, thresholds):
            out.append((target, i, SUP, own, major, sw, n, 0, sv))
    return np.array(out, SITE) if out else np.zeros(0, SITE)


def alleles_from_script(ops, b_elems: bytes, a_pos: int, a_back: bool, site_positions):
    """[(index into site_positions, allele)] in ascending site order: site_positions are the target's SEL positions, ascending.
    A MATCH or DELETE that consumes a-element e sits at x = a_pos +/- e; an INSERT leaves nothing."""
    at = {int(x): k for k, x in enumerate(site_positions)}
    assert len(at) == len(site_positions) and list(site_positions) == sorted(site_positions)
    out, i, j = [], 0, 0
    for op in ops:
        op = int(op)
        assert op in (1, 2, 3)
        if op != 2:
            x = a_pos - i if a_back else a_pos + i
            if x in at:
                out.append((at[x], code(b_elems[j]) if op == 1 else DEL))
            i += 1
        if op != 3:
            j += 1
    out.sort()
    assert len({k for k, _ in out}) == len(out)              # every a-element is consumed once
    return out


def row_totals(records, sites):
    """the totals of one row: records [(site index, allele)], sites[k] the SITE record of site index k"""
    t = dict.fromkeys(SUM_FIELDS, 0)
    for k, a in records:
        s = sites[k]
        t["n_sites"] += 1
        t["n_own"] += a == int(s["own"])
        t["n_major"] += a == int(s["major"])
        t["n_minor"] += a == int(s["minor"])
        t["n_other"] += a != int(s["major"]) and a != int(s["minor"])
    return t


def histogram(n_sites: int, records):
    """allele counts per site over the records of many rows: [n_sites, 5]"""
    h = np.zeros((n_sites, 5), np.int64)
    for k, a in records:
        h[k, a] += 1
    return h


def box_counts(sel, tot, weight):
    """the five counts of every box: [n, 5]"""
    c = np.zeros((len(tot), 5), np.int64)
    c[:, :4] = sel
    c[:, 4] = np.maximum(tot.astype(np.int64) - 1 + weight - c[:, :4].sum(axis=1), 0)
    return c


def tsv_line(s, name=None) -> str:
    return "\t".join([str(int(s["target"])) if name is None else name, str(int(s["pos"]) + 1), "SEL" if int(s["kind"]) == SEL else "SUP",
                      LETTERS[int(s["own"])], LETTERS[int(s["major"])], LETTERS[int(s["minor"])], str(int(s["n"])), str(int(s["n_major"])),
                      str(int(s["n_minor"]))])


# ----------------------------------------------------------------------------- the planted diploid
# Two haplotypes of one 20 kb sequence: haplotype 1 differs from haplotype 0 by a planted substitution or a planted
# single-base deletion every 97 bases, alternating.  Haplotype 0 is the contig the reads are mapped to.  Around a deletion the
# contig reads ACGT and the C is lost, so that the cheapest alignment is unique and puts the gap on the planted box.  300
# reads of 2 kb, half from each haplotype, at 3 % error (1 % each kind): 30x, 15x a haplotype.  A site must show 10 rows, 4 of
# them and a quarter of all on the second allele: a sequencing error reaches that on no column at this depth, and half the
# rows carry a planted allele.
DIPLOID = dict(seed=4711, glen=20000, step=97, first=2000, last=18000, n_reads=300, rl=2000, err=0.03, R=0.30, overlap_min=64, weight=1,
               thresholds=(10, 4, 250))


def planted_diploid(D=DIPLOID):
    """(hap0, hap1, reads, hap_of, planted): planted = {position on hap0: (kind 'sub' | 'del', allele of hap0, allele of
    hap1)}; every second read, by a seeded draw, is reverse-complemented"""
    from map_ref import mutate, rand_text, rc
    rng = np.random.default_rng(D["seed"])
    h0 = bytearray(rand_text(rng, D["glen"]))
    planted = {}
    for k, p in enumerate(range(D["first"], D["last"], D["step"])):
        if k % 2:
            h0[p - 1:p + 3] = b"ACGT"
            planted[p] = ("del", code(h0[p]), DEL)
        else:
            alt = (code(h0[p]) + 1 + int(rng.integers(0, 3))) % 4
            planted[p] = ("sub", code(h0[p]), alt)
    h0 = bytes(h0)
    h1 = bytearray()
    for p, ch in enumerate(h0):
        if p in planted:
            if planted[p][0] == "sub":
                h1.append(ord("ACGT"[planted[p][2]]))
        else:
            h1.append(ch)
    h1 = bytes(h1)
    reads, hap_of = [], []
    for r in range(D["n_reads"]):
        h = r % 2
        src = h1 if h else h0
        s = int(rng.integers(0, len(src) - D["rl"] + 1))
        reads.append(mutate(rng, src[s:s + D["rl"]], D["err"], keep=20))
        hap_of.append(h)
    flip = rng.integers(0, 2, len(reads)).astype(bool)
    return h0, h1, [rc(x) if f else x for x, f in zip(reads, flip)], hap_of, planted


def planted_conditions(sites, planted, say=print):
    """what both planted tests require of the sites found on the contig: every planted site is found as a SEL site with the
    two haplotypes' alleles as major and minor, and at most 1 % of the reported sites (of either kind) are unplanted"""
    sel = {int(s["pos"]): s for s in sites if int(s["kind"]) == SEL}
    missing = [p for p in planted if p not in sel]
    wrong = [p for p in planted if p in sel and {int(sel[p]["major"]), int(sel[p]["minor"])} != {planted[p][1], planted[p][2]}]
    extra = [s for s in sites if int(s["pos"]) not in planted or int(s["kind"]) != SEL]
    say("planted", len(planted), "reported", len(sites), "missing", missing, "wrong alleles", wrong, "unplanted", len(extra))
    assert not missing and not wrong
    assert len(extra) * 100 <= len(sites)
    return len(extra)
