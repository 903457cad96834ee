"""The phase rule of DESIGN §5.14 (include/pba.h: pba_alleles_phase, pba_overlap_rows_phase, pba_phase_rows_apply,
pba_correct_reads_phased) restated in plain numpy, independent of the engine -- the expectation the device is held to, exactly
(tests/test_gpu_phase.py), pinned by hand without a GPU (tests/test_phase_cpu.py) -- the correction of one target from the rows of
its own copy composed from the CPU oracle's pieces, and the planted input both tests share.

A record is (site, allele): `site` indexes the SITE records (tests/sites_ref.py) and names a SEL record.  v = +1 if allele ==
major, -1 if allele == minor, else 0; o0 = +1 if own == major, -1 if own == minor, else 0; lab(g) = sign(g) if |g| >= min_margin
else 0.  o(0) = o0; h(k)[r] = lab(sum o(k-1)[site] v); f(k)[s] = self_weight o0[s] + sum h(k)[row] v; o(k) = sign f(k);
g[r] = sum o(n_iter)[site] v, label = lab(g)."""
import numpy as np

import sites_ref as sr

ROW = np.dtype([(n, "<i4") for n in ("label", "score", "n_informative", "n_records")])
SITE = np.dtype([("site", "<u4")] + [(n, "<i4") for n in ("orient", "score", "n_agree", "n_disagree")])
STAT_FIELDS = ("n_rows", "n_same", "n_other", "n_unphased", "n_sites", "n_records", "n_flipped_last")


def value(site, allele: int) -> int:
    return 1 if allele == int(site["major"]) else (-1 if allele == int(site["minor"]) else 0)


def lab(g, min_margin: int):
    g = np.asarray(g, np.int64)
    return np.where(np.abs(g) >= min_margin, np.sign(g), 0)


def phase_ref(sites, rows_records, n_iter: int, min_margin: int, self_weight: int):
    """(rows of ROW, sites of SITE in SEL-rank order, stats): rows_records[r] = [(site index, allele)] of row r"""
    sel = [x for x, s in enumerate(sites) if int(s["kind"]) == sr.SEL]
    rank = {x: k for k, x in enumerate(sel)}
    o0 = np.array([value(sites[x], int(sites[x]["own"])) for x in sel], np.int64)
    n, ns = len(rows_records), len(sel)
    row_of, at, v = [], [], []
    for r, recs in enumerate(rows_records):
        for x, a in recs:
            row_of.append(r); at.append(rank[int(x)]); v.append(value(sites[int(x)], int(a)))
    row_of, at, v = np.array(row_of, np.int64), np.array(at, np.int64), np.array(v, np.int64)

    def row_sums(o):
        g = np.zeros(n, np.int64)
        np.add.at(g, row_of, o[at] * v)
        return g

    o, prev, f = o0.copy(), o0.copy(), self_weight * o0
    for _ in range(n_iter):
        h = lab(row_sums(o), min_margin)
        f = self_weight * o0
        np.add.at(f, at, h[row_of] * v)
        prev, o = o, np.sign(f)
    g = row_sums(o)
    label = lab(g, min_margin)
    rows = np.zeros(n, ROW)
    rows["label"], rows["score"] = label, g
    np.add.at(rows["n_informative"], row_of, (o[at] * v != 0).astype(np.int32))
    rows["n_records"] = [len(x) for x in rows_records]
    out = np.zeros(ns, SITE)
    out["site"], out["orient"], out["score"] = sel, o, f
    t = label[row_of] * v * o[at]
    np.add.at(out["n_agree"], at, (t > 0).astype(np.int32))
    np.add.at(out["n_disagree"], at, (t < 0).astype(np.int32))
    stats = dict(n_rows=n, n_same=int((label > 0).sum()), n_other=int((label < 0).sum()), n_unphased=int((label == 0).sum()), n_sites=ns,
                 n_records=int(v.size), n_flipped_last=int((o != prev).sum()) if n_iter else 0)
    return rows, out, stats


def apply(labels, keep_unphased: bool):
    """the indices of the rows kept"""
    return [k for k, x in enumerate(labels) if int(x) > 0 or (int(x) == 0 and keep_unphased)]


# ----------------------------------------------------------------------------- correction from the rows of the own copy
def correct_phased_ref(oracle, texts, t, rows_t, weight, R, thresholds, params, keep_unphased=True):
    """Target t through the CPU oracle's composition: every row aligned with traceback and elected (the boxes all rows vote into),
    sites_of over those boxes, alleles_from_script per row, phase_ref, a fresh consensus elected by the kept rows only, evolve.
    Returns dict(plain=text all rows evolve to, text=the phased text, kept=indices into rows_t, labels, sites, records, stats)."""
    from correct_helpers import pair_texts
    from pacbioassembly_amd import engine as eng
    T = texts[t]
    walks = []
    c = oracle.consensus(T, weight)
    for r in rows_t:
        pr = eng.overlap_row_pair(r, len(T), len(texts[int(r["query"])]))
        a, b, fwd = pair_texts(pr, texts, int(r["strand"]))
        res = oracle.align(a, b, R, a_fwd=fwd, b_fwd=fwd, want_ops=True)
        assert res["rc"] >= 0 and res["cost"] == int(r["cost"]) and res["matlen_a"] == int(r["matlen_a"]), (r, res)
        walks.append((int(pr["a_pos"]), fwd, res["ops"], b))
        c.elect(int(pr["a_pos"]), fwd, res["ops"], eng.script_vals(res["ops"], b, fwd))
    sel, sup, tot, _ = c.dump(len(T) + 8)
    c.evolve()
    plain = c.text(2 * len(T) + 8)
    n = len(T)
    sites = sr.sites_of(sel[:n], sup[:n], tot[:n], T, weight, thresholds, t)
    idx = [x for x, s in enumerate(sites) if int(s["kind"]) == sr.SEL]
    pos = [int(sites[x]["pos"]) for x in idx]
    records = [[(idx[k], a) for k, a in sr.alleles_from_script(ops, b if fwd else b[::-1], a_pos, not fwd, pos)]
               for a_pos, fwd, ops, b in walks]
    rows, psites, stats = phase_ref(sites, records, *params)
    kept = apply(rows["label"], keep_unphased)
    c2 = oracle.consensus(T, weight)
    for k in kept:
        a_pos, fwd, ops, b = walks[k]
        c2.elect(a_pos, fwd, ops, eng.script_vals(ops, b, fwd))
    c2.evolve()
    return dict(plain=plain, text=c2.text(2 * len(T) + 8), kept=kept, labels=rows["label"], rows=rows, sites=sites, records=records,
                stats=stats)


# ----------------------------------------------------------------------------- the planted input
# A smaller sibling of sites_ref.DIPLOID under the same generator: two haplotypes of one 10 kb sequence that differ by a planted
# substitution or single-base deletion every 97 bases, 160 reads of 2 kb, half from each, at 3 % error: 32x, 16x a haplotype.
# All-vs-all on both strands, every read a target.  A read's pile-up is as deep as the reads that overlap it: a site must show 8
# rows, 3 of them and a quarter of all on the second allele.  Two iterations, a row decided by a margin of 2, the target's own
# base counting once.
PLANTED = dict(sr.DIPLOID, seed=4713, glen=10000, first=500, last=9500, n_reads=160, thresholds=(8, 3, 250))
PARAMS = (2, 2, 1)          # n_iter, min_margin, self_weight


def wrong_pairs(oracle, h0, reads, hap_of, planted, mask, R):
    """(wrong, total): over the reads mapped to haplotype 0 by the CPU oracle and aligned with traceback, the (read, planted site)
    pairs where the read carries the OTHER haplotype's allele, and all pairs a read covers"""
    from map_ref import map_reads_ref
    from polish_helpers import row_texts
    rows, _, _ = map_reads_ref(oracle, [h0], reads, mask, R)
    pos = sorted(planted)
    wrong = total = 0
    for k, r in enumerate(rows):
        if not r["found"]:
            continue
        pr, a, b = row_texts(r, [h0], reads, R)
        o = oracle.align(a, b, R, want_ops=True)
        if o["rc"] < 0:
            continue
        for s, al in sr.alleles_from_script(o["ops"], b, int(pr["a_pos"]), False, pos):
            total += 1
            wrong += al == planted[pos[s]][2 - hap_of[k]]
    return wrong, total
