#!/usr/bin/env python3
"""What phasing overlap rows by their alleles costs, and what it buys read correction (pba_overlap_rows_phase,
pba_correct_reads_phased), on bench_sites.py's synthetic diploid: two haplotypes of one genome that differ by a
planted substitution or single-base deletion every --het bases, --reads reads of --len bases drawn from both at --coverage, 5 %
insertions, deletions and substitutions each, every second one reverse-complemented; all-vs-all on both strands.
  phase    pba_overlap_rows_phase next to pba_overlap_rows_alleles on the same rows and sites, alternating: the allele walk it
           follows plus gather, classify, 2 x n_iter + 1 passes; the call's own split (its walks, its phase kernels) beside it.
  correct  pba_correct_reads_phased next to pba_correct_reads on the same reads, alternating: three walks against one.
  share    both corrected sets mapped to haplotype 0 and their alleles read at the planted positions: the share of (read,
           planted site) pairs at which a read carries its own haplotype's allele.
Each call is timed between two HIP events after a device-wide synchronise; one warm-up of everything that is timed; prints one
JSON line with median / min / max of each."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import numpy as np
import torch
from pacbioassembly_amd import Context, Pileup, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=20_000)
ap.add_argument("--len", type=int, default=15_000)
ap.add_argument("--coverage", type=float, default=20.0)
ap.add_argument("--het", type=int, default=1000, help="bases between planted differences of the two haplotypes")
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--weight", type=int, default=1)
ap.add_argument("--thresholds", type=int, nargs=3, default=(8, 3, 250), metavar=("MIN_DEPTH", "MIN_ALT", "MIN_PERMILLE"))
ap.add_argument("--params", type=int, nargs=3, default=(2, 2, 1), metavar=("N_ITER", "MIN_MARGIN", "SELF_WEIGHT"))
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()

ctx = Context(0)
mask = eng.mask_from_pattern("111*11*11*1*1111")
n = a.reads
h0 = eng.synth_genome(2, max(int(n * a.len / a.coverage), 2 * a.len))
rng = np.random.default_rng(5)
at = np.arange(a.het, h0.size - a.het, a.het)
sub, dele = at[::2], at[1::2]
h1 = h0.copy()
acgt = np.frombuffer(b"ACGT", np.uint8)
code = np.searchsorted(acgt, h0[sub])
alt = (code + rng.integers(1, 4, sub.size)) % 4
h1[sub] = acgt[alt]
h1 = np.delete(h1, dele)
n_hap = [n // 2 + (h if n % 2 else 0) for h in (0, 1)]
parts = [eng.synth_reads(3 + h, hap, n_hap[h], a.len, 0.05, 0.05, 0.05, nthreads=16)[0] for h, hap in enumerate((h0, h1))]
text = np.concatenate(parts)
offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(a.len)
S0 = ctx.seqs_from_text(text, offs, strict_acgt=True)
S = ctx.seqs_revcomp(S0, np.random.default_rng(4).integers(0, 2, n).astype(np.uint8))
S0.close()
Rc = ctx.seqs_revcomp(S)
rows, _ = ctx.overlap_strands_sharded(S, mask, a.R, 32, 64, reads_rc=Rc)


def events(fn):
    """fn() between two HIP events on the null stream, after a device-wide synchronise on both sides"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def spread(vals):
    return {"median": round(statistics.median(vals), 3), "min": round(min(vals), 3), "max": round(max(vals), 3)}


p = Pileup(ctx, S, weight=a.weight)
p.vote(rows, a.R, reads_rc=Rc)
sites = p.sites(*a.thresholds)
p.close()

calls = {"alleles": lambda: ctx.overlap_alleles(S, rows, a.R, sites, reads_rc=Rc, cap=0),
         "phase": lambda: ctx.overlap_phase(S, rows, a.R, sites, *a.params, reads_rc=Rc),
         "correct": lambda: ctx.correct_reads(S, mask, a.R, 32, 64, weight=a.weight, reads_rc=Rc),
         "correct_phased": lambda: ctx.correct_reads_phased(S, mask, a.R, tuple(a.thresholds), *a.params, weight=a.weight, reads_rc=Rc)}
kept = {}
for k, fn in calls.items():                                   # warm-up, and the results the report reads
    kept[k] = fn()
ms = {k: [] for k in calls}
inner = {"walks": [], "kernels": []}
for rep in range(max(1, a.reps)):
    for pair in (("alleles", "phase"), ("correct", "correct_phased")):
        for k in (pair if rep % 2 == 0 else pair[::-1]):
            out, t = events(calls[k])
            ms[k].append(t)
            if k == "phase":
                inner["walks"].append(out[2]["alleles_ms"]); inner["kernels"].append(out[2]["phase_ms"])
            if k.startswith("correct"):
                out[0].close()

# the share of planted sites at which a corrected read carries its own haplotype's allele
T = ctx.seqs_from_text(h0, np.array([0, h0.size], np.uint64), strict_acgt=True)
ix = ctx.index_build_set(T, mask)
want = np.zeros(at.size, eng.SITE_DTYPE)
want["pos"], want["kind"] = at, eng.PBA_SITE_SEL
own = np.searchsorted(acgt, h0[at])
want["own"], want["major"] = own, own
want["minor"][::2], want["minor"][1::2] = alt, eng.PBA_ALLELE_DEL
want["n"], want["n_major"], want["n_minor"] = 2, 1, 1
planted = ctx.sites_create(T, want)
hap_allele = np.stack([want["major"], want["minor"]]).astype(np.int64)       # [haplotype, site]
hap_of = np.repeat([0, 1], n_hap)
share = {}
for k, name in (("correct", "plain"), ("correct_phased", "phased")):
    C = kept[k][0]
    Cc = ctx.seqs_revcomp(C)
    mrows, _ = ctx.map_reads(ix, T, C, a.R, strands=3, reads_rc=Cc)
    out, off, _, _ = ctx.map_alleles(T, C, mrows, a.R, planted, 64, reads_rc=Cc)
    read = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    good = out["allele"].astype(np.int64) == hap_allele[hap_of[read], out["site"].astype(np.int64)]
    share[name] = round(float(good.mean()), 4) if good.size else 0.0
    share[name + "_pairs"] = int(good.size)
    Cc.close(); C.close()

pst, cst = kept["phase"][2], kept["correct_phased"][2]
res = {"workload": f"diploid: {n} x {a.len} reads at {a.coverage}x of two haplotypes differing every {a.het} bases, {len(rows)} rows",
       "rows": int(len(rows)), "thresholds": list(a.thresholds), "params": list(a.params), "sel_sites": int(pst["n_sites"]),
       "allele_records": int(pst["n_records"]), "rows_same": int(pst["n_same"]), "rows_other": int(pst["n_other"]),
       "rows_unphased": int(pst["n_unphased"]), "flipped_last": int(pst["n_flipped_last"]),
       "alleles_ms": spread(ms["alleles"]), "phase_ms": spread(ms["phase"]), "phase_walks_ms": spread(inner["walks"]),
       "phase_kernels_ms": spread(inner["kernels"]),
       "correct_ms": spread(ms["correct"]), "correct_phased_ms": spread(ms["correct_phased"]),
       "correct_rows_voted": int(kept["correct"][1]["n_rows"].sum()), "correct_phased_rows_voted": int(kept["correct_phased"][1]["n_rows"].sum()),
       "correct_phased_rows_other": int(cst["n_other"]), "own_allele_share": share}
print(json.dumps(res))
