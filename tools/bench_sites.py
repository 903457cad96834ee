#!/usr/bin/env python3
"""What the site scan and the allele walk cost (pba_pileup_sites, pba_overlap_rows_alleles) on a synthetic
diploid: two haplotypes of one genome that differ by a planted substitution or single-base deletion every --het bases, --reads
reads of --len bases drawn from both at --coverage, 5 % insertions, deletions and substitutions each, every second one
reverse-complemented; all-vs-all on both strands, every row voting on its target.
  scan   pba_pileup_sites on a voted pile-up, next to pba_pileup_evolve on the same pile-up (the scan only reads it, so it runs
         first, --scan-reps times; evolve spends it): whole calls -- flag pass, two scans, compaction, the records back on the
         host -- and GB/s against the 20 bytes per box the flag pass must read.
  walk   pba_overlap_rows_alleles next to pba_overlap_rows_windows (W = --window) on the same rows, alternating: the sibling sink
         over the same walk; rows/s.
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
ap.add_argument("--window", type=int, default=100)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--scan-reps", type=int, default=5)
a = ap.parse_args()

ctx = Context(0)
mask = eng.mask_from_pattern("111*11*11*1*1111")
n = a.reads
h0 = eng.synth_genome(2, max(int(n * a.len / a.coverage), 2 * a.len))
rng = np.random.default_rng(5)
at = np.arange(a.het, h0.size - a.het, a.het)
sub = at[::2]
h1 = h0.copy()
acgt = np.frombuffer(b"ACGT", np.uint8)
code = np.searchsorted(acgt, h0[sub])
h1[sub] = acgt[(code + rng.integers(1, 4, sub.size)) % 4]
h1 = np.delete(h1, at[1::2])
parts = [eng.synth_reads(3 + h, hap, n // 2 + (h if n % 2 else 0), a.len, 0.05, 0.05, 0.05, nthreads=16)[0] for h, hap in enumerate((h0, h1))]
text = np.concatenate(parts)
offs = np.arange(n + 1, dtype=np.uint64) * np.uint64(a.len)
S0 = ctx.seqs_from_text(text, offs, strict_acgt=True)
S = ctx.seqs_revcomp(S0, np.random.default_rng(4).integers(0, 2, n).astype(np.uint8))
S0.close()
Rc = ctx.seqs_revcomp(S)
rows, _ = ctx.overlap_strands_sharded(S, mask, a.R, 32, 64, reads_rc=Rc)
boxes = int(S.lengths().astype(np.int64).sum())


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


def one_pile(timed: bool):
    """a fresh voted pile-up scanned --scan-reps times and then evolved: (scan ms list, evolve ms, sites of the last scan)"""
    p = Pileup(ctx, S, weight=a.weight)
    p.vote(rows, a.R, reads_rc=Rc)
    scans, sites = [], None
    for _ in range(a.scan_reps if timed else 1):
        if sites is not None:
            sites.close()
        sites, ms = events(lambda: p.sites(*a.thresholds))
        scans.append(ms)
    out, ms = events(p.evolve)
    out[0].close()
    p.close()
    return scans, ms, sites


_, _, sites = one_pile(False)                                # warm-up, and the sites the walk uses
scan_ms, evolve_ms = [], []
for _ in range(max(1, a.reps)):
    s, e, x = one_pile(True)
    x.close()
    scan_ms += s
    evolve_ms.append(e)

walks = {"alleles": lambda: ctx.overlap_alleles(S, rows, a.R, sites, reads_rc=Rc, cap=0),
         "windows": lambda: ctx.overlap_windows(S, rows, a.R, a.window, reads_rc=Rc, cap=0)}
totals = {}
for k, fn in walks.items():                                  # warm-up; cap = 0: the walk and the slots' way back, no second call
    out = fn()
    totals[k] = int(out[1][-1]) if k == "alleles" else int(out[4])
walk_ms = {k: [] for k in walks}
for rep in range(max(1, a.reps)):
    for k in (list(walks) if rep % 2 == 0 else list(walks)[::-1]):
        walk_ms[k].append(events(walks[k])[1])

recs = sites.get()
res = {"workload": f"diploid: {n} x {a.len} reads at {a.coverage}x of two haplotypes differing every {a.het} bases, {len(rows)} rows voting",
       "boxes": boxes, "rows": int(len(rows)), "thresholds": list(a.thresholds), "sites": int(recs.size),
       "sel_sites": int((recs["kind"] == eng.PBA_SITE_SEL).sum()), "allele_records": totals["alleles"], "windows": totals["windows"],
       "scan_ms": spread(scan_ms), "evolve_ms": spread(evolve_ms),
       "scan_gb_per_s": round(boxes * 20 / (statistics.median(scan_ms) * 1e-3) / 1e9, 1),
       "alleles_ms": spread(walk_ms["alleles"]), "windows_ms": spread(walk_ms["windows"]),
       "alleles_rows_per_s": round(len(rows) / (statistics.median(walk_ms["alleles"]) * 1e-3)),
       "windows_rows_per_s": round(len(rows) / (statistics.median(walk_ms["windows"]) * 1e-3))}
print(json.dumps(res))
