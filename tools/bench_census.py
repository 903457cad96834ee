#!/usr/bin/env python3
"""The seed-key census and repeat masking on synthetic reads with planted repeats: --reads reads of --len bases
@15 % error of a --genome genome into which THIS tool plants --copies copies of one 2 kb element and one 1 kb tandem satellite
of period 5 (seeded; the copies at seeded places that do not touch), a seeded random half reverse-complemented.  Prints one JSON
line and writes it to profiles/census_line.json:
  * the census of the reads (head_tail, the weight-12 mask): k_census_count's HIP-event time over --repeat fresh censuses
    (median and best) and visited positions per second; the same for a set of the same shape that is all T -- every add on one
    counter, the worst case for the plain one-atomic-per-key form -- and for the stock genome as one contig in mode "all";
  * in the same run, pba_seqs_revcomp on the same set (HIP events around the call) as the yardstick -- another read-a-set pass --
    and census / revcomp as a ratio.  No gate;
  * overlap_strands next to overlap_strands_masked at cutoff(--fraction): rows, n_candidates, n_pairs, kernel milliseconds (scan +
    sort + walk events) of each, and how many rows join two reads that share no unique base of the genome.
Nothing here is gated and the parent has nothing to compare with: a first measurement.  "runs" says how many runs stand
behind each figure."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pacbioassembly_amd import Context, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=3000)
ap.add_argument("--len", type=int, default=15_000, dest="read_len")
ap.add_argument("--copies", type=int, default=20)
ap.add_argument("--genome", type=int, default=5_000_000)
ap.add_argument("--fraction", type=float, default=0.001, help="share of the distinct keys the cutoff may give up")
ap.add_argument("--repeat", type=int, default=5, help="fresh censuses timed")
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--max-trial", type=int, default=32)
ap.add_argument("--overlap-min", type=int, default=64)
ap.add_argument("--out", default="census_line.json", help="file name under profiles/ (a tuning variant's line goes beside the real one)")
a = ap.parse_args()
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ELEMENT, SATELLITE = 2000, 1000

n, rl = a.reads, a.read_len
g = np.array(eng.synth_genome(2, a.genome), copy=True)
rng = np.random.default_rng(11)
element = rng.choice(np.frombuffer(b"ACGT", np.uint8), ELEMENT)
slots = rng.choice(a.genome // (2 * ELEMENT) - 1, a.copies + 1, replace=False) * (2 * ELEMENT)     # places that do not touch
planted = []
for at in slots[:-1].tolist():
    g[at:at + ELEMENT] = element
    planted.append((at, at + ELEMENT))
sat = int(slots[-1])
g[sat:sat + SATELLITE] = np.tile(np.frombuffer(b"ACGAT", np.uint8), SATELLITE // 5)
planted.append((sat, sat + SATELLITE))
text, offs, starts = eng.synth_reads(3, g, n, rl, 0.05, 0.05, 0.05, nthreads=16)
flip = rng.integers(0, 2, n).astype(bool)
reads = [text[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
reads = [t.translate(_COMP)[::-1] if f else t for t, f in zip(reads, flip)]
del text

ctx = Context(0)
mask = eng.mask_from_pattern("111*11*11*1*1111")


def events(fn):
    """fn() between two HIP events on the null stream, after a device-wide synchronise on both sides"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def timed_census(S, mode="head_tail"):
    ctx.census(S, mask, mode).close()                        # untimed: first launch, the pooled buffer
    ms, st = [], None
    for _ in range(a.repeat):
        c = ctx.census(S, mask, mode)
        st = c.stats
        ms.append(st["count_ms"])
        c.close()
    ms.sort()
    med = ms[len(ms) // 2]
    return {"count_ms_median": round(med, 4), "count_ms_best": round(ms[0], 4), "n_visited": int(st["n_visited"]), "n_zero_keys": int(st["n_zero_keys"]),
            "visited_per_s_median": round(st["n_visited"] / (med * 1e-3), 1) if med > 0 else None}


def unique_shared(i, k):
    lo, hi = max(int(starts[i]), int(starts[k])), min(int(starts[i]), int(starts[k])) + rl
    return (hi - lo) - sum(max(0, min(hi, e) - max(lo, s)) for s, e in planted) if hi > lo else 0


def found(rows, st2):
    no_locus = sum(1 for r in rows if unique_shared(int(r["target"]), int(r["query"])) <= 0)
    return {"rows": int(len(rows)), "rows_without_a_shared_unique_base": int(no_locus), "n_candidates": int(sum(s["n_candidates"] for s in st2)),
            "n_pairs": int(sum(s["n_pairs"] for s in st2)), "n_probe_entries": [int(s["n_probe_entries"]) for s in st2],
            "kernel_ms": round(sum(s[k] for s in st2 for k in ("scan_ms", "sort_ms", "walk_ms")), 2)}


S = ctx.seqs_from_list(reads, strict_acgt=True)
census_line = timed_census(S)
T = ctx.seqs_from_list([b"T" * len(t) for t in reads], strict_acgt=True)
one_key_line = timed_census(T)
T.close()
G = ctx.seqs_from_list([g.tobytes()], strict_acgt=True)
contig_line = timed_census(G, "all")
G.close()
ctx.seqs_revcomp(S).close()
rc_set, revcomp_ms = events(lambda: ctx.seqs_revcomp(S))
_, census_call_ms = events(lambda: ctx.census(S, mask).close())

cen = ctx.census(S, mask)
hist, n_distinct, max_count = cen.histogram(65536)
max_occ = cen.cutoff(a.fraction)
over, vis = cen.read_repeats(S, max_occ)
ctx.overlap_strands(S, mask, a.R, a.max_trial, a.overlap_min, reads_rc=rc_set)          # untimed: the work buffers of both calls
t = time.perf_counter()
plain = found(*ctx.overlap_strands(S, mask, a.R, a.max_trial, a.overlap_min, reads_rc=rc_set))
plain["wall_s"] = round(time.perf_counter() - t, 3)
t = time.perf_counter()
rows, st2, n_masked = ctx.overlap_strands_masked(S, mask, a.R, cen, max_occ, a.max_trial, a.overlap_min, reads_rc=rc_set)
masked = found(rows, st2)
masked["wall_s"] = round(time.perf_counter() - t, 3)
masked["n_masked"] = n_masked

line = {
    "library": os.environ.get("PBA_LIB_PATH", "in-tree"),
    "workload": f"census of {n} x {rl} reads @15% of a {a.genome} genome with {a.copies} copies of a {ELEMENT}-base element and a {SATELLITE}-base "
                f"period-5 satellite planted by the tool (seeded), {int(flip.sum())} reads reverse-complemented; weight-12 mask, head_tail; "
                f"R={a.R}, max_trial={a.max_trial}, overlap_min={a.overlap_min}, cutoff fraction {a.fraction}",
    "runs": f"census figures: median and best of {a.repeat} fresh censuses after one untimed; revcomp, the census call and both overlap calls: one "
            "timed run each after one untimed", "repeats": a.repeat, "reads": n,
    "census": census_line, "census_all_T_same_shape": one_key_line, "census_genome_one_contig_mode_all": contig_line,
    "census_call_ms": round(census_call_ms, 3), "revcomp_call_ms": round(revcomp_ms, 3),
    "census_over_revcomp": round(census_call_ms / revcomp_ms, 3) if revcomp_ms else None,
    "n_distinct": n_distinct, "max_count": max_count, "hist_1_to_8": [int(x) for x in hist[1:9]], "max_occ": max_occ,
    "reads_over_half_repeat": int((over * 2 > vis).sum()),
    "overlap_strands": plain, "overlap_strands_masked": masked,
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", a.out), "w") as f:
    f.write(json.dumps(line) + "\n")
print(json.dumps(line))
