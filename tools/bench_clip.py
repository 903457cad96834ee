#!/usr/bin/env python3
"""overlap -> clip -> apply -> overlap -> layout on BASELINE configs[1]'s genome (5 Mb): --reads synthetic 15 kb reads @15 %
error with planted defects -- a share --chimeras of them replaced by a join of two pieces from places at least two read
lengths apart (pieces the set does not hold; the second reverse-complemented by a seeded draw), a share --junk of them with a
random tail of a fifth of the read length -- and a seeded random half reverse-complemented.  Prints one JSON line and writes
it to profiles/clip_line.json: the per-stage HIP-event times (overlap scan / sort / walk of both strands; clip events / sweep
/ gather), the clip counters, how many planted reads were flagged (n_runs >= 2), cut within `margin` of the junction, or left
spanning it, and the layout's contig count with and without clipping.
There is no parent to compare with and no time threshold.  The expectation to check is only that events + sweep + gather cost
far less than the overlap call that feeds them.  The line is ONE run (one untimed clip + apply before the timed one, no
repeats): it says so in "runs"."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from pacbioassembly_amd import Context, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=3000)
ap.add_argument("--read-len", type=int, default=15_000)
ap.add_argument("--genome", type=int, default=5_000_000)
ap.add_argument("--chimeras", type=float, default=0.05, help="share of the reads replaced by a chimera")
ap.add_argument("--junk", type=float, default=0.05, help="share of the reads given a random tail")
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--max-trial", type=int, default=32)
ap.add_argument("--overlap-min", type=int, default=64)
ap.add_argument("--margin", type=int, default=100)
ap.add_argument("--min-cov", type=int, default=2)
ap.add_argument("--min-len", type=int, default=1000)
ap.add_argument("--hang", type=int, default=64)
ap.add_argument("--min-reads", type=int, default=2)
ap.add_argument("--targets-per-call", type=int, default=10_000)
a = ap.parse_args()
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def rc(x):
    return x.translate(_COMP)[::-1]


n, rl = a.reads, a.read_len
n_chim, n_junk = int(round(a.chimeras * n)), int(round(a.junk * n))
g = eng.synth_genome(2, a.genome)
text, offs, starts = eng.synth_reads(3, g, n + 2 * n_chim, rl, 0.05, 0.05, 0.05, nthreads=16)      # reads n ..: the pool of pieces
src = lambda i: text[int(offs[i]):int(offs[i + 1])].tobytes()
rng = np.random.default_rng(6)
planted = rng.permutation(n)[:n_chim + n_junk]
texts, chim, junk = [src(i) for i in range(n)], {}, {}
pool = list(range(n, n + 2 * n_chim))
for i in planted[:n_chim]:
    x = pool.pop(int(rng.integers(0, len(pool))))
    far = [k for k in pool if abs(int(starts[k]) - int(starts[x])) >= 2 * rl]
    y = far[int(rng.integers(0, len(far)))]
    pool.remove(y)
    J = int(rng.integers(rl // 3, 2 * rl // 3 + 1))
    tail = src(y)[:rl - J]
    texts[int(i)] = src(x)[:J] + (rc(tail) if rng.integers(0, 2) else tail)
    chim[int(i)] = J
for i in planted[n_chim:]:
    texts[int(i)] += rng.choice(ACGT, rl // 5).tobytes()
    junk[int(i)] = (rl, rl + rl // 5)
flip = rng.integers(0, 2, n).astype(bool)
for i in np.flatnonzero(flip):
    i, L = int(i), len(texts[int(i)])
    texts[i] = rc(texts[i])
    if i in chim:
        chim[i] = L - chim[i]
    if i in junk:
        junk[i] = (L - junk[i][1], L - junk[i][0])
del text

ctx = Context(0)
mask = eng.mask_from_pattern("111*11*11*1*1111")
S = ctx.seqs_from_list(texts, strict_acgt=True)


def overlap(X):
    t = time.perf_counter()
    rows, ost = ctx.overlap_strands_sharded(X, mask, a.R, a.max_trial, a.overlap_min, a.targets_per_call)
    return rows, sum(s.get(k, 0.0) for s in ost for k in ("scan_ms", "sort_ms", "walk_ms")), time.perf_counter() - t


rows, ovl_ms, ovl_wall = overlap(S)
warm = ctx.clip(S, rows, a.margin, a.min_cov, a.min_len)      # warm-up: first launches and the ctx's work buffers
warm.apply(S).close()
warm.close()
t1 = time.perf_counter()
cl = ctx.clip(S, rows, a.margin, a.min_cov, a.min_len)
clipped = cl.apply(S)
t2 = time.perf_counter()
st, table = cl.stats, cl.rows()
rows2, ovl2_ms, ovl2_wall = overlap(clipped)
lay0 = ctx.layout(S, rows, a.hang, a.min_reads)
lay1 = ctx.layout(clipped, rows2, a.hang, a.min_reads)


def lay_line(lay):
    info = lay.contigs()
    lens = np.sort(info["length"].astype(np.int64))[::-1]
    return {"contigs": int(len(info)), "longest": int(lens[0]) if lens.size else 0,
            "n50": int(lens[np.searchsorted(np.cumsum(lens), lens.sum() / 2)]) if lens.size else 0,
            "placed": int(lay.stats["n_placed"]), "contained": int(lay.stats["n_contained"])}


m = a.margin
spans = lambda r, lo, hi: bool(r["state"] != 0 and r["beg"] <= lo and r["end"] >= hi)
near = lambda r, J: bool(r["state"] == 2 and (abs(int(r["beg"]) - J) <= m or abs(int(r["end"]) - J) <= m))
clip_ms = st["events_ms"] + st["sweep_ms"] + st["gather_ms"]
line = {
    "workload": f"clip of {n} x {rl} reads @15% of a {a.genome} genome, {len(chim)} chimeras, {len(junk)} junk tails of {rl // 5}, "
                f"{int(flip.sum())} reverse-complemented, R={a.R}, max_trial={a.max_trial}, overlap_min={a.overlap_min}, margin={m}, "
                f"min_cov={a.min_cov}, min_len={a.min_len}, roles=3",
    "runs": "single unrepeated run: one untimed clip + apply, then the timed one", "reads": n, "repeats": 1,
    "overlap_rows": int(len(rows)), "overlap_event_ms": round(ovl_ms, 2), "overlap_wall_s": round(ovl_wall, 3),
    "events_ms": round(st["events_ms"], 3), "sweep_ms": round(st["sweep_ms"], 3), "gather_ms": round(st["gather_ms"], 3),
    "clip_wall_s": round(t2 - t1, 4), "clip_over_overlap": round(clip_ms / ovl_ms, 5) if ovl_ms else None,
    "counters": {k: int(v) for k, v in st.items() if not k.endswith("_ms")},
    "chimeras": {"planted": len(chim), "whole": sum(int(table[i]["state"]) == 1 for i in chim),
                 "flagged_multi_run": sum(int(table[i]["n_runs"]) >= 2 for i in chim), "cut_within_margin": sum(near(table[i], J) for i, J in chim.items()),
                 "flagged_or_cut_near": sum(int(table[i]["n_runs"]) >= 2 or near(table[i], J) for i, J in chim.items()),
                 "span_junction": sum(spans(table[i], J - m, J + m) for i, J in chim.items()),
                 "dropped": sum(int(table[i]["state"]) == 0 for i in chim)},
    "junk": {"planted": len(junk), "whole": sum(int(table[i]["state"]) == 1 for i in junk),
             "junk_bases_kept": sum(max(0, min(int(table[i]["end"]), hi) - max(int(table[i]["beg"]), lo)) for i, (lo, hi) in junk.items()),
             "junk_bases": sum(hi - lo for lo, hi in junk.values())},
    "clean": {"reads": n - len(chim) - len(junk), "whole": sum(int(r["state"]) == 1 for r in table if int(r["read"]) not in chim and int(r["read"]) not in junk)},
    "overlap_after_rows": int(len(rows2)), "overlap_after_event_ms": round(ovl2_ms, 2),
    "layout_without_clip": lay_line(lay0), "layout_with_clip": lay_line(lay1),
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "clip_line.json"), "w") as f:
    f.write(json.dumps(line) + "\n")
print(json.dumps(line))
