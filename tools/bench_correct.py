#!/usr/bin/env python3
"""Read correction from overlap pile-ups (pba_correct_reads) on one GPU: n synthetic reads @15 % error at the requested
coverage (the generator bench.py uses), a seeded random half of them reverse-complemented on the device as
tools/bench_overlap_strands.py does, every read corrected from its overlaps on the strands asked for.  One warm-up call of
the same shape, then --reps timed calls over all targets.  Prints one JSON line: overlap / vote / evolve milliseconds (HIP
events on the engine's stream; median, min and max over the timed calls), rows voted per second, bases corrected per
second, and -- on a sample of targets -- the edit distance of the read and of the corrected read to the genome it was drawn
from (host bit-vector edit distance, free end on the genome side), before and after."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pacbioassembly_amd import Context, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=20000)
ap.add_argument("--read-len", type=int, default=15000)
ap.add_argument("--coverage", type=float, default=20.0)
ap.add_argument("--strands", type=int, default=3)
ap.add_argument("--weight", type=int, default=1)
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--trials", type=int, default=32)
ap.add_argument("--reps", type=int, default=3, help="timed calls after the warm-up")
ap.add_argument("--sample", type=int, default=200, help="targets whose distance to the genome is measured")
a = ap.parse_args()
n, rl = a.reads, a.read_len
L = int(n * rl / a.coverage)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def prefix_distance(read: bytes, genome: bytes) -> int:
    """min over j of the edit distance between `read` and genome[:j] (Myers / Hyyro bit-vector over Python integers)."""
    m = len(read)
    if m == 0:
        return 0
    peq = {}
    for i, c in enumerate(read):
        peq[c] = peq.get(c, 0) | (1 << i)
    full, top = (1 << m) - 1, 1 << (m - 1)
    pv, mv, score = full, 0, m
    best = m
    for c in genome:
        eq = peq.get(c, 0)
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | (~(xh | pv) & full)
        mh = pv & xh
        if ph & top:
            score += 1
        elif mh & top:
            score -= 1
        ph = ((ph << 1) | 1) & full
        mh = (mh << 1) & full
        pv = mh | (~(xv | ph) & full)
        mv = ph & xv
        if score < best:
            best = score
    return best


ctx = Context(0)
g = eng.synth_genome(2, L)
reads, offs, starts = eng.synth_reads(3, g, n, rl, nthreads=16)
S = ctx.seqs_from_text(reads, offs, strict_acgt=True)
del reads
flip = np.random.default_rng(4).integers(0, 2, n).astype(np.uint8)
M = ctx.seqs_revcomp(S, flip)                              # the mixed-strand set
S.close()
Mrc = ctx.seqs_revcomp(M)
mask = eng.mask_from_pattern("111*11*11*1*1111")
# warm-up: the call that is timed, whole (code objects loaded, the engine's work buffers grown to this shape)
ctx.correct_reads(M, mask, a.R, a.trials, 64, strands=a.strands, weight=a.weight, reads_rc=Mrc)[0].close()

runs, wall = [], []
corrected = rows = None
for _ in range(max(1, a.reps)):
    if corrected is not None:
        corrected.close()
    t = time.perf_counter()
    corrected, rows, st = ctx.correct_reads(M, mask, a.R, a.trials, 64, strands=a.strands, weight=a.weight, reads_rc=Mrc)
    wall.append(time.perf_counter() - t)
    runs.append(ctx.last_correct_profile())


def spread(vals, nd=1):
    return {"median": round(statistics.median(vals), nd), "min": round(min(vals), nd), "max": round(max(vals), nd)}


pr = runs[-1]
vote_ms = statistics.median(r["vote_ms"] for r in runs)
wall_s = statistics.median(wall)
# distance to the truth on a sample: the read (turned back to the genome's strand) against the genome from its start
pick = np.sort(np.random.default_rng(5).choice(n, min(a.sample, n), replace=False))
d_before, d_after = [], []
gb = g.tobytes()
for t_id in pick:
    seg = gb[int(starts[t_id]):int(starts[t_id]) + rl + rl // 4]
    before, after = M.get_text(int(t_id)), corrected.get_text(int(t_id))
    if flip[t_id]:
        before, after = before.translate(_COMP)[::-1], after.translate(_COMP)[::-1]
    d_before.append(prefix_distance(before, seg))
    d_after.append(prefix_distance(after, seg))
changed = int((rows["len_in"] != rows["len_out"]).sum())
print(json.dumps({
    "workload": f"read correction, {n} x {rl} reads @15%, genome {L} ({a.coverage}x), {int(flip.sum())} reads reverse-complemented, "
                f"strands={a.strands}, weight={a.weight}, R={a.R}, {a.trials} trials/end",
    "reps": len(runs),
    "overlap_ms": spread([r["overlap_ms"] for r in runs]),
    "vote_ms": spread([r["vote_ms"] for r in runs]),
    "evolve_ms": spread([r["evolve_ms"] for r in runs]),
    "wall_s": spread(wall, 3),
    "chunks": int(pr["n_chunks"]),
    "rows_voted": int(pr["n_rows"]),
    "rows_voted_per_s": round(pr["n_rows"] / (vote_ms * 1e-3), 1) if vote_ms > 0 else None,
    "bases_in": int(pr["n_bases_in"]), "bases_out": int(pr["n_bases_out"]),
    "bases_corrected_per_s": round(pr["n_bases_in"] / wall_s, 1) if wall_s > 0 else None,
    "targets_without_rows": int((rows["n_rows"] == 0).sum()),
    "targets_with_new_length": changed,
    "overlaps": {"plus": int(st[0]["n_overlaps"]), "minus": int(st[1]["n_overlaps"])},
    "truth_sample": {"targets": int(pick.size), "mean_distance_before": round(float(np.mean(d_before)), 2),
                     "mean_distance_after": round(float(np.mean(d_after)), 2),
                     "mean_error_rate_before": round(float(np.mean(d_before)) / rl, 4),
                     "mean_error_rate_after": round(float(np.mean(d_after)) / rl, 4),
                     "targets_closer": int(sum(x > y for x, y in zip(d_before, d_after))),
                     "targets_farther": int(sum(x < y for x, y in zip(d_before, d_after)))},
}))
