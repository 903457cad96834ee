#!/usr/bin/env python3
"""pba_polish_contigs on BASELINE configs[1]'s genome (5 Mb) cut into --contigs equal contigs: the contigs are drafted with
seeded substitutions and indels at --draft-error, n synthetic 15 kb reads @15 % error (a seeded random half of them
reverse-complemented on the device) are mapped on the draft, vote and evolve, --rounds times.  One warm-up call, then --reps
timed calls.  Prints one JSON line: the per-stage HIP-event medians of the round log, rows voted per second, the mean edit
distance of sampled contig windows to the true genome before and after, and -- on a small sample of its own -- whether the
result equals the loop composed from the CPU oracle's pieces (tests/polish_helpers.py)."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from pacbioassembly_amd import Context, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000)
ap.add_argument("--read-len", type=int, default=15_000)
ap.add_argument("--genome", type=int, default=5_000_000)
ap.add_argument("--contigs", type=int, default=50)
ap.add_argument("--draft-error", type=float, default=0.02)
ap.add_argument("--rounds", type=int, default=1)
ap.add_argument("--weight", type=int, default=1)
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--trials", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--sample", type=int, default=40, help="contig windows of --window bases whose distance to the genome is measured")
ap.add_argument("--window", type=int, default=2000)
a = ap.parse_args()
from map_ref import mutate                                  # (the seeded substitution / insertion / deletion of the tests)
from polish_helpers import oracle_polish_round, polish_case


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
mask = eng.mask_from_pattern("111*11*11*1*1111")
g = eng.synth_genome(2, a.genome)
gb = g.tobytes()
cuts = np.linspace(0, g.size, a.contigs + 1).astype(np.int64)
rng = np.random.default_rng(6)
draft = [mutate(rng, gb[int(cuts[c]):int(cuts[c + 1])], a.draft_error) for c in range(a.contigs)]
T = ctx.seqs_from_list(draft, strict_acgt=True)
text, offs, _ = eng.synth_reads(3, g, a.reads, a.read_len, 0.05, 0.05, 0.05, nthreads=16)
S = ctx.seqs_from_text(text, offs, strict_acgt=True)
del text
flip = np.random.default_rng(4).integers(0, 2, a.reads).astype(np.uint8)
Rd = ctx.seqs_revcomp(S, flip)
S.close()
Rc = ctx.seqs_revcomp(Rd)


def call():
    return ctx.polish_contigs(T, Rd, mask, a.R, a.trials, 500, strands=3, weight=a.weight, rounds=a.rounds, reads_rc=Rc)


call()[0].close()                                           # warm-up: the call that is timed, whole
logs, wall, out = [], [], None
for _ in range(max(1, a.reps)):
    if out is not None:
        out.close()
    t = time.perf_counter()
    out, rows, log = call()
    wall.append(time.perf_counter() - t)
    logs.append(log)


def spread(vals, nd=2):
    return {"median": round(statistics.median(vals), nd), "min": round(min(vals), nd), "max": round(max(vals), nd)}


def windows(texts):
    """mean distance of sampled windows (the first --window bases of a contig) to the genome from the contig's cut"""
    pick = np.random.default_rng(5).choice(a.contigs, min(a.sample, a.contigs), replace=False)
    return float(np.mean([prefix_distance(texts[c][:a.window], gb[int(cuts[c]):int(cuts[c]) + a.window + a.window // 4]) for c in pick]))


stage = {k: spread([float(l[k].sum()) for l in logs]) for k in ("index_ms", "map_ms", "vote_ms", "evolve_ms")}
voted = int(logs[-1]["n_voted"].sum())
polished = [out.get_text(c) for c in range(a.contigs)]
# identity with the oracle on a small input of its own (the one tests/test_gpu_polish.py uses), one round
from oraclelib import Oracle
contigs, reads = polish_case(701)
Ts, Rs = ctx.seqs_from_list(contigs, strict_acgt=True), ctx.seqs_from_list(reads, strict_acgt=True)
ix = ctx.index_build_set(Ts, mask)
mrows, _ = ctx.map_reads(ix, Ts, Rs, a.R)
want, _ = oracle_polish_round(Oracle(), contigs, reads, mrows)
small, _, _ = ctx.polish_contigs(Ts, Rs, mask, a.R)
print(json.dumps({
    "workload": f"polish {a.contigs} contigs of a {a.genome} genome drafted at {a.draft_error} error from {a.reads} x {a.read_len} reads "
                f"@15%, {int(flip.sum())} reverse-complemented, strands=3, weight={a.weight}, R={a.R}, {a.trials} trials, {a.rounds} round(s)",
    "reps": len(logs), **stage, "wall_s": spread(wall, 3),
    "rows_mapped": int(logs[-1]["n_mapped"].sum()), "rows_voted": voted,
    "rows_voted_per_s": round(voted / (stage["vote_ms"]["median"] * 1e-3), 1) if stage["vote_ms"]["median"] > 0 else None,
    "chunks": int(logs[-1]["n_chunks"].sum()), "bases_in": int(logs[-1]["n_bases_in"][0]), "bases_out": int(logs[-1]["n_bases_out"][-1]),
    "truth_sample": {"windows": min(a.sample, a.contigs), "window": a.window, "mean_distance_before": round(windows(draft), 2),
                     "mean_distance_after": round(windows(polished), 2)},
    "oracle_sample": {"contigs": len(contigs), "reads": len(reads), "identical": [small.get_text(c) for c in range(len(contigs))] == want},
}))
