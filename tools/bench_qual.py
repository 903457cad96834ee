#!/usr/bin/env python3
"""What the evidence costs evolve (pba_pileup_evolve_qual against pba_pileup_evolve) on the inputs of
tools/bench_polish.py (--workload polish: BASELINE configs[1]'s 5 Mb genome cut into 50 drafted contigs, the tiled kernels,
10 000 mapped 15 kb reads voting) or of tools/bench_correct.py (--workload correct: 20 000 reads of 15 kb at 20x, the
per-target kernels, their overlap rows voting).  Every repetition makes twin pile-ups, votes both alike and evolves one plainly
and one with evidence, in alternating order, in one process after a warm-up pair; each call is timed between two HIP events
after a device-wide synchronise.  Prints one JSON line: median / min / max of both, their ratio, the characters per box c and
the ratio of bytes moved (40 + 10 c) / (40 + c) to hold it against.  --plain: evolve alone (a build without the evidence
entry points, to time the parent commit on the same inputs).  --no-votes: fresh boxes (c = 1), no mapping or overlaps."""
import argparse, json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from pacbioassembly_amd import Context, Pileup, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--workload", choices=("polish", "correct"), default="polish")
ap.add_argument("--reads", type=int, default=0, help="0: 10 000 (polish) / 20 000 (correct)")
ap.add_argument("--read-len", type=int, default=15_000)
ap.add_argument("--genome", type=int, default=5_000_000)
ap.add_argument("--contigs", type=int, default=50)
ap.add_argument("--draft-error", type=float, default=0.02)
ap.add_argument("--coverage", type=float, default=20.0)
ap.add_argument("--weight", type=int, default=1)
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--qmax", type=int, default=60)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--no-votes", action="store_true")
ap.add_argument("--plain", action="store_true")
a = ap.parse_args()

ctx = Context(0)
mask = eng.mask_from_pattern("111*11*11*1*1111")
if a.workload == "polish":
    from map_ref import mutate
    n = a.reads or 10_000
    g = eng.synth_genome(2, a.genome)
    gb = g.tobytes()
    cuts = np.linspace(0, g.size, a.contigs + 1).astype(np.int64)
    rng = np.random.default_rng(6)
    T = ctx.seqs_from_list([mutate(rng, gb[int(cuts[c]):int(cuts[c + 1])], a.draft_error) for c in range(a.contigs)], strict_acgt=True)
    vote = lambda p: None
    if not a.no_votes:
        text, offs, _ = eng.synth_reads(3, g, n, a.read_len, 0.05, 0.05, 0.05, nthreads=16)
        S = ctx.seqs_from_text(text, offs, strict_acgt=True)
        Rd = ctx.seqs_revcomp(S, np.random.default_rng(4).integers(0, 2, n).astype(np.uint8))
        S.close()
        Rc = ctx.seqs_revcomp(Rd)
        ix = ctx.index_build_set(T, mask)
        rows, _ = ctx.map_reads(ix, T, Rd, a.R, 50, 500, reads_rc=Rc)
        ix.close()
        vote = lambda p: p.vote_mapped(Rd, rows, a.R, 64, reads_rc=Rc)
    what = f"polish: {a.contigs} contigs of a {a.genome} genome drafted at {a.draft_error}, {0 if a.no_votes else n} x {a.read_len} reads voting"
else:
    n = a.reads or 20_000
    g = eng.synth_genome(2, int(n * a.read_len / a.coverage))
    text, offs, _ = eng.synth_reads(3, g, n, a.read_len, 0.05, 0.05, 0.05, nthreads=16)
    S = ctx.seqs_from_text(text, offs, strict_acgt=True)
    T = ctx.seqs_revcomp(S, np.random.default_rng(4).integers(0, 2, n).astype(np.uint8))
    S.close()
    vote = lambda p: None
    if not a.no_votes:
        Rc = ctx.seqs_revcomp(T)
        rows, _ = ctx.overlap_strands_sharded(T, mask, a.R, 32, 64, reads_rc=Rc)
        vote = lambda p: p.vote(rows, a.R, reads_rc=Rc)
    what = f"correct: {n} x {a.read_len} reads at {a.coverage}x, {'no rows' if a.no_votes else str(len(rows)) + ' rows'} voting"


def events(fn):
    """fn() between two HIP events on the null stream, after a device-wide synchronise on both sides"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def voted():
    p = Pileup(ctx, T, weight=a.weight)
    vote(p)
    return p


def one(kind):
    """a fresh voted pile-up evolved the `kind` way: (milliseconds, characters out)"""
    p = voted()
    out, ms = events((lambda: p.evolve_qual(a.qmax)) if kind == "qual" else p.evolve)
    chars = int(out[1]["len_out"].sum())
    for x in out:
        if hasattr(x, "close"):
            x.close()
    p.close()
    return ms, chars


kinds = ("plain",) if a.plain else ("plain", "qual")
for k in kinds:
    one(k)                                                  # warm-up: the calls that are timed, whole
ms = {k: [] for k in kinds}
chars = 0
for rep in range(max(1, a.reps)):
    for k in (kinds if rep % 2 == 0 else kinds[::-1]):
        t, chars = one(k)
        ms[k].append(t)


def spread(vals):
    return {"median": round(statistics.median(vals), 3), "min": round(min(vals), 3), "max": round(max(vals), 3)}


boxes = int(T.lengths().astype(np.int64).sum())
c = chars / max(boxes, 1)
res = {"workload": what, "weight": a.weight, "reps": len(ms["plain"]), "boxes": boxes, "chars": chars, "chars_per_box": round(c, 4),
       "evolve_ms": spread(ms["plain"])}
if not a.plain:
    res["evolve_qual_ms"] = spread(ms["qual"])
    res["ratio"] = round(res["evolve_qual_ms"]["median"] / res["evolve_ms"]["median"], 3)
    res["byte_ratio"] = round((40 + 10 * c) / (40 + c), 3)
print(json.dumps(res))
