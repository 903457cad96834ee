#!/usr/bin/env python3
"""pba_map_reads on BASELINE configs[1]'s workload (5 Mb genome, n synthetic 15 kb reads @15 % error, R = 0.30, 50 trials)
with a seeded random half of the reads reverse-complemented on the device.  One JSON line with three comparisons, each a
step = index build + locate, wall time between stream fences, the fastest and all of --steps timed steps after --warmup:
  a  one contig, one strand: map_reads(strands = 1) through a one-sequence set index against pba_locate -- what the contig
     resolution costs;
  b  both strands: map_reads(strands = 3) against two full pba_locate passes (the reads, then their reverse complement);
  c  the same genome cut into --contigs equal contigs, strands = 3.
--locate-only times just the pba_locate steps and binds none of the new entry points: for a library built from an earlier
commit, named by PBA_LIB_PATH, on the same reads."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=100_000)
ap.add_argument("--read-len", type=int, default=15_000)
ap.add_argument("--genome", type=int, default=5_000_000)
ap.add_argument("--contigs", type=int, default=1000)
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--trials", type=int, default=50)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--locate-only", action="store_true")
a = ap.parse_args()

from pacbioassembly_amd import _lib
NEW = ("pba_index_build_set", "pba_index_seqs", "pba_map_reads")
if a.locate_only:
    for name in NEW:
        _lib.SYMBOLS.pop(name, None)
from pacbioassembly_amd import Context, engine as eng

ctx = Context(0)
mask = eng.mask_from_pattern("111*11*11*1*1111")
g = eng.synth_genome(2, a.genome)
text, offs, _ = eng.synth_reads(3, g, a.reads, a.read_len, 0.05, 0.05, 0.05, nthreads=16)
S = ctx.seqs_from_text(text, offs, strict_acgt=True)
del text
flip = np.random.default_rng(4).integers(0, 2, a.reads).astype(np.uint8)
Rd = ctx.seqs_revcomp(S, flip)                                   # the mixed-strand set
S.close()
t = time.perf_counter()
Rc = ctx.seqs_revcomp(Rd)
revcomp_ms = (time.perf_counter() - t) * 1e3
T1 = ctx.seqs_from_text(g, np.array([0, g.size], np.uint64), strict_acgt=True)


def timed(step):
    """step() -> dict of counts; returns {"ms": fastest, "all_ms": [...], "kernel_ms": of the fastest, **counts}."""
    for _ in range(a.warmup):
        step()
    ctx.sync()
    out, walls = None, []
    for _ in range(max(1, a.steps)):
        ctx.sync()
        t = time.perf_counter()
        info = step()
        ctx.sync()
        walls.append((time.perf_counter() - t) * 1e3)
        if walls[-1] == min(walls):
            out = info
    return dict(ms=round(min(walls), 2), all_ms=[round(x, 2) for x in walls], **out)


def locate_step(sets):
    def step():
        ix = ctx.index_build(T1, 0, mask)
        located = pairs = 0
        kms = 0.0
        for X in sets:
            rows, st = ctx.locate(ix, T1, 0, X, a.R, a.trials, 500)
            pr = ctx.last_profile()
            kms += pr["align_ms"] + pr["align_redo_ms"]
            located += st["n_located"]; pairs += st["n_pairs"]
        ix.close()
        return dict(kernel_ms=round(kms, 2), n_located=int(located), n_pairs=int(pairs))
    return step


def map_step(T, strands):
    def step():
        ix = ctx.index_build_set(T, mask)
        ix_ms = ctx.last_profile()["index_ms"]
        rows, st = ctx.map_reads(ix, T, Rd, a.R, a.trials, 500, strands=strands, reads_rc=Rc)
        pr = ctx.last_profile()
        ix.close()
        return dict(kernel_ms=round(pr["align_ms"] + pr["align_redo_ms"], 2), index_levels_ms=round(ix_ms, 3),
                    n_located=int(rows["found"].sum()), n_minus=int((rows["strand"] == -1).sum()),
                    n_pairs=int(st["strand"][0]["n_pairs"] + st["strand"][1]["n_pairs"]), n_second_walk=st["n_second_walk"],
                    n_redo=int(pr["n_redo"]))
    return step


res = {"workload": f"{a.reads} x {a.read_len} reads @15% on a {a.genome} genome, {int(flip.sum())} reads reverse-complemented, "
                   f"R={a.R}, {a.trials} trials, step = index build + locate",
       "steps": a.steps, "warmup": a.warmup, "library": "PBA_LIB_PATH" if os.environ.get("PBA_LIB_PATH") else "in-tree",
       "revcomp_all_reads_ms": round(revcomp_ms, 2),
       "locate_one_pass": timed(locate_step([Rd])),
       "locate_two_passes": timed(locate_step([Rd, Rc]))}
if not a.locate_only:
    res["a_one_contig_one_strand"] = timed(map_step(T1, 1))
    res["a_over_locate"] = round(res["a_one_contig_one_strand"]["ms"] / res["locate_one_pass"]["ms"], 4)
    res["b_both_strands"] = timed(map_step(T1, 3))
    res["b_over_two_passes"] = round(res["b_both_strands"]["ms"] / res["locate_two_passes"]["ms"], 4)
    cuts = np.linspace(0, g.size, a.contigs + 1).astype(np.uint64)
    Tc = ctx.seqs_from_text(g, cuts, strict_acgt=True)
    res["c_contigs"] = dict(n=a.contigs, **timed(map_step(Tc, 3)))
    res["c_over_b"] = round(res["c_contigs"]["ms"] / res["b_both_strands"]["ms"], 4)
print(json.dumps(res))
