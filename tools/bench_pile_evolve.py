#!/usr/bin/env python3
"""pba_pileup_create + pba_pileup_evolve of a one-sequence set of --bases bases (no votes): the one pile-up workload a
library from before the tiled kernels can run too (PBA_LIB_PATH=<its build> with --old-abi, which binds none of the entry
points added since).  --seqs N cuts the bases into N equal sequences, of at most 60 000 bases each so that the per-target
kernels serve instead of the tiled ones.  One warm-up, then --reps timed repetitions; one JSON line with the wall
milliseconds between stream fences of each."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--bases", type=int, default=5_000_000)
ap.add_argument("--seqs", type=int, default=1)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--old-abi", action="store_true")
a = ap.parse_args()
from pacbioassembly_amd import _lib
if a.old_abi:
    for name in ("pba_map_row_pair", "pba_pileup_vote_mapped", "pba_polish_contigs", "pba_polish_contigs_budget"):
        _lib.SYMBOLS.pop(name, None)
from pacbioassembly_amd import Context, Pileup, engine as eng
ctx = Context(0)
g = eng.synth_genome(2, a.bases)
per = a.bases // a.seqs
if a.seqs < 1 or per * a.seqs != a.bases or (a.seqs > 1 and per > 60_000):
    sys.exit("--seqs must cut --bases into equal sequences of at most 60 000 bases")
S = ctx.seqs_from_text(g, np.arange(a.seqs + 1, dtype=np.uint64) * np.uint64(per), strict_acgt=True)
ms = []
for rep in range(a.reps + 1):
    ctx.sync()
    t = time.perf_counter()
    out, rows = Pileup(ctx, S).evolve()
    ctx.sync()
    ms.append((time.perf_counter() - t) * 1e3)
    assert int(rows["len_out"].sum()) == a.bases
    out.close()
print(json.dumps({"workload": f"pileup create + evolve, {a.seqs} sequence(s) of {per} bases, no votes", "library": os.environ.get("PBA_LIB_PATH", "in-tree"),
                  "warmup_ms": round(ms[0], 2), "ms": [round(x, 2) for x in ms[1:]]}))
