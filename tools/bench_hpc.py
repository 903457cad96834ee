#!/usr/bin/env python3
"""Homopolymer compression on synthetic reads: --reads reads of --len bases @15 % error of a --genome genome,
a seeded random half reverse-complemented.  Prints one JSON line and writes it to profiles/hpc_line.json:
  * the compress stages (heads / emit / pack, HIP events) and the bases in and out; the lift of the rows (HIP events around
    the call: upload, kernel, download);
  * in the same run, pba_seqs_revcomp on the same set (HIP events around the call) as the yardstick -- another
    read-a-set, write-a-set pass -- and compress / revcomp as a ratio.  No gate;
  * the rows overlap_strands finds on the set as given next to overlap_hpc, once on the stock synthetic set and once on the
    same set after the run lengths of every read are drawn again (homopolymer noise planted HERE, seeded: every run of two
    bases or more grows or shrinks by one base with probability --noise, never to zero; single bases stay).
pba_synth_reads spreads its errors uniformly, so the first pair of row counts says little about real data, and the second is
noise of this tool's own making.  The line is ONE run (one untimed compress + lift before the timed one, no repeats): it says
so in "runs"."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from pacbioassembly_amd import Context, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=3000)
ap.add_argument("--len", type=int, default=15_000, dest="read_len")
ap.add_argument("--genome", type=int, default=5_000_000)
ap.add_argument("--noise", type=float, default=0.2, help="share of the runs of two bases or more whose length changes by one")
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--max-trial", type=int, default=32)
ap.add_argument("--overlap-min", type=int, default=64)
ap.add_argument("--targets-per-call", type=int, default=10_000)
a = ap.parse_args()
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def redraw(rng, text, noise):
    x = np.frombuffer(text, np.uint8)
    heads = np.flatnonzero(np.concatenate(([True], x[1:] != x[:-1])))
    runs = np.diff(np.concatenate((heads, [x.size])))
    again = (runs >= 2) & (rng.random(runs.size) < noise)
    runs = np.where(again, runs + rng.choice((-1, 1), runs.size), runs)
    return np.repeat(x[heads], runs).tobytes()


n, rl = a.reads, a.read_len
g = eng.synth_genome(2, a.genome)
text, offs, _ = eng.synth_reads(3, g, n, rl, 0.05, 0.05, 0.05, nthreads=16)
rng = np.random.default_rng(7)
flip = rng.integers(0, 2, n).astype(bool)
stock = [text[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
stock = [t.translate(_COMP)[::-1] if f else t for t, f in zip(stock, flip)]
noisy = [redraw(rng, t, a.noise) for t in stock]
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


def overlaps(S):
    t = time.perf_counter()
    rows, st2 = ctx.overlap_strands_sharded(S, mask, a.R, a.max_trial, a.overlap_min, a.targets_per_call)
    plain = {"rows": int(len(rows)), "event_ms": round(sum(s.get(k, 0.0) for s in st2 for k in ("scan_ms", "sort_ms", "walk_ms")), 2),
             "wall_s": round(time.perf_counter() - t, 3)}
    t = time.perf_counter()
    lifted, st2, hpc = ctx.overlap_hpc(S, mask, a.R, a.max_trial, a.overlap_min, targets_per_call=a.targets_per_call)
    comp = {"rows": int(len(lifted)), "event_ms": round(sum(s.get(k, 0.0) for s in st2 for k in ("scan_ms", "sort_ms", "walk_ms")), 2),
            "wall_s": round(time.perf_counter() - t, 3)}
    pairs = lambda r: {(int(x["target"]), int(x["query"])) for x in r}
    both = pairs(rows) & pairs(lifted)
    hpc.close()
    return {"overlap_strands": plain, "overlap_hpc": comp, "pairs_in_both": len(both), "pairs_plain_only": len(pairs(rows) - both),
            "pairs_hpc_only": len(pairs(lifted) - both)}, lifted


S = ctx.seqs_from_list(stock, strict_acgt=True)
found_stock, lifted = overlaps(S)
warm_set, warm = ctx.seqs_hpc(S)                               # warm-up: first launches and the ctx's work buffers
crows, _ = ctx.overlap_strands_sharded(warm_set, mask, a.R, a.max_trial, a.overlap_min, a.targets_per_call)
warm.lift_overlaps(crows)
ctx.seqs_revcomp(S).close()
warm_set.close()
warm.close()

t0 = time.perf_counter()
comp, hpc = ctx.seqs_hpc(S)
t1 = time.perf_counter()
st = hpc.stats
_, lift_ms = events(lambda: hpc.lift_overlaps(crows))
rc_set, revcomp_ms = events(lambda: ctx.seqs_revcomp(S))
_, hpc_call_ms = events(lambda: ctx.seqs_hpc(S))
rc_set.close()
comp.close()
hpc.close()
S.close()

S2 = ctx.seqs_from_list(noisy, strict_acgt=True)
found_noisy, _ = overlaps(S2)

kernels_ms = st["heads_ms"] + st["emit_ms"] + st["pack_ms"]
line = {
    "workload": f"hpc of {n} x {rl} reads @15% of a {a.genome} genome, {int(flip.sum())} reverse-complemented; R={a.R}, max_trial={a.max_trial}, "
                f"overlap_min={a.overlap_min}; noisy set: every run of >= 2 bases one base longer or shorter with probability {a.noise} (seeded)",
    "runs": "single unrepeated run: one untimed compress + lift + revcomp, then the timed ones", "reads": n, "repeats": 1,
    "n_bases_in": int(st["n_bases_in"]), "n_bases_out": int(st["n_bases_out"]), "max_len_out": int(st["max_len_out"]), "n_chunks": int(st["n_chunks"]),
    "heads_ms": round(st["heads_ms"], 3), "emit_ms": round(st["emit_ms"], 3), "pack_ms": round(st["pack_ms"], 3),
    "compress_stages_ms": round(kernels_ms, 3), "compress_call_ms": round(hpc_call_ms, 3), "compress_wall_s": round(t1 - t0, 4),
    "lift_rows": int(len(crows)), "lift_call_ms": round(lift_ms, 3),
    "revcomp_call_ms": round(revcomp_ms, 3), "compress_over_revcomp": round(hpc_call_ms / revcomp_ms, 3) if revcomp_ms else None,
    "found_on_stock_set": found_stock, "found_on_noisy_set": found_noisy,
}
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "hpc_line.json"), "w") as f:
    f.write(json.dumps(line) + "\n")
print(json.dumps(line))
