#!/usr/bin/env python3
"""overlap -> layout -> stitch -> one round of pba_polish_contigs on BASELINE configs[1]'s genome (5 Mb): --reads synthetic
15 kb reads @15 % error, a seeded random half of them reverse-complemented on the device.  Prints one JSON line: the
per-stage HIP-event times (overlap scan / sort / walk of both strands, layout classify / chain / stitch, the polish round's
stages), the layout's counters, contig count and N50, and the mean edit distance of sampled contig windows to the genome
before and after polishing.  The expectation to check: layout and stitch cost far less than the overlap call that feeds them.
A measured line belongs in profiles/layout_line.json.
--consensus (opt-in; the defaults are unchanged) adds a leg next to the polish leg: pba_layout_consensus of the same layout
and rows (stitch -> place -> vote -> evolve, one round, no index and no mapper), its stage times and counters, and the
distance of the same sampled windows as stitched, after layout_consensus and after the one polish round; the line is also
written to profiles/layout_consensus_line.json.  The expectation to record: place costs a few row-sized launches, vote costs
what polish's vote stage costs for the same number of voting reads.  Compare times against the polish leg of the same run at
the parent commit's code, never against itself."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from pacbioassembly_amd import Context, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000)
ap.add_argument("--read-len", type=int, default=15_000)
ap.add_argument("--genome", type=int, default=5_000_000)
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--max-trial", type=int, default=32)
ap.add_argument("--overlap-min", type=int, default=64)
ap.add_argument("--hang", type=int, default=64)
ap.add_argument("--min-reads", type=int, default=2)
ap.add_argument("--targets-per-call", type=int, default=10_000)
ap.add_argument("--sample", type=int, default=40, help="contig windows of --window bases whose distance to the genome is measured")
ap.add_argument("--window", type=int, default=2000)
ap.add_argument("--consensus", action="store_true", help="also run pba_layout_consensus on the layout and report it next to the polish leg")
a = ap.parse_args()
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def infix_distance(pat: bytes, text: bytes) -> int:
    """min edit distance between `pat` and any substring of `text` (Myers' bit-vector search over Python integers)."""
    m = len(pat)
    if m == 0:
        return 0
    peq = {}
    for i, c in enumerate(pat):
        peq[c] = peq.get(c, 0) | (1 << i)
    full, top = (1 << m) - 1, 1 << (m - 1)
    pv, mv, score, best = full, 0, m, m
    for c in text:
        eq = peq.get(c, 0)
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | (~(xh | pv) & full)
        mh = pv & xh
        if ph & top:
            score += 1
        elif mh & top:
            score -= 1
        ph = (ph << 1) & full                                 # (no carry in: a match may start at any text position)
        mh = (mh << 1) & full
        pv = mh | (~(xv | ph) & full)
        mv = ph & xv
        best = min(best, score)
    return best


ctx = Context(0)
mask = eng.mask_from_pattern("111*11*11*1*1111")
g = eng.synth_genome(2, a.genome)
gb = g.tobytes()
text, offs, starts = eng.synth_reads(3, g, a.reads, a.read_len, 0.05, 0.05, 0.05, nthreads=16)
S = ctx.seqs_from_text(text, offs, strict_acgt=True)
del text
flip = np.random.default_rng(4).integers(0, 2, a.reads).astype(np.uint8)
Rd = ctx.seqs_revcomp(S, flip)
S.close()
Rc = ctx.seqs_revcomp(Rd)

t0 = time.perf_counter()
rows, ost = ctx.overlap_strands_sharded(Rd, mask, a.R, a.max_trial, a.overlap_min, a.targets_per_call, reads_rc=Rc)
t_ovl = time.perf_counter()
warm = ctx.layout(Rd, rows, a.hang, a.min_reads)          # warm-up: first launches and the ctx's work buffers
warm.stitch(Rd).close()
warm.close()
t1 = time.perf_counter()
lay = ctx.layout(Rd, rows, a.hang, a.min_reads)
contigs = lay.stitch(Rd)
t2 = time.perf_counter()
st = lay.stats
info, table = lay.contigs(), lay.rows()
lens = np.sort(info["length"].astype(np.int64))[::-1]
n50 = int(lens[np.searchsorted(np.cumsum(lens), lens.sum() / 2)]) if lens.size else 0
polished, prow, plog = ctx.polish_contigs(contigs, Rd, mask, a.R, 50, 500, strands=3, rounds=1, reads_rc=Rc)
t3 = time.perf_counter()
cons = None
if a.consensus:
    ctx.layout_consensus(lay, Rd, rows, a.R, a.overlap_min, reads_rc=Rc)[0].close()      # warm-up, as for the layout
    t4 = time.perf_counter()
    cons, crow, cst = ctx.layout_consensus(lay, Rd, rows, a.R, a.overlap_min, reads_rc=Rc)
    t5 = time.perf_counter()


def windows(S):
    """mean distance of the first --window bases of sampled contigs to the genome around where the head read was drawn"""
    nc = len(info)
    if not nc:
        return None
    pick = np.random.default_rng(5).choice(nc, min(a.sample, nc), replace=False)
    out = []
    for c in pick:
        head = int(info["head_read"][c])
        forward = int(table["orient"][head]) == int(flip[head])       # the walk undoes the flip: the contig runs with the genome
        anchor = int(starts[head]) if forward else int(starts[head]) + a.read_len
        lo, hi = (anchor - a.window // 2, anchor + 3 * a.window // 2) if forward else (anchor - 3 * a.window // 2, anchor + a.window // 2)
        region = gb[max(lo, 0):max(hi, 0)]
        w = S.get_text(int(c))[:a.window]
        out.append(infix_distance(w, region if forward else region.translate(_COMP)[::-1]))
    return round(float(np.mean(out)), 2)


ovl_ms = sum(s.get(k, 0.0) for s in ost for k in ("scan_ms", "sort_ms", "walk_ms"))
line = {
    "workload": f"layout of {a.reads} x {a.read_len} reads @15% of a {a.genome} genome, {int(flip.sum())} reverse-complemented, R={a.R}, "
                f"max_trial={a.max_trial}, overlap_min={a.overlap_min}, hang={a.hang}, min_reads={a.min_reads}",
    "overlap_rows": int(len(rows)), "overlap_event_ms": round(ovl_ms, 2), "overlap_wall_s": round(t_ovl - t0, 3),
    "classify_ms": round(st["classify_ms"], 3), "chain_ms": round(st["chain_ms"], 3), "stitch_ms": round(st["stitch_ms"], 3),
    "layout_wall_s": round(t2 - t1, 3), "layout_over_overlap": round((st["classify_ms"] + st["chain_ms"] + st["stitch_ms"]) / ovl_ms, 5) if ovl_ms else None,
    "counters": {k: int(v) for k, v in st.items() if not k.endswith("_ms")},
    "contigs": int(len(info)), "n50": n50, "longest": int(lens[0]) if lens.size else 0,
    "polish": {k: round(float(plog[k].sum()), 2) for k in ("index_ms", "map_ms", "vote_ms", "evolve_ms")}, "polish_wall_s": round(t3 - t2, 3),
    "polish_rows_voted": int(plog["n_voted"].sum()),
    "truth_sample": {"windows": int(min(a.sample, len(info))), "window": a.window, "mean_distance_before": windows(contigs),
                     "mean_distance_after": windows(polished)},
}
if cons is not None:
    line["consensus"] = {k: round(float(cst[k]), 3) for k in ("stitch_ms", "place_ms", "vote_ms", "evolve_ms")}
    line["consensus_wall_s"] = round(t5 - t4, 3)
    line["consensus_counters"] = {k: int(v) for k, v in cst.items() if not k.endswith("_ms")}
    line["truth_sample"].update(mean_distance_stitched=line["truth_sample"]["mean_distance_before"],
                                mean_distance_after_consensus=windows(cons), mean_distance_after_polish=line["truth_sample"]["mean_distance_after"])
    with open(os.path.join(ROOT, "profiles", "layout_consensus_line.json"), "w") as f:
        f.write(json.dumps(line) + "\n")
print(json.dumps(line))
