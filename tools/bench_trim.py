#!/usr/bin/env python3
"""Per-window counts and trimmed rows against run-length alignments, on one set of overlap rows and one GPU: n synthetic
reads at the requested error and coverage, a seeded random half of them reverse-complemented on the device as
tools/bench_correct.py does, their overlap rows on both strands found once (untimed), then pba_overlap_rows_windows,
pba_overlap_rows_trim and pba_overlap_rows_cigar timed on those rows: one untimed warm-up call of each, then --reps rounds
that run the three one after the other, so that whatever else the host is doing falls on all of them alike.

A time is the host clock around one call (every call ends synchronised): the traced passes, the copies, the host's layout of
the rows.  The windows call fetches every window into the caller's array; the CIGAR call is made with cap = 0 (its offsets and
counts complete, no run copied to the caller: at 15 kb a full fetch is gigabytes), so it is timed at its cheapest.  The trim
call also reports, from HIP events on the engine's stream, what its traced passes and its trim kernels took.  Prints one JSON
line: median, min and max over the rounds."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pacbioassembly_amd import Context, engine as eng

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=100000)
ap.add_argument("--read-len", type=int, default=15000)
ap.add_argument("--coverage", type=float, default=20.0)
ap.add_argument("--error", type=float, default=0.15, help="total error rate of the generator, a third each I / D / X")
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--trials", type=int, default=32)
ap.add_argument("--W", type=int, default=100)
ap.add_argument("--max-err", type=float, default=0.25)
ap.add_argument("--min-span", type=int, default=64)
ap.add_argument("--reps", type=int, default=3, help="timed rounds after the warm-up")
a = ap.parse_args()
n, rl = a.reads, a.read_len
L = int(n * rl / a.coverage)

ctx = Context(0)
g = eng.synth_genome(2, L)
reads, offs, _ = eng.synth_reads(3, g, n, rl, a.error / 3, a.error / 3, a.error / 3, nthreads=16)
S = ctx.seqs_from_text(reads, offs, strict_acgt=True)
del reads
flip = np.random.default_rng(4).integers(0, 2, n).astype(np.uint8)
M = ctx.seqs_revcomp(S, flip)                              # the mixed-strand set
S.close()
Mrc = ctx.seqs_revcomp(M)
mask = eng.mask_from_pattern("111*11*11*1*1111")
rows, _ = ctx.overlap_strands_sharded(M, mask, a.R, a.trials, 64, strands=3, reads_rc=Mrc)
rows = np.ascontiguousarray(rows, eng.STRAND_OVERLAP_DTYPE)
nr = rows.size
off = np.zeros(nr + 1, np.uint64)
total = C.c_uint64()
ptr = lambda x: x.ctypes.data_as(C.c_void_p)


def windows(win, cap):
    ctx.check(ctx.lib.pba_overlap_rows_windows(ctx.h, M.h, Mrc.h, ptr(rows), nr, a.R, a.W, win, cap, ptr(off), C.byref(total), None, None),
              "overlap_rows_windows")
    return int(total.value)


def cigar():
    ctx.check(ctx.lib.pba_overlap_rows_cigar(ctx.h, M.h, Mrc.h, ptr(rows), nr, a.R, None, 0, ptr(off), C.byref(total), None, None),
              "overlap_rows_cigar")
    return int(total.value)


trims = np.zeros(max(nr, 1), eng.TRIM_ROW_DTYPE)
tstats = eng._lib.PbaTrimStats()


def trim():
    ctx.check(ctx.lib.pba_overlap_rows_trim(ctx.h, M.h, Mrc.h, ptr(rows), nr, a.R, a.W, a.max_err, a.min_span, ptr(trims), C.byref(tstats)),
              "overlap_rows_trim")
    return {k: getattr(tstats, k) for k, _ in eng._lib.PbaTrimStats._fields_}


# warm-up, untimed: code objects loaded, the traced pass's scratch grown to this shape, the totals learnt
n_windows = windows(None, 0)
win = np.zeros(max(n_windows, 1), eng.ALN_COUNTS_DTYPE)
windows(ptr(win), n_windows)
n_runs = cigar()
st = trim()

t_win, t_trim, t_cig, ev_win, ev_trim = [], [], [], [], []
for _ in range(max(1, a.reps)):
    t = time.perf_counter(); windows(ptr(win), n_windows); t_win.append(time.perf_counter() - t)
    t = time.perf_counter(); st = trim(); t_trim.append(time.perf_counter() - t)
    ev_win.append(st["windows_ms"]); ev_trim.append(st["trim_ms"])
    t = time.perf_counter(); cigar(); t_cig.append(time.perf_counter() - t)


def spread(vals, scale=1e3, nd=1):
    v = [x * scale for x in vals]
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


print(json.dumps({
    "workload": f"{nr} overlap rows of {n} x {rl} reads @{a.error:.0%}, genome {L} ({a.coverage}x), {int(flip.sum())} reads "
                f"reverse-complemented, both strands, R={a.R}, {a.trials} trials/end; W={a.W}, max_err={a.max_err}, min_span={a.min_span}",
    "reps": len(t_win),
    "rows": int(nr), "windows": n_windows, "runs": n_runs,
    "overlap_rows_windows_ms": spread(t_win),
    "overlap_rows_cigar_ms_cap0": spread(t_cig),
    "overlap_rows_trim_ms": spread(t_trim),
    "trim_traced_passes_ms_events": spread(ev_win, 1.0),
    "trim_kernel_ms_events": spread(ev_trim, 1.0, 3),
    "trim_kernel_share": round(statistics.median(ev_trim) / (statistics.median(t_trim) * 1e3), 5),
    "windows_over_cigar": round(statistics.median(t_win) / statistics.median(t_cig), 3),
    "trimmed": {"whole": int(st["n_whole"]), "cut": int(st["n_cut"]), "dropped": int(st["n_dropped"]), "chunks": int(st["n_chunks"])},
}))
