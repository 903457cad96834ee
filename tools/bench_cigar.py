#!/usr/bin/env python3
"""Run-length alignments against edit scripts on one batch: reads located on a genome (pba_locate), the located pairs as
tools/bench_consensus.py makes them (the genome as `a`), then the same batch through pba_align_batch_trace and through
pba_align_batch_cigar, alternating in one process, warmed, several repeats each.  The script path is the yardstick: the walk
is the same, the sink adds two element fetches per diagonal move.  Once at the synthetic reads' 15 % error and once at 1 %
(the corrected-read regime).  Prints one JSON line; --out also writes it to a file."""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from pacbioassembly_amd import Context, engine as eng
from pacbioassembly_amd.engine import ALN_COUNTS_DTYPE, PAIR_DTYPE, PBA_INDEX_ALL, RESULT_DTYPE

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=32768)
ap.add_argument("--read-len", type=int, default=15000)
ap.add_argument("--genome", type=int, default=5_000_000)
ap.add_argument("--R", type=float, default=0.30)
ap.add_argument("--repeats", type=int, default=4)
ap.add_argument("--out", default="")
a = ap.parse_args()
ctx = Context(0)
g = eng.synth_genome(2, a.genome)
T = ctx.seqs_from_list([g.tobytes()])
ix = ctx.index_build(T, 0, eng.mask_from_pattern("111*11*11*1*1111"), PBA_INDEX_ALL)
ptr = lambda x: C.c_void_p(x.ctypes.data)


def regime(name, p):
    reads, offs, _ = eng.synth_reads(3, g, a.reads, a.read_len, p, p, p, nthreads=16)
    Rd = ctx.seqs_from_text(reads, offs, strict_acgt=True)
    rows, _ = ctx.locate(ix, T, 0, Rd, a.R, 50, 500)
    hit = rows[rows["found"] == 1]
    n = int(hit.size)
    md = 1 + int(a.read_len * a.R)
    pairs = np.zeros(n, PAIR_DTYPE)
    pairs["a_seq"] = 0; pairs["a_pos"] = hit["pos"]; pairs["a_len"] = np.minimum(a.genome - hit["pos"], hit["seglen"] + md + 16)
    pairs["b_seq"] = hit["read"]; pairs["b_pos"] = hit["j"]; pairs["b_len"] = hit["seglen"]
    out = np.zeros(n, RESULT_DTYPE)
    # scripts: a_len + b_len byte slots per pair
    ooff = np.zeros(n + 1, np.uint64)
    ooff[1:] = np.cumsum(pairs["a_len"].astype(np.int64) + pairs["b_len"].astype(np.int64))
    ops = np.zeros(int(ooff[-1]) + 1, np.uint8)
    ne = np.zeros(n, np.int32)
    # runs: pba_cigar_bound word slots per pair
    coff = np.zeros(n + 1, np.uint64)
    coff[1:] = np.cumsum([eng.cigar_bound(int(p_["a_len"]), int(p_["b_len"]), a.R) for p_ in pairs])
    cig = np.zeros(int(coff[-1]) + 1, np.uint32)
    ncig = np.zeros(n, np.int32)
    counts = np.zeros(n, ALN_COUNTS_DTYPE)

    def trace():
        ctx.check(ctx.lib.pba_align_batch_trace(ctx.h, T.h, Rd.h, ptr(pairs), n, a.R, 0, 0, 0, ptr(out), ptr(ops), ptr(ooff), ptr(ne)), "trace")

    def cigar():
        ctx.check(ctx.lib.pba_align_batch_cigar(ctx.h, T.h, Rd.h, ptr(pairs), n, a.R, 0, 0, 0, ptr(out), ptr(cig), ptr(coff), ptr(ncig),
                                                ptr(counts)), "cigar")

    wall, kern = {"trace": [], "cigar": []}, {"trace": [], "cigar": []}
    for rep in range(a.repeats + 1):                            # the first round of both warms up
        for which, fn in (("trace", trace), ("cigar", cigar)):
            t = time.perf_counter()
            fn()                                                # (returns synchronised, its results on the host)
            dt = time.perf_counter() - t
            pr = ctx.last_profile()
            if rep:
                wall[which].append(dt)
                kern[which].append(pr["align_ms"] + pr["align_redo_ms"])
    ok = int((out["rc"] >= 0).sum())
    assert ok and (ne[out["rc"] >= 0] > 0).all() and (ncig[out["rc"] >= 0] > 0).all()
    assert (counts["n_x"] + counts["n_ins"] + counts["n_del"] == out["cost"]).all()
    res = {"pairs": n, "ok": ok, "mean_runs": round(float(ncig.sum()) / max(ok, 1), 1), "mean_ops": round(float(ne.sum()) / max(ok, 1), 1)}
    for which in ("trace", "cigar"):
        w, k = np.array(wall[which]), np.array(kern[which])
        res[which] = {"pairs_per_s_wall": round(n / float(np.median(w)), 1), "pairs_per_s_kernels": round(n / (float(np.median(k)) / 1e3), 1),
                      "wall_s": [round(float(x), 3) for x in w], "kernel_ms": [round(float(x), 1) for x in k],
                      "spread_wall": round(float((w.max() - w.min()) / np.median(w)), 3),
                      "spread_kernels": round(float((k.max() - k.min()) / np.median(k)), 3)}
    # device-to-host bytes of one call: results, counts per pair, then every script slot / the real runs and their offsets
    res["trace"]["d2h_bytes"] = int(n * 32 + n * 4 + int(ooff[-1]))
    res["cigar"]["d2h_bytes"] = int(n * 32 + n * 4 + n * 16 + (n + 1) * 8 + 4 * int(ncig.sum()))
    return name, res


line = {"workload": f"{a.reads} synthetic {a.read_len}-base reads located on a {a.genome}-base genome, R = {a.R}: scripts "
                    f"(pba_align_batch_trace) and runs (pba_align_batch_cigar) of the located pairs, alternating, {a.repeats} repeats each"}
for name, p in (("err15", 0.05), ("err1", 1.0 / 300)):
    k, v = regime(name, p)
    line[k] = v
s = json.dumps(line)
print(s)
if a.out:
    with open(a.out, "w") as f:
        f.write(s + "\n")
