#!/usr/bin/env python3
"""What reading a FASTA / FASTQ file into a sequence set costs, next to the same reads handed over already split.

  tools/bench_fastx.py --reads 100000 --len 15000 [--fastq] [--width 0] [--out profiles/fastx_line.json]

The file image of synthetic reads (15 % error, fixed-width names; FASTA in lines of --width, 0 = one line) is built on the host
-- that is not timed.  Timed, one warm-up pass and --passes passes of each, medians with min-max:
  fastx   seqs_from_fastx of the image: host clock, and the HIP-event times of its stats (copy, parse, pack)
  text    seqs_from_text of the same reads as text plus offsets: host clock.  Nothing of that path is this tool's subject: it
          is the floor an ingest can reach, since the ASCII has to cross and be packed either way
plus write_fasta of the parsed set (host clock).  One JSON object under the key "fasta" / "fastq" of --out; the other key of
an existing file is kept.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pacbioassembly_amd import Context, engine as eng  # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def image(reads: np.ndarray, n: int, rl: int, fastq: bool, width: int) -> np.ndarray:
    """'>r000000123\\n' + bases (+ '\\n+\\n' + qualities) + '\\n' per read, as one u8 array"""
    name = np.empty((n, 12), np.uint8)
    name[:, 0] = ord("@" if fastq else ">")
    name[:, 1] = ord("r")
    ids = np.arange(n, dtype=np.int64)
    for k in range(9):
        name[:, 10 - k] = 48 + (ids // 10 ** k) % 10
    name[:, 11] = 10
    seq = reads.reshape(n, rl)
    if fastq:
        rec = np.empty((n, 12 + rl + 3 + rl + 1), np.uint8)
        rec[:, :12] = name
        rec[:, 12:12 + rl] = seq
        rec[:, 12 + rl:12 + rl + 3] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 12 + rl + 3:-1] = ord("I")
        rec[:, -1] = 10
        return rec.reshape(-1)
    if width <= 0 or width >= rl:
        rec = np.empty((n, 12 + rl + 1), np.uint8)
        rec[:, :12] = name
        rec[:, 12:12 + rl] = seq
        rec[:, -1] = 10
        return rec.reshape(-1)
    full, rest = divmod(rl, width)
    body = np.empty((n, full, width + 1), np.uint8)
    body[:, :, :width] = seq[:, :full * width].reshape(n, full, width)
    body[:, :, width] = 10
    parts = [name, body.reshape(n, -1)]
    if rest:
        tail = np.empty((n, rest + 1), np.uint8)
        tail[:, :rest] = seq[:, full * width:]
        tail[:, rest] = 10
        parts.append(tail)
    return np.concatenate(parts, axis=1).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--len", type=int, default=15_000, dest="rl")
    ap.add_argument("--fastq", action="store_true")
    ap.add_argument("--width", type=int, default=0)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, rl = a.reads, a.rl
    ctx = Context(0)
    genome = eng.synth_genome(2, max(a.genome, 2 * rl))
    reads, offs, _ = eng.synth_reads(3, genome, n, rl, 0.05, 0.05, 0.05, nthreads=a.threads)
    img = image(reads, n, rl, a.fastq, a.width)

    fx_wall, ev, text_wall, wr_wall, stats = [], {"h2d_ms": [], "parse_ms": [], "pack_ms": []}, [], [], None
    for p in range(a.passes + 1):
        t0 = time.perf_counter()
        S, ix = ctx.seqs_from_fastx(img)
        t1 = time.perf_counter()
        if p == a.passes:                                         # once: the round trip is the file's reads
            assert S.count == n and ix.stats["n_bases"] == n * rl and not S.non_acgt
            assert ix.names(img)[n - 1] == "r%09d" % (n - 1)
        w0 = time.perf_counter()
        out = S.write_fasta(None, 60, 0, n) if p else b""
        w1 = time.perf_counter()
        S.close()
        t2 = time.perf_counter()
        W = ctx.seqs_from_text(reads, offs, strict_acgt=False)
        t3 = time.perf_counter()
        W.close()
        if p:                                                     # pass 0 warms the pool and the allocator
            fx_wall.append((t1 - t0) * 1e3); text_wall.append((t3 - t2) * 1e3); wr_wall.append((w1 - w0) * 1e3)
            for k in ev:
                ev[k].append(ix.stats[k])
            stats = ix.stats
            wr_bytes = len(out)
    fx, tx = statistics.median(fx_wall), statistics.median(text_wall)
    line = {"tool": "bench_fastx", "format": "fastq" if a.fastq else "fasta", "reads": n, "read_len": rl, "width": a.width,
            "file_bytes": int(img.size), "device": ctx.device_info()["name"],
            "fastx_wall_ms": spread(fx_wall), "fastx_events_ms": {k: spread(v) for k, v in ev.items()},
            "seqs_from_text_wall_ms": spread(text_wall), "fastx_over_text": round(fx / tx, 3),
            "file_gb_per_s_wall": round(img.size / fx / 1e6, 3),
            "file_gb_per_s_parse": round(img.size / statistics.median(ev["parse_ms"]) / 1e6, 3),
            "write_fasta_wall_ms": spread(wr_wall), "write_fasta_bytes": wr_bytes,
            "stats": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in stats.items()}}
    print(json.dumps(line))
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                doc = json.load(f)
        doc[line["format"]] = line
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
