#!/usr/bin/env python3
"""Streamed locate against what a caller with fresh reads every step does today.

  tools/bench_stream.py --reads 100000 --batches 8 [--form text|records] [--out FILE]

The BASELINE configs[1] shape (synthetic 15 kb reads @15 % error against a 5 Mb genome) cut into equal batches; one warm-up
pass and --passes timed passes of each leg, medians with min-max, one JSON line:
  serial    per batch seqs_from_text (seqs_from_records) + locate + destroy, host clock                         -- (a)
  streamed  host clock from the first submit to the last collect / batches, two batches in flight, with the
            per-batch h2d / pack / locate / stall event times; the fill of the pinned buffers is timed apart       -- (b)
  floor     one batch in flight at a time: the copy from pinned memory alone and the locate alone, by HIP
            events; the floor of a batch is the larger of the two                                                -- (c)
The resident ms per step of the whole set (bench.py) is measured by bench.py itself.
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

MASK_PAT = "111*11*11*1*1111"


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--read-len", type=int, default=15_000)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--R", type=float, default=0.30)
    ap.add_argument("--trials", type=int, default=50)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--form", choices=["text", "records"], default="text")
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    per = a.reads // a.batches
    n, rl = per * a.batches, a.read_len
    records = a.form == "records"
    ctx = Context(0)
    genome = eng.synth_genome(2, a.genome)
    reads, _, _ = eng.synth_reads(3, genome, n, rl, 0.05, 0.05, 0.05, nthreads=a.threads)
    T = ctx.seqs_from_text(genome, np.array([0, genome.size], np.uint64), strict_acgt=True)
    ix = ctx.index_build(T, 0, eng.mask_from_pattern(MASK_PAT), eng.PBA_INDEX_ALL)
    offs = np.arange(per + 1, dtype=np.uint64) * np.uint64(rl)
    if records:       # the same reads as binary read files, one per batch (host packing is not part of any leg)
        rec = 4 + (rl + 3) // 4
        files = []
        for b in range(a.batches):
            f = np.empty((per, rec), np.uint8)
            for i in range(per):
                f[i] = np.frombuffer(eng.text2bin(reads[(b * per + i) * rl:(b * per + i + 1) * rl].tobytes()), np.uint8)
            files.append(f.reshape(-1))
        file_bytes = [f.tobytes() for f in files]                                    # (what seqs_from_records takes)
        batch = lambda b: files[b]                                                   # noqa: E731
        slot_bytes = per * rec
    else:
        batch = lambda b: reads[b * per * rl:(b + 1) * per * rl]                     # noqa: E731
        slot_bytes = per * rl

    def serial_pass():
        t0, located = time.perf_counter(), 0
        for b in range(a.batches):
            S = ctx.seqs_from_records(file_bytes[b], 0, 1 << 30) if records else ctx.seqs_from_text(batch(b), offs, strict_acgt=True)
            _, st = ctx.locate(ix, T, 0, S, a.R, a.trials, 500)
            S.close()
            located += st["n_located"]
        return (time.perf_counter() - t0) * 1e3 / a.batches, located

    st = ctx.locate_stream(ix, T, 0, a.R, a.trials, 500, slot_bytes=slot_bytes, slot_reads=per,
                           form=eng.PBA_STREAM_RECORDS if records else eng.PBA_STREAM_TEXT)

    def fill(b):
        t0 = time.perf_counter()
        buf, o = st.buffer()
        src = batch(b)
        buf[:src.size] = src
        if records:
            o[0], o[1], o[2] = src.size, 0, 1 << 30
        else:
            o[:per + 1] = offs
        return (time.perf_counter() - t0) * 1e3

    def stream_pass(in_flight):
        profs, fills, located = [], 0.0, 0
        t0 = time.perf_counter()
        for b in range(a.batches):
            fills += fill(b)
            st.submit(per)
            if b + 1 >= in_flight:
                _, s = st.collect()
                located += s["n_located"]
                profs.append(st.profile())
        for _ in range(in_flight - 1):
            _, s = st.collect()
            located += s["n_located"]
            profs.append(st.profile())
        wall = (time.perf_counter() - t0) * 1e3
        return wall / a.batches, fills / a.batches, profs, located

    serial_pass(); stream_pass(2); stream_pass(1)                                    # warm-up: pools, code objects, first touches
    ser, strm, strm_nofill, fl, alone_h2d, alone_loc, alone_pack = [], [], [], [], [], [], []
    per_batch = {k: [] for k in ("h2d_ms", "pack_ms", "locate_ms", "stall_ms")}
    located = set()
    for _ in range(a.passes):                                                        # the legs alternate inside one session
        w, l0 = serial_pass(); ser.append(w)
        w, f, profs, l1 = stream_pass(2); strm.append(w); strm_nofill.append(w - f); fl.append(f)
        for k in per_batch:
            per_batch[k].append(statistics.median(p[k] for p in profs))
        _, _, profs, l2 = stream_pass(1)
        alone_h2d.append(statistics.median(p["h2d_ms"] for p in profs))
        alone_pack.append(statistics.median(p["pack_ms"] for p in profs))
        alone_loc.append(statistics.median(p["locate_ms"] for p in profs))
        located |= {l0, l1, l2}
    assert len(located) == 1, located                                                # every leg located the same reads
    nbytes = slot_bytes
    floor = [max(h, l) for h, l in zip(alone_h2d, alone_loc)]
    out = {
        "tool": "bench_stream", "form": a.form, "reads": n, "batches": a.batches, "read_len": rl, "genome": a.genome, "R": a.R,
        "batch_bytes": nbytes, "n_located": located.pop(), "device": ctx.device_info()["name"],
        "a_serial_ms_per_batch": spread(ser),
        "b_streamed_ms_per_batch": spread(strm), "b_streamed_less_fill_ms_per_batch": spread(strm_nofill),
        "b_fill_ms_per_batch": spread(fl), "b_per_batch_event_ms": {k: spread(v) for k, v in per_batch.items()},
        "c_alone_h2d_ms": spread(alone_h2d), "c_alone_pack_ms": spread(alone_pack), "c_alone_locate_ms": spread(alone_loc),
        "c_floor_ms_per_batch": spread(floor),
        "link_GBps": round(nbytes / (statistics.median(alone_h2d) * 1e-3) / 1e9, 2),
        "b_over_c": round(statistics.median(strm) / statistics.median(floor), 3),
        "b_less_fill_over_c": round(statistics.median(strm_nofill) / statistics.median(floor), 3),
        "a_over_b": round(statistics.median(ser) / statistics.median(strm), 3),
        "b_below_a_by_more_than_a_spread": bool(statistics.median(ser) - statistics.median(strm) > max(ser) - min(ser)),
        "b_less_fill_below_a_by_more_than_a_spread": bool(statistics.median(ser) - statistics.median(strm_nofill) > max(ser) - min(ser)),
    }
    st.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
