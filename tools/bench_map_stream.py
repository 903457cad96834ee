#!/usr/bin/env python3
"""Streamed mapping against what a caller with fresh reads every step does without it.

  tools/bench_map_stream.py --reads 100000 --batch 12500 [--parent-lib FILE] [--out FILE]

The workload of tools/bench_map.py -- a 5 Mb genome cut into --contigs equal contigs, synthetic 15 kb reads @15 % error, a
seeded random half of them reverse-complemented (here on the host: the legs start from host text), R = 0.30, 50 trials,
strands = 3 -- cut into batches of --batch reads.  End to end, host text to collected rows, reads per second:
  a  streamed   one MapStream, one batch in flight behind the other (submit k+1, then collect k); the copy of a batch into
                the pinned buffer is part of the leg and is also timed apart, with the per-batch h2d / pack / locate / stall
                event times of the stream;
  b  parent     per batch seqs_from_text + seqs_revcomp + map_reads + close, what a caller did before the stream existed.
                With --parent-lib (or PBA_PARENT_LIB) this leg runs against that library -- one built from the commit
                before pba_map_stream -- and binds none of the new entry points; otherwise against the in-tree library.
A leg is a process of its own (a process binds one library): one warm-up pass, --passes timed passes.  The legs alternate,
--repeats times each, in one invocation; the figures are medians with min - max over all timed passes of a leg.  Both legs'
rows (read and nseq made global for leg b) must be identical: their digests are compared.  One JSON line."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MASK_PAT = "111*11*11*1*1111"
NEW = ("pba_map_stream_create", "pba_map_stream_buffer", "pba_map_stream_submit", "pba_map_stream_collect",
       "pba_map_stream_pending", "pba_map_stream_last_profile", "pba_map_stream_destroy")


def spread(v, nd=3):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--batch", type=int, default=12_500)
    ap.add_argument("--read-len", type=int, default=15_000)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--contigs", type=int, default=1000)
    ap.add_argument("--R", type=float, default=0.30)
    ap.add_argument("--trials", type=int, default=50)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--threads", type=int, default=int(os.environ.get("OMP_NUM_THREADS", "8")))
    ap.add_argument("--parent-lib", default=os.environ.get("PBA_PARENT_LIB"))
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", choices=["a", "b"], default=None, help="(internal) run one leg and write its result to --leg-out")
    ap.add_argument("--leg-out", default=None)
    return ap.parse_args()


def leg(a):
    """One leg in this process: {"wall_ms": [per pass], "digest": ..., ...}."""
    import numpy as np
    from pacbioassembly_amd import _lib
    if a.leg == "b" and os.environ.get("PBA_LIB_PATH"):
        for name in NEW:
            _lib.SYMBOLS.pop(name, None)
    from pacbioassembly_amd import Context, engine as eng
    per, rl = a.batch, a.read_len
    nb = a.reads // per
    n = nb * per
    ctx = Context(0)
    g = eng.synth_genome(2, a.genome)
    text, _, _ = eng.synth_reads(3, g, n, rl, 0.05, 0.05, 0.05, nthreads=a.threads)
    text = text.reshape(n, rl)
    flip = np.random.default_rng(4).integers(0, 2, n).astype(bool)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    text[flip] = comp[text[flip][:, ::-1]]                       # the mixed-strand reads, as host text
    text = text.reshape(-1)
    cuts = np.linspace(0, g.size, a.contigs + 1).astype(np.uint64)
    T = ctx.seqs_from_text(g, cuts, strict_acgt=True)
    ix = ctx.index_build_set(T, eng.mask_from_pattern(MASK_PAT))
    offs = np.arange(per + 1, dtype=np.uint64) * np.uint64(rl)
    batch = lambda b: text[b * per * rl:(b + 1) * per * rl]      # noqa: E731
    res = {"leg": a.leg, "library": "PBA_LIB_PATH" if os.environ.get("PBA_LIB_PATH") else "in-tree", "reads": n, "batches": nb}

    if a.leg == "a":
        st = ctx.map_stream(ix, T, a.R, a.trials, 500, strands=3, slot_bytes=per * rl, slot_reads=per)

        def one_pass():
            rows, profs, fills = [], [], 0.0
            t0 = time.perf_counter()
            for b in range(nb):
                t = time.perf_counter()
                buf, o = st.buffer()
                buf[:per * rl] = batch(b)
                o[:per + 1] = offs
                fills += time.perf_counter() - t
                st.submit(per)
                if b:
                    rows.append(st.collect()[0]); profs.append(st.profile())
            rows.append(st.collect()[0]); profs.append(st.profile())
            wall = time.perf_counter() - t0
            rows = np.concatenate(rows)                          # (the stream's ids run on from pass to pass: count from this pass's first)
            kept = rows["nseq"] >= 0
            rows["read"] -= rows["read"][0]
            rows["nseq"][kept] -= rows["nseq"][kept].min()
            return wall * 1e3, fills * 1e3, rows, profs
    else:
        def one_pass():
            rows, read_base, nseq_base = [], 0, 0
            t0 = time.perf_counter()
            for b in range(nb):
                S = ctx.seqs_from_text(batch(b), offs, strict_acgt=True)
                Rc = ctx.seqs_revcomp(S)
                r, _ = ctx.map_reads(ix, T, S, a.R, a.trials, 500, strands=3, reads_rc=Rc)
                Rc.close(); S.close()
                r = r.copy()
                r["read"] += read_base
                kept = r["nseq"] >= 0
                r["nseq"][kept] += nseq_base
                read_base += per; nseq_base += int(kept.sum())
                rows.append(r)
            wall = time.perf_counter() - t0
            return wall * 1e3, 0.0, np.concatenate(rows), []

    one_pass()                                                   # warm-up: pools, code objects, first touches
    walls, fills, events, digests = [], [], {k: [] for k in ("h2d_ms", "pack_ms", "locate_ms", "stall_ms")}, set()
    hidden = []
    for _ in range(a.passes):
        w, f, rows, profs = one_pass()
        walls.append(w); fills.append(f)
        digests.add(hashlib.sha256(np.ascontiguousarray(rows).tobytes()).hexdigest())
        for k in events:
            events[k] += [float(p[k]) for p in profs]
        # batch k+1's upload hides behind batch k's walks when they take longer than its copy and pack
        hidden += [float(q["stall_ms"]) for p, q in zip(profs, profs[1:]) if p["locate_ms"] > q["h2d_ms"] + q["pack_ms"]]
    assert len(digests) == 1, "the rows differ between passes"
    res.update(wall_ms=walls, fill_ms=fills, digest=digests.pop(), n_found=int(rows["found"].sum()),
               n_minus=int((rows["strand"] == -1).sum()), device=ctx.device_info()["name"])
    if a.leg == "a":
        res["per_batch_event_ms"] = {k: spread(v) for k, v in events.items()}
        res["stall_ms_where_the_walks_cover_the_next_upload"] = spread(hidden) if hidden else None
        res["n_batches_where_the_walks_cover_the_next_upload"] = len(hidden)
        st.close()
    with open(a.leg_out, "w") as f:
        json.dump(res, f)


def main():
    a = args()
    if a.leg:
        return leg(a)
    me = [sys.executable, os.path.abspath(__file__)] + [x for x in sys.argv[1:]]
    got = {"a": [], "b": []}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(a.repeats):                             # the legs alternate inside one invocation
            for which in ("a", "b"):
                out = os.path.join(tmp, f"{which}{rep}.json")
                env = dict(os.environ)
                env.pop("PBA_LIB_PATH", None)
                if which == "b" and a.parent_lib:
                    env["PBA_LIB_PATH"] = os.path.abspath(a.parent_lib)
                subprocess.run(me + ["--leg", which, "--leg-out", out], check=True, env=env)
                got[which].append(json.load(open(out)))
                print(f"leg {which}, repeat {rep}: {[round(x) for x in got[which][-1]['wall_ms']]} ms per pass", file=sys.stderr, flush=True)
    digests = {r["digest"] for rs in got.values() for r in rs}
    assert len(digests) == 1, ("the legs' rows differ", digests)
    n = got["a"][0]["reads"]
    rate = {w: [n / (ms * 1e-3) for r in got[w] for ms in r["wall_ms"]] for w in got}
    rate_nofill = [n / ((ms - f) * 1e-3) for r in got["a"] for ms, f in zip(r["wall_ms"], r["fill_ms"])]
    med = {w: statistics.median(v) for w, v in rate.items()}
    b_spread = max(rate["b"]) - min(rate["b"])
    last = got["a"][-1]
    line = {
        "tool": "bench_map_stream", "reads": n, "batch": a.batch, "batches": got["a"][0]["batches"], "read_len": a.read_len,
        "genome": a.genome, "contigs": a.contigs, "R": a.R, "trials": a.trials, "passes": a.passes, "repeats": a.repeats,
        "device": last["device"], "n_found": last["n_found"], "n_minus": last["n_minus"], "rows_identical": True,
        "b_library": got["b"][0]["library"],
        "a_streamed_reads_per_s": spread(rate["a"], 0), "a_streamed_less_fill_reads_per_s": spread(rate_nofill, 0),
        "a_fill_ms_per_pass": spread([f for r in got["a"] for f in r["fill_ms"]]),
        "b_parent_route_reads_per_s": spread(rate["b"], 0),
        "a_over_b": round(med["a"] / med["b"], 3),
        "a_above_b_by_more_than_b_spread": bool(med["a"] - med["b"] > b_spread),
        "a_less_fill_over_b": round(statistics.median(rate_nofill) / med["b"], 3),
        "a_less_fill_above_b_by_more_than_b_spread": bool(statistics.median(rate_nofill) - med["b"] > b_spread),
        "a_ms_per_batch": spread([ms / got["a"][0]["batches"] for r in got["a"] for ms in r["wall_ms"]]),
        "b_ms_per_batch": spread([ms / got["b"][0]["batches"] for r in got["b"] for ms in r["wall_ms"]]),
        "a_per_batch_event_ms": last["per_batch_event_ms"],
        "a_stall_ms_where_the_walks_cover_the_next_upload": last["stall_ms_where_the_walks_cover_the_next_upload"],
        "a_n_batches_where_the_walks_cover_the_next_upload": last["n_batches_where_the_walks_cover_the_next_upload"],
    }
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
