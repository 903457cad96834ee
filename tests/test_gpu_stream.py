"""Streamed locate (pba_loc_stream): batches that are copied and packed behind the locate of the batch before give, row for
row, what one pba_locate over all the reads gives; the one-pass pack writes the bytes pba_seqs_from_text writes, and leaves
nothing of an earlier batch in a reused slot."""
import os
import subprocess

import numpy as np
import pytest

from conftest import MASK_PAT, ROOT, gold_json, gold_npz
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import (PAIR_DTYPE, PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL, PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP,
                                       PBA_STREAM_RECORDS, PBA_STREAM_TEXT, PbaError)

pytestmark = pytest.mark.gpu
R, TRIALS, MIN_LEN = 0.30, 50, 500
ROW_FIELDS = ("read", "nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs", "diag_cost")


@pytest.fixture(scope="module")
def world(ctx):
    """A 6 kb contig, its index, and 150 reads: 500-1 400 bases at 15 % error, 15 of another genome, 10 below min_len."""
    g = eng.synth_genome(71, 6000)
    rd, off, _ = eng.synth_reads(72, g, 150, 1400)
    other = eng.synth_genome(73, 6000)
    ro, oo, _ = eng.synth_reads(74, other, 150, 1400)
    reads = []
    for i in range(150):
        src, so = (ro, oo) if i % 10 == 4 else (rd, off)
        L = 100 + 29 * (i % 11) if i % 15 == 7 else 500 + (i * 37) % 901
        reads.append(src[int(so[i]):int(so[i]) + L].tobytes())
    T = ctx.seqs_from_list([g.tobytes()], strict_acgt=True)
    mask = eng.mask_from_pattern(MASK_PAT)
    ix = ctx.index_build(T, 0, mask, PBA_INDEX_ALL)
    resident = {}
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    for k in (PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP):
        resident[k] = ctx.locate(ix, T, 0, Rd, R, TRIALS, MIN_LEN, kernel=k)
    Rd.close()
    yield dict(g=g, T=T, ix=ix, mask=mask, reads=reads, resident=resident)
    ix.close()
    T.close()


def rows_equal(a, b):
    assert len(a) == len(b)
    for f in ROW_FIELDS:
        assert (a[f] == b[f]).all(), f


def export_bytes(S):
    import torch
    cap = max(int(S.packed_bytes), 16)
    d = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                  # the fill runs on torch's stream, the export on the engine's
    offs = S.export(d.data_ptr(), cap)
    return d.cpu().numpy()[:int(S.packed_bytes)].copy(), offs.copy(), S.lengths().copy()


def run_pipelined(st, batches):
    """every submit before the collect of the batch before: two batches in flight throughout"""
    rows, stats = [], []
    for k, b in enumerate(batches):
        st.submit_reads(b)
        if k:
            r, s = st.collect()
            rows.append(r); stats.append(s)
    r, s = st.collect()
    rows.append(r); stats.append(s)
    return rows, stats


@pytest.mark.parametrize("kernel", [PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP])
def test_stream_equals_resident(ctx, world, kernel):
    reads = world["reads"]
    sizes, batches, at = [37, 1, 0, 64, 5, 43], [], 0
    for n in sizes:
        batches.append(reads[at:at + n]); at += n
    assert at == len(reads) == 150
    st = ctx.locate_stream(world["ix"], world["T"], 0, R, TRIALS, MIN_LEN, kernel=kernel, slot_bytes=64 * 1400, slot_reads=64)
    rows, stats = run_pipelined(st, batches)
    assert [len(r) for r in rows] == sizes
    want, want_stats = world["resident"][kernel]
    got = np.concatenate(rows)
    rows_equal(got, want)
    assert (got["read"] == np.arange(150)).all()
    for k in want_stats:
        assert sum(s[k] for s in stats) == want_stats[k], k
    assert int(got["found"].sum()) > 60 and int((got["found"] == 0).sum()) > 10
    pr = st.profile()
    assert pr["n_reads"] == 43 and pr["n_bytes"] == sum(len(x) for x in batches[-1])
    assert pr["h2d_ms"] >= 0 and pr["pack_ms"] > 0 and pr["locate_ms"] > 0 and pr["stall_ms"] >= 0
    st.close()


def test_stream_golden(ctx):
    """the reads of the first locator golden through a stream, 50 at a time (test_locate_golden holds the resident path to it)"""
    from test_oracle_golden import check_locator_rows, locator_inputs
    meta = gold_json("locator.json")[0]
    want = gold_npz("locator.npz")[meta["name"]]
    g, reads, offs = locator_inputs(meta)
    texts = [reads[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(meta["n_reads"])]
    T = ctx.seqs_from_list([g.tobytes()], strict_acgt=True)
    ix = ctx.index_build(T, 0, meta["mask"], PBA_INDEX_ALL)
    st = ctx.locate_stream(ix, T, 0, meta["R"], meta["trials"], meta["min_len"], slot_bytes=50 * meta["read_len"], slot_reads=50)
    rows, stats = run_pipelined(st, [texts[a:a + 50] for a in range(0, len(texts), 50)])
    check_locator_rows(np.concatenate(rows), want, meta["columns"], meta["name"])
    for k, v in meta["stats"].items():
        assert sum(s[k] for s in stats) == v, k
    st.close(); ix.close(); T.close()


# every residue class of the layout: 64 bases per 16 packed bytes, 32 per plane word and per thread, 16 per dword, 4 per byte,
# 2 048 per work item; and the empty read
BYTE_LENGTHS = [64, 65, 127, 32, 33, 31, 16, 17, 15, 5, 6, 7, 1, 2047, 2048, 2049, 4097, 0, 128, 63, 3, 4096]


def random_reads(lengths, seed):
    rs = np.random.RandomState(seed)
    return [np.frombuffer(b"ACGT", np.uint8)[rs.randint(0, 4, L)].tobytes() for L in lengths]


def test_stream_bytes_text(ctx, world):
    """pba_seqs_export of a streamed batch == that of pba_seqs_from_text, byte for byte, with every kind of length first and
    last in a batch, each batch landing in a slot that held another one"""
    K = len(BYTE_LENGTHS)
    st = ctx.locate_stream(world["ix"], world["T"], 0, R, TRIALS, MIN_LEN, slot_bytes=sum(BYTE_LENGTHS) + 100, slot_reads=K + 1)
    for rot in range(K):
        lengths = BYTE_LENGTHS[rot:] + BYTE_LENGTHS[:rot]
        reads = random_reads(lengths, 100 + rot)
        st.submit_reads(reads)
        P = st.pending()
        fresh = ctx.seqs_from_list(reads, strict_acgt=True)
        assert P.count == K and P.max_len == fresh.max_len and P.packed_bytes == fresh.packed_bytes and not P.non_acgt
        got, want = export_bytes(P), export_bytes(fresh)
        for a, b in zip(got, want):
            assert a.shape == b.shape and (a == b).all(), rot
        assert [P.get_text(i) for i in (0, K // 2, K - 1)] == [reads[i] for i in (0, K // 2, K - 1)]
        fresh.close()
        rows, _ = st.collect()
        assert len(rows) == K and not rows["found"].any()
    st.close()


def test_stream_bytes_records(ctx, world):
    """records form: the file is the arena, as pba_seqs_from_records has it"""
    K = len(BYTE_LENGTHS)
    cap = sum(4 + (L + 3) // 4 for L in BYTE_LENGTHS)
    st = ctx.locate_stream(world["ix"], world["T"], 0, R, TRIALS, MIN_LEN, slot_bytes=cap, slot_reads=K, form=PBA_STREAM_RECORDS)
    for rot in (0, 1, 13, 17, 5):
        lengths = (BYTE_LENGTHS[rot:] + BYTE_LENGTHS[:rot])[:K - rot % 3]          # (files of different sizes in the same slot)
        reads = random_reads(lengths, 300 + rot)
        file = b"".join(eng.text2bin(t) for t in reads)
        st.submit_records(file, 0, 1 << 30)
        P = st.pending()
        fresh = ctx.seqs_from_records(file, 0, 1 << 30)
        kept = [t for t in reads if len(t) > 0]
        assert P.count == fresh.count == len(kept) and P.packed_bytes == fresh.packed_bytes == len(file)
        got, want = export_bytes(P), export_bytes(fresh)
        for a, b in zip(got, want):
            assert a.shape == b.shape and (a == b).all(), rot
        assert [P.get_text(i) for i in range(len(kept))] == kept
        # the planes, through the bit-vector kernel: every read against itself, forward and backward
        pairs = np.array([(i, 0, len(t), i, 0, len(t), 0) for i, t in enumerate(kept)] +
                         [(i, len(t) - 1, len(t), i, len(t) - 1, len(t), 3) for i, t in enumerate(kept)], PAIR_DTYPE)
        a = ctx.align_batch(P, P, pairs, R, kernel=PBA_KERNEL_BITVEC)
        b = ctx.align_batch(fresh, fresh, pairs, R, kernel=PBA_KERNEL_BITVEC)
        long = pairs["b_len"] >= 64
        assert (a == b).all() and (a["cost"][long] == 0).all() and (a["rc"][long] == pairs["b_len"][long]).all()
        fresh.close()
        rows, _ = st.collect()
        assert len(rows) == len(kept)
    st.close()


def test_stream_reused_slot_holds_nothing_of_the_batch_before(ctx, world):
    """a slot filled to capacity, then a small batch in the same slot: planes and packed bytes behind the short reads are the
    fresh set's, for the aligner (accessors that run to the sequence's end, both directions) and for the export"""
    big = [bytes(b"T" * 1400) if i % 2 else world["reads"][0][:500] * 2 + b"T" * 400 for i in range(8)]
    small = random_reads([45, 100, 333, 64, 31, 257], 900) + [world["reads"][0], world["reads"][1]]
    assert len(world["reads"][0]) >= 500 and len(world["reads"][1]) >= 500
    st = ctx.locate_stream(world["ix"], world["T"], 0, R, TRIALS, MIN_LEN, slot_bytes=8 * 1400, slot_reads=8)
    st.submit_reads(big)                                   # slot 0, to capacity
    big_bytes, _, _ = export_bytes(st.pending())
    st.collect()
    st.submit_reads(small)                                 # slot 1
    st.collect()
    st.submit_reads(small)                                 # slot 0 again
    P = st.pending()
    fresh = ctx.seqs_from_list(small, strict_acgt=True)
    got, want = export_bytes(P), export_bytes(fresh)
    offs, lens = want[1], want[2]
    for i in range(len(small)):                            # where a short read ends, the batch before had set bits
        end = int(offs[i]) + (int(lens[i]) + 3) // 4
        assert big_bytes[end:end + 16].any(), i
    tail = big_bytes[len(want[0]):len(want[0]) + 1024]     # ... and so had the slack behind the last one
    assert len(tail) == 1024 and all(tail[k:k + 16].any() for k in range(0, 1024, 16))
    for a, b in zip(got, want):
        assert a.shape == b.shape and (a == b).all()
    n = len(small)
    pairs = []
    for i in range(n):
        for j in (i, (i + 1) % n):
            li, lj = len(small[i]), len(small[j])
            pairs.append((i, 0, li, j, 0, lj, 0))
            pairs.append((i, li - 1, li, j, lj - 1, lj, 3))
    pairs = np.array(pairs, PAIR_DTYPE)
    a = ctx.align_batch(P, P, pairs, R, kernel=PBA_KERNEL_BITVEC)
    b = ctx.align_batch(fresh, fresh, pairs, R, kernel=PBA_KERNEL_BITVEC)
    assert (a == b).all()
    assert all(int(a["rc"][4 * i]) == len(small[i]) and int(a["cost"][4 * i]) == 0 for i in range(n) if len(small[i]) >= 64)
    rows, stats = st.collect()
    want_rows, want_stats = ctx.locate(world["ix"], world["T"], 0, fresh, R, TRIALS, MIN_LEN)
    want_rows = want_rows.copy()
    want_rows["read"] += 16                                # 8 + 8 reads went through the stream before
    want_rows["nseq"][want_rows["nseq"] >= 0] += 8 + 2
    rows_equal(rows, want_rows)
    assert stats == want_stats and stats["n_reads_kept"] == 2
    fresh.close()
    st.close()


def status_of(fn, *a):
    try:
        fn(*a)
    except PbaError as e:
        return e.status
    return 0


def test_stream_refusals_and_recovery(ctx, world):
    reads, lib = world["reads"], ctx.lib
    st = ctx.locate_stream(world["ix"], world["T"], 0, R, TRIALS, MIN_LEN, slot_bytes=6000, slot_reads=4)
    assert status_of(st.collect) == -1                                  # nothing pending
    buf, offs = st.buffer()
    offs[0], offs[1] = 0, 6001
    assert status_of(st.submit, 1) == -4                                # over slot_bytes
    assert status_of(st.submit, 5) == -4                                # over slot_reads
    offs[0], offs[1], offs[2] = 0, 10, 5
    assert status_of(st.submit, 2) == -1                                # decreasing offsets
    assert status_of(st.collect) == -1 and status_of(st.pending) == -1  # the refused batches left nothing pending
    first = reads[0:3]
    st.submit_reads(first)
    st.submit_reads(reads[3:5])
    assert status_of(st.submit, 0) == -1 and status_of(st.buffer) == -1  # both slots pending
    rows = np.zeros(4, eng.LOC_ROW_DTYPE)
    n = eng.C.c_uint32()
    assert lib.pba_loc_stream_collect(st.h, eng._ptr(rows), 2, eng.C.byref(n), None) == -1      # cap below the batch size ...
    r0, _ = st.collect()                                                                        # ... and the batch is still there
    r1, _ = st.collect()
    want, _ = world["resident"][PBA_KERNEL_BITVEC]
    rows_equal(np.concatenate([r0, r1]), want[:5])
    # a batch with one N: refused at collect, dropped, and its reads keep their ids
    bad = [reads[5], reads[6][:200] + b"N" + reads[6][201:], reads[7]]
    st.submit_reads(bad)
    st.submit_reads(reads[8:12])
    assert status_of(st.collect) == -6
    r3, _ = st.collect()
    rows_equal(r3, want[8:12])
    assert int(r3["read"][0]) == 8 and (r3["nseq"][r3["nseq"] >= 0] >= 0).all()
    kept_before = sum(len(x) >= MIN_LEN for x in reads[:8])
    assert int(r3["nseq"][r3["nseq"] >= 0][0]) == kept_before
    st.submit_reads([])                                                 # the stream goes on: an empty batch
    r4, s4 = st.collect()
    assert len(r4) == 0 and s4["n_reads_kept"] == 0
    # a read beyond the engine limit
    big = ctx.locate_stream(world["ix"], world["T"], 0, R, TRIALS, MIN_LEN, slot_bytes=70000, slot_reads=2)
    _, o = big.buffer()
    o[0], o[1] = 0, 65001
    assert status_of(big.submit, 1) == -4 and status_of(big.collect) == -1
    big.close()
    # pba_locate's own checks, at create
    ht = ctx.index_build(world["T"], 0, world["mask"], PBA_INDEX_HEAD_TAIL)
    assert status_of(ctx.locate_stream, ht, world["T"], 0, R) == -1
    ht.close()
    assert status_of(lambda: ctx.locate_stream(world["ix"], world["T"], 0, R, kernel=7)) == -1
    assert status_of(lambda: ctx.locate_stream(world["ix"], world["T"], 0, R, form=2)) == -1
    # destroy with two batches pending
    st.submit_reads(reads[12:15])
    st.submit_reads(reads[15:16])
    st.close()
    rows2, _ = ctx.locate(world["ix"], world["T"], 0, ctx.seqs_from_list(reads[:5]), R, TRIALS, MIN_LEN)   # the ctx is fine
    rows_equal(rows2, want[:5])


def test_stream_example_prints_what_locator_gpu_prints(lib, tmp_path):
    from cons_scenarios import LOCATOR_CLI, locator_cli_inputs
    gold = gold_json("locator_cli.json")
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    libdir = os.path.join(ROOT, "pacbioassembly_amd", "lib")
    for name in ("locator_gpu", "locator_stream_gpu"):
        subprocess.run(["g++", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(out, name),
                        os.path.join(ROOT, "examples", name + ".cpp"), "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}"], check=True)
    contig, texts = locator_cli_inputs()
    cf = tmp_path / "contig.txt"
    cf.write_bytes(contig + b"\n")
    stdin = b"\n".join(texts) + b"\n"
    ref = subprocess.run([os.path.join(out, "locator_gpu"), str(cf), LOCATOR_CLI["pattern"]], input=stdin, capture_output=True, timeout=300)
    assert ref.returncode == 0, ref.stderr.decode()
    for per_batch in ("64", "1"):                          # 1: 400 batches, each smaller than one wavefront's worth
        r = subprocess.run([os.path.join(out, "locator_stream_gpu"), str(cf), LOCATOR_CLI["pattern"], "0.15", per_batch],
                           input=stdin, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        rows = [[int(x) for x in line.split()] for line in r.stdout.decode().splitlines()]
        assert [x[:4] for x in rows] == gold["rows"] and len(rows) > 250
        assert [x[4] for x in rows] == gold["col5"]
        assert r.stdout == ref.stdout and r.stderr == ref.stderr
