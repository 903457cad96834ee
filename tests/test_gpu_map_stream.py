"""Streamed mapping (pba_map_stream): batches whose both strands are copied and packed behind the walks of the batch before
give, row for row and stat for stat, what one pba_map_reads over all the reads gives (and what tests/map_ref.py gives); the
slot's two sets hold the bytes pba_seqs_from_text and pba_seqs_revcomp write, and nothing of an earlier batch.  The world's
composition is judged on the CPU in tests/test_map_stream_cpu.py.  Needs a real MI355X (-m gpu)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import MASK_PAT, ROOT
from map_ref import map_reads_ref, rc
from map_stream_inputs import BATCH_SIZES, MIN_LEN, N_READS, R, TRIALS, batches_of, composition, rows_tsv, world
from seqs_edge_inputs import EDGE_LENGTHS, ROTATIONS, host_packed, np_revcomp, self_pairs
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import (MAP_ROW_DTYPE, PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP, PBA_STREAM_RECORDS,
                                       PBA_STREAM_TEXT)
from test_gpu_map import ROW_COLS, same_rows, same_stats
from test_gpu_stream import export_bytes, random_reads, run_pipelined, status_of

pytestmark = pytest.mark.gpu
KERNELS = [PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP]
ALL_COLS = ROW_COLS + ("diag_cost",)
STAT_KEYS = ("n_reads_kept", "n_probe_hits", "n_pairs", "n_located", "n_cells")


@pytest.fixture(scope="module")
def mw(ctx, oracle):
    """The world, its set index, the resident answers (computed once, never modified) and the restatement's."""
    contigs, reads, _ = world()
    mask = eng.mask_from_pattern(MASK_PAT)
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    ix = ctx.index_build_set(T, mask)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    resident = {(k, s): ctx.map_reads(ix, T, Rd, R, TRIALS, MIN_LEN, kernel=k, strands=s) for k in KERNELS for s in (1, 2, 3)}
    Rd.close()
    ref_rows, ref_stats, _ = map_reads_ref(oracle, contigs, reads, mask, R, TRIALS, MIN_LEN, strands=3)
    yield dict(contigs=contigs, reads=reads, mask=mask, T=T, ix=ix, resident=resident, ref=(ref_rows, ref_stats))
    ix.close()
    T.close()


def all_cols_equal(got, want):
    assert len(got) == len(want)
    same_rows(got, want, ALL_COLS)


def sum_stats(stats):
    return {"strand": [{k: sum(s["strand"][i][k] for s in stats) for k in STAT_KEYS} for i in range(2)],
            "n_second_walk": sum(s["n_second_walk"] for s in stats)}


# ----------------------------------------------------------------------------- 1. streamed equals resident
@pytest.mark.parametrize("strands", [1, 2, 3])
@pytest.mark.parametrize("kernel", KERNELS)
def test_streamed_equals_resident(ctx, mw, kernel, strands):
    reads = mw["reads"]
    batches = batches_of(reads)
    st = ctx.map_stream(mw["ix"], mw["T"], R, TRIALS, MIN_LEN, kernel=kernel, strands=strands, slot_bytes=64 * 1400, slot_reads=64)
    rows, stats = run_pipelined(st, batches)
    assert [len(r) for r in rows] == BATCH_SIZES
    want, want_stats = mw["resident"][(kernel, strands)]
    got = np.concatenate(rows)
    assert got.dtype == MAP_ROW_DTYPE
    all_cols_equal(got, want)
    assert (got["read"] == np.arange(N_READS)).all()
    assert sum_stats(stats) == want_stats
    if strands == 3:
        ref_rows, ref_stats = mw["ref"]
        same_rows(got, ref_rows)
        same_stats(sum_stats(stats), ref_stats)
        verdict = composition(got, sum_stats(stats)["n_second_walk"], reads)
        assert all(verdict.values()), verdict
    else:
        assert sum_stats(stats)["n_second_walk"] == 0 and int(got["found"].sum()) >= 30
        assert set(got["strand"][got["found"] == 1].tolist()) == {1 if strands == 1 else -1}
    pr = st.profile()
    assert pr["n_reads"] == 43 and pr["n_bytes"] == sum(len(x) for x in batches[-1])
    assert pr["h2d_ms"] >= 0 and pr["pack_ms"] > 0 and pr["locate_ms"] > 0 and pr["stall_ms"] >= 0
    assert max(pr["h2d_ms"], pr["pack_ms"], pr["locate_ms"], pr["stall_ms"]) < 60_000
    st.close()


# ----------------------------------------------------------------------------- 2. both sets of a slot, byte for byte
def check_slot_sets(ctx, st, fresh, fresh_rc, kept, text_layout_fwd):
    """pending()'s two sets against the resident set and its revcomp, and the rc set against numpy + the host codec"""
    P, Q = st.pending()
    assert Q is not None
    assert np_revcomp(b"AACGTT" + b"C") == b"GAACGTT" and all(np_revcomp(t) == rc(t) for t in kept[:3])
    for borrowed, want_set, texts in ((P, fresh, kept), (Q, fresh_rc, [np_revcomp(t) for t in kept])):
        assert borrowed.count == want_set.count == len(kept) and borrowed.max_len == want_set.max_len
        assert borrowed.packed_bytes == want_set.packed_bytes and not borrowed.non_acgt
        got, want = export_bytes(borrowed), export_bytes(want_set)
        for a, b in zip(got, want):
            assert a.shape == b.shape and (a == b).all()
        if text_layout_fwd or borrowed is Q:
            host = host_packed(texts, got[1])
            assert host.shape == got[0].shape and (host == got[0]).all()
        assert [borrowed.get_text(i) for i in range(len(kept))] == texts
        # the planes, which export does not show: every read against itself across the borrowed and the resident set
        pairs = self_pairs(texts)
        res = ctx.align_batch(borrowed, want_set, pairs, R, kernel=PBA_KERNEL_BITVEC)
        base = ctx.align_batch(want_set, want_set, pairs, R, kernel=PBA_KERNEL_BITVEC)
        assert (res == base).all()
        assert (res["rc"] == pairs["b_len"]).all() and (res["cost"] == 0).all()


def test_rotations_put_short_reads_first_and_last():
    firsts = [EDGE_LENGTHS[r] for r, _ in ROTATIONS]
    lasts = [EDGE_LENGTHS[r - 1] for r, _ in ROTATIONS]
    assert any(0 < x < 32 for x in firsts) and any(0 < x < 32 for x in lasts) and 0 in firsts and 0 in lasts
    assert any(x > 2048 for x in firsts) and any(x > 2048 for x in lasts)


@pytest.mark.parametrize("form", [PBA_STREAM_TEXT, PBA_STREAM_RECORDS])
def test_both_sets_of_a_slot_byte_for_byte(ctx, mw, form):
    K = len(EDGE_LENGTHS)
    text = form == PBA_STREAM_TEXT
    cap = sum(EDGE_LENGTHS) + 100 if text else sum(4 + (L + 3) // 4 for L in EDGE_LENGTHS)
    st = ctx.map_stream(mw["ix"], mw["T"], R, TRIALS, MIN_LEN, slot_bytes=cap, slot_reads=K, form=form)
    for rot, _ in ROTATIONS:                                   # (every batch lands in a slot that held another one)
        lengths = EDGE_LENGTHS[rot:] + EDGE_LENGTHS[:rot]
        reads = random_reads(lengths, 500 + rot)
        if text:
            st.submit_reads(reads)
            kept = reads
            fresh = ctx.seqs_from_list(reads, strict_acgt=True)
        else:
            file = b"".join(eng.text2bin(t) for t in reads)
            st.submit_records(file, 0, 1 << 30)
            kept = [t for t in reads if len(t) > 0]
            fresh = ctx.seqs_from_records(file, 0, 1 << 30)
        fresh_rc = ctx.seqs_revcomp(fresh)
        check_slot_sets(ctx, st, fresh, fresh_rc, kept, text)
        fresh.close(); fresh_rc.close()
        rows, _ = st.collect()
        assert len(rows) == len(kept) and not rows["found"].any()
    st.close()


# ----------------------------------------------------------------------------- 3. a reused slot
def test_reused_slot_holds_nothing_of_the_batch_before(ctx, mw):
    """64 long reads to the slot's capacity, then 3 short ones in the same slot: rows and both sets' bytes are a fresh
    stream's, and the resident sets'"""
    reads = mw["reads"]
    long_reads = [x for x in reads if len(x) >= 900][:32]
    big = [(x + x)[:1400] for x in long_reads] * 2
    small = random_reads([45, 333, 31], 77)[:2] + [reads[0]]
    assert len(big) == 64 and len(reads[0]) >= MIN_LEN

    def small_through(st):
        st.submit_reads(small)
        P, Q = st.pending()
        out = export_bytes(P), export_bytes(Q)
        fresh = ctx.seqs_from_list(small, strict_acgt=True)
        fresh_rc = ctx.seqs_revcomp(fresh)
        check_slot_sets(ctx, st, fresh, fresh_rc, small, True)
        fresh.close(); fresh_rc.close()
        return out, st.collect()

    used = ctx.map_stream(mw["ix"], mw["T"], R, TRIALS, MIN_LEN, slot_bytes=64 * 1400, slot_reads=64)
    used.submit_reads(big)                                     # slot 0, to capacity
    P, Q = used.pending()
    big_bytes = export_bytes(P)[0], export_bytes(Q)[0]
    used.collect()
    used.submit_reads(small)                                   # slot 1
    used.collect()
    (got_f, got_r), (got_rows, got_stats) = small_through(used)    # slot 0 again
    new = ctx.map_stream(mw["ix"], mw["T"], R, TRIALS, MIN_LEN, slot_bytes=64 * 1400, slot_reads=64)
    (want_f, want_r), (want_rows, want_stats) = small_through(new)
    for got, want, before in ((got_f, want_f, big_bytes[0]), (got_r, want_r, big_bytes[1])):
        for a, b in zip(got, want):
            assert a.shape == b.shape and (a == b).all()
        offs, lens = want[1], want[2]
        for i in range(len(small)):                            # where a short read ends, the batch before had set bits
            end = int(offs[i]) + (int(lens[i]) + 3) // 4
            assert before[end:end + 16].any(), i
    want_rows = want_rows.copy()
    want_rows["read"] += 64 + 3
    want_rows["nseq"][want_rows["nseq"] >= 0] += 64 + 1
    all_cols_equal(got_rows, want_rows)
    assert got_stats == want_stats and int(got_rows["found"][2]) == int(mw["resident"][(PBA_KERNEL_BITVEC, 3)][0]["found"][0])
    used.close(); new.close()


# ----------------------------------------------------------------------------- 4. refusals and recovery
def test_refusals_and_recovery(ctx, mw):
    reads, ix, T, lib = mw["reads"], mw["ix"], mw["T"], ctx.lib
    want, _ = mw["resident"][(PBA_KERNEL_BITVEC, 3)]
    # create: pba_map_reads' checks, at the door
    other = ctx.seqs_from_list([mw["contigs"][0], mw["contigs"][1][:2999]], strict_acgt=True)
    other_ix = ctx.index_build_set(other, mw["mask"])
    assert status_of(ctx.map_stream, other_ix, T, R) == -1
    one_ix = ctx.index_build(T, 0, mw["mask"])
    assert status_of(ctx.map_stream, one_ix, T, R) == -1
    assert status_of(lambda: ctx.map_stream(ix, T, R, strands=0)) == -1 and status_of(lambda: ctx.map_stream(ix, T, R, strands=4)) == -1
    assert status_of(lambda: ctx.map_stream(ix, T, R, kernel=7)) == -1 and status_of(lambda: ctx.map_stream(ix, T, R, form=2)) == -1
    assert status_of(lambda: ctx.map_stream(ix, T, 1.5)) == -1
    withn = ctx.seqs_from_list([mw["contigs"][0][:700] + b"N" + mw["contigs"][0][701:1500]])
    withn_ix = ctx.index_build_set(withn, mw["mask"])
    assert status_of(ctx.map_stream, withn_ix, withn, R) == -6
    for x in (other_ix, one_ix, withn_ix, other, withn):
        x.close()
    # submit: the host checks of pba_loc_stream_submit
    st = ctx.map_stream(ix, T, R, TRIALS, MIN_LEN, slot_bytes=6000, slot_reads=4)
    assert status_of(st.collect) == -1 and status_of(st.pending) == -1          # nothing pending
    buf, offs = st.buffer()
    offs[0], offs[1] = 0, 6001
    assert status_of(st.submit, 1) == -4                                # over slot_bytes
    assert status_of(st.submit, 5) == -4                                # over slot_reads
    offs[0], offs[1], offs[2] = 0, 10, 5
    assert status_of(st.submit, 2) == -1                                # decreasing offsets
    assert status_of(st.collect) == -1 and status_of(st.pending) == -1  # the refused batches left nothing pending
    big = ctx.map_stream(ix, T, R, TRIALS, MIN_LEN, slot_bytes=70000, slot_reads=2)
    _, o = big.buffer()
    o[0], o[1] = 0, 65001
    assert status_of(big.submit, 1) == -4 and status_of(big.collect) == -1       # a read over the engine limit
    big.close()
    # cap below the batch size leaves the batch pending
    st.submit_reads(reads[0:3])
    st.submit_reads(reads[3:5])
    assert status_of(st.submit, 0) == -1 and status_of(st.buffer) == -1  # both slots pending
    raw = np.zeros(4, MAP_ROW_DTYPE)
    n = eng.C.c_uint32()
    assert lib.pba_map_stream_collect(st.h, eng._ptr(raw), 2, eng.C.byref(n), None) == -1
    r0, _ = st.collect()
    r1, _ = st.collect()
    all_cols_equal(np.concatenate([r0, r1]), want[:5])
    # a batch with a byte outside ACGT -- an N, a lower-case base; first, middle and last byte of the batch -- is dropped at
    # collect; its reads keep their ids, and the clean batch behind it continues past them
    at = 5
    for bad_byte in (b"N", b"a"):
        for where in ("first", "middle", "last"):
            trio = [bytearray(x) for x in reads[at:at + 3]]
            k, p = {"first": (0, 0), "middle": (1, len(trio[1]) // 2), "last": (2, len(trio[2]) - 1)}[where]
            trio[k][p:p + 1] = bad_byte
            st.submit_reads([bytes(x) for x in trio])
            st.submit_reads(reads[at + 3:at + 5])
            assert status_of(st.collect) == -6, (bad_byte, where)
            assert st.profile()["n_reads"] == 3
            r, s = st.collect()
            all_cols_equal(r, want[at + 3:at + 5])
            assert r["read"].tolist() == [at + 3, at + 4]
            at += 5
    assert at == 35 and sum(len(x) >= MIN_LEN for x in reads[:35]) < 35          # (a read below min_len went through: nseq != read)
    st.submit_reads([])                                                 # the stream goes on: an empty batch
    r, s = st.collect()
    assert len(r) == 0 and s["n_second_walk"] == 0 and s["strand"][0]["n_reads_kept"] == 0
    # close with two batches pending; the ctx is fine afterwards
    st.submit_reads(reads[35:38])
    st.submit_reads(reads[38:39])
    st.close()
    Rd = ctx.seqs_from_list(reads[:5], strict_acgt=True)
    again, _ = ctx.map_reads(ix, T, Rd, R, TRIALS, MIN_LEN, kernel=PBA_KERNEL_BITVEC)
    all_cols_equal(again, want[:5])
    Rd.close()


# ----------------------------------------------------------------------------- 5. one strand
def test_strands_1_holds_no_reverse_complement(ctx, mw):
    reads = mw["reads"]
    st = ctx.map_stream(mw["ix"], mw["T"], R, TRIALS, MIN_LEN, kernel=PBA_KERNEL_BITVEC, strands=1, slot_bytes=64 * 1400, slot_reads=64)
    st.submit_reads(reads[:40])
    P, Q = st.pending()
    assert Q is None and P.count == 40
    fresh = ctx.seqs_from_list(reads[:40], strict_acgt=True)
    for a, b in zip(export_bytes(P), export_bytes(fresh)):
        assert a.shape == b.shape and (a == b).all()
    fresh.close()
    rows, stats = st.collect()
    all_cols_equal(rows, mw["resident"][(PBA_KERNEL_BITVEC, 1)][0][:40])
    assert not (rows["strand"] == -1).any() and stats["strand"][1] == dict.fromkeys(STAT_KEYS, 0) and stats["n_second_walk"] == 0
    st.close()


# ----------------------------------------------------------------------------- 6. the example
def test_example_prints_the_rows(ctx, mw, tmp_path):
    out = os.path.join(ROOT, "tests", "cpp", "_build")
    os.makedirs(out, exist_ok=True)
    libdir = os.path.join(ROOT, "pacbioassembly_amd", "lib")
    exe = os.path.join(out, "map_stream_gpu")
    subprocess.run(["g++", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "examples", "map_stream_gpu.cpp"), "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}"], check=True)
    cf = tmp_path / "contigs.txt"
    cf.write_bytes(b"".join(c + b"\n" for c in mw["contigs"]))
    stdin = b"\n".join(mw["reads"]) + b"\n"
    want, _ = mw["resident"][(PBA_KERNEL_BITVEC, 3)]
    for per_batch in ("64", "7"):
        r = subprocess.run([exe, str(cf), MASK_PAT, str(R), per_batch, "3"], input=stdin, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == rows_tsv(want)
        assert r.stderr.decode().startswith(f"totally {int((want['nseq'] >= 0).sum())} sequences processed, {int(want['found'].sum())} mapped")
