"""Every entry point held to its reference with the ctx on a stream the caller owns (pba_ctx_set_stream; include/pba.h:
"Streams") -- with work of the caller's still PENDING on that stream when the call is made, which
no other test arranges: everywhere else the inputs come from host memory or are synchronised, and the queues are idle.

The delay is torch.cuda._sleep on the caller's stream (a loop of add_ on a large tensor where torch has none), calibrated once
per module with events on a stream: make_sleep.  Two lengths, both measured (DESIGN §3.3 has the figures):
  D_LONG_MS   in front of the producer of a hand-off: at least ten times the longest host time, call to return, of any hand-off
              entry point at these shapes on idle queues -- the producer is still pending when the entry point issues its first
              device step, and Hand.call asserts that it was pending when the call was made
  D_SHORT_MS  in front of every library call of parts b and c: as long as the whole of part b stays within about twice its cost
              without a delay

a. Hand-offs, one test per entry of caller_stream_inputs.HANDOFFS (every entry point that takes a device pointer).  The buffer
   holds a poison and is synchronised; then the delay and the producer are queued on the stream -- the copy of the real input
   for an entry point that reads the buffer, the caller's own fill for one that writes it -- and the entry point is called at
   once.  The result must be what the same steps give synchronised on the ctx's own stream (the same function run through
   Hand(None)), and what the plain references say: the texts, the host codec's bytes, pba_index_build's dump, the probe model,
   pba_overlap_all's rows and the model's, census_ref.  The poison is a valid input with another answer.  There is no negative
   control on the ctx's own stream: it would be a race run on purpose.
b. Every case of stale_cases.CASES, fresh state, the ctx and torch on a caller's stream, D_SHORT_MS queued on it in front of
   every pba_* call (DelayedLib).  The case's own checker holds it to its own reference.
c. pba_loc_stream and pba_map_stream created, fed and destroyed on a caller's stream behind the same delays, three batches
   through two slots; and the stream recorded at create: submit / pending / collect with the ctx on another stream are refused
   and leave the object usable, destroy is legal anywhere.

What b and c can see: a step enqueued on a stream other than the ctx's -- its own, the legacy default stream, a copy stream
without its event.  Such a step no longer waits for the steps before it, which sit behind the delay, and reads what they have not
written yet.  What they cannot see: a stray PRODUCER, which merely finishes early (a memset moved to another stream still lands
before the kernel that needs it); and anything from the first implicit device-wide synchronise inside a call onwards -- a hipFree
in a DevBuf's destructor is one -- since behind it the stream is idle again.  That is why the delay stands in front of every
call and not once per case.  Needs a real MI355X (-m gpu)."""
import functools
import time

import numpy as np
import pytest

import caller_stream_inputs as ci
import census_ref as cr
import overlap_edge_inputs as oi
import overlap_ref as orf
import stale_cases as sc
from caller_stream_inputs import delayed_lib, on_stream
from conftest import MASK_PAT
from map_stream_inputs import MIN_LEN as MAP_MIN_LEN, R as MAP_R, TRIALS as MAP_TRIALS
from pacbioassembly_amd import ProbeTable
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL, PBA_KERNEL_BITVEC, PbaError
from seqs_edge_inputs import host_packed
from test_gpu_map_stream import all_cols_equal, mw, sum_stats  # noqa: F401  (mw: the mapper's world, as a fixture of this module too)
from test_gpu_stream import MIN_LEN, R, TRIALS, rows_equal, run_pipelined, world  # noqa: F401  (world: likewise)

pytestmark = pytest.mark.gpu

D_LONG_MS = 20.0                   # 39 x the longest hand-off call measured (pba_overlap_all_probes, 0.51 ms): DESIGN §3.3
D_SHORT_MS = 0.4                   # 1 128 library calls in part b: 0.45 s of delay beside 0.42 - 0.45 s of cases (measured: 0.89 s)
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


# ----------------------------------------------------------------------------- the delay
def make_sleep():
    """sleep(stream, ms): about `ms` milliseconds of nothing queued on `stream`, sized by a measurement on this device (events
    around a delay of known size, doubled until it lasts 5 ms) and by no clock-rate constant"""
    import torch
    s = torch.cuda.Stream()
    if hasattr(torch.cuda, "_sleep"):
        def unit(n):
            torch.cuda._sleep(int(n))
        n = 1 << 20
    else:
        big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")

        def unit(n):
            for _ in range(int(n)):
                big.add_(1.0)
        n = 4

    def measure(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            unit(n)
            e1.record()
        s.synchronize()
        return e0.elapsed_time(e1)
    measure(n)                                                    # (the first launch pays for loading the kernel)
    ms = measure(n)
    while ms < 5.0 and n < 1 << 40:
        n *= 2
        ms = measure(n)
    per_ms = n / ms
    print(f"delay: {n} units took {ms:.3f} ms -> {per_ms:.1f} units per ms")

    def sleep(stream, want_ms):
        with torch.cuda.stream(stream):
            unit(max(1, round(want_ms * per_ms)))
    sleep.per_ms = per_ms
    return sleep


@pytest.fixture(scope="module")
def sleep(ctx):
    return make_sleep()


class Hand:
    """How a hand-off function queues its producer and makes its call.  Hand(None): the producer on torch's current stream,
    synchronised before the call -- the reference.  Hand(sleep, stream): D_LONG_MS and then the producer queued on `stream`, the
    call made at once; the producer must still be pending at that moment, or the run has shown nothing."""

    def __init__(self, sleep=None, stream=None, d_long=None):
        self.sleep, self.stream, self.times = sleep, stream, []
        self.d_long = D_LONG_MS if d_long is None else d_long
        self.done = None

    def produce(self, fn):
        import torch
        if self.sleep is None:
            fn()
            torch.cuda.synchronize()
            return
        self.sleep(self.stream, self.d_long)
        with torch.cuda.stream(self.stream):
            fn()
            self.done = torch.cuda.Event()
            self.done.record()

    def call(self, fn, *args, **kw):
        if self.done is not None:
            assert not self.done.query(), "the producer had finished before the call was made: enlarge D_LONG_MS"
            self.done = None
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        self.times.append((getattr(fn, "__name__", type(fn).__name__), (time.perf_counter() - t0) * 1e3))
        return out


def dev(a):
    """a host array on the device (u64 as the i64 of the same bits: torch's own dtype for it); the caller synchronises"""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.copy()).cuda()


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


# ----------------------------------------------------------------------------- a. the inputs of the hand-offs
@functools.lru_cache(maxsize=None)
def seq_texts():
    rng = np.random.RandomState(515)
    return [np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, n)].tobytes() for n in ci.SEQ_LENGTHS]


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)


PACKED_OFFS = np.array([0, 0, 16, 32, 48], np.uint64)             # a 16-byte granule for every sequence that has a base
PACKED_BYTES = 64


@functools.lru_cache(maxsize=None)
def index_text():
    rng = np.random.RandomState(2000)
    return np.frombuffer(b"ACGT", np.uint8)[rng.randint(0, 4, ci.INDEX_TEXT_LEN)].tobytes()


INDEX_MODES = (PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL)
INDEX_CAP = ci.INDEX_TEXT_LEN // ci.INDEX_PARTS + 64
OVL_CASE = sc.OVL_CASE                                            # the smallest set of overlap_edge_inputs: twelve reads of 300 bases
MASK_LO, MASK_HI, MASK_GUARD = 7, 19, 64                          # the smallest non-empty shard of test_gpu_census.test_mask_probes


def index_mask():
    return eng.mask_from_pattern(MASK_PAT)


def ovl_params():
    S, Rr, pat, mt, om = oi.case_params(OVL_CASE)
    return S.texts, Rr, orf.mask_of(pat), mt, om


@functools.lru_cache(maxsize=None)
def census_inputs():
    texts, _ = cr.planted_reads()
    P, mask = cr.PLANTED, cr.MASKS["w12"]
    want = cr.census(texts, mask, "head_tail")
    entries = orf.probe_entries(texts, mask, P["max_trial"], MASK_LO, MASK_HI)
    left, n_masked = cr.masked_entries(entries, want, P["max_occ"])
    slots = np.full((MASK_HI - MASK_LO) * 2 * P["max_trial"] + MASK_GUARD, ALL_ONES, np.uint64)
    slots[:entries.size] = entries
    return texts, mask, slots, left, n_masked


# ----------------------------------------------------------------------------- a. the hand-offs: (ctx, Hand, ...) -> what came out
def hand_seqs_from_device_text(ctx, h):
    import torch
    texts = seq_texts()
    text = np.frombuffer(b"".join(texts), np.uint8)
    stage_t, stage_o = dev(text), dev(offsets_of(ci.SEQ_LENGTHS))
    d_text, d_offs = dev(np.full(text.size, ord("A"), np.uint8)), dev(offsets_of(ci.RESPLIT_LENGTHS))
    torch.cuda.synchronize()
    h.produce(lambda: (d_text.copy_(stage_t), d_offs.copy_(stage_o)))
    S = h.call(ctx.seqs_from_device_text, d_text.data_ptr(), d_offs.data_ptr(), len(texts), text.size, max(ci.SEQ_LENGTHS))
    out = S.lengths().tolist(), [S.get_text(i) for i in range(S.count)]
    S.close()
    return out


def hand_seqs_export(ctx, h):
    import torch
    S = ctx.seqs_from_list(seq_texts(), strict_acgt=True)
    cap = int(S.packed_bytes) + 32
    dst = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.produce(lambda: dst.fill_(0xFF))
    offs = h.call(S.export, dst.data_ptr(), cap)
    out = int(S.packed_bytes), offs.tolist(), dst.cpu().numpy().tobytes()
    S.close()
    return out


def hand_seqs_from_device_packed(ctx, h):
    import torch
    texts = seq_texts()
    stage = dev(host_packed(texts, PACKED_OFFS))
    assert stage.numel() == PACKED_BYTES
    buf = torch.zeros(PACKED_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    h.produce(lambda: buf.copy_(stage))
    S = h.call(ctx.seqs_from_device_packed, buf.data_ptr(), PACKED_BYTES, PACKED_OFFS, np.array(ci.SEQ_LENGTHS, np.uint32))
    out = S.lengths().tolist(), [S.get_text(i) for i in range(S.count)]
    S.close()
    return out


def hand_index_scan(ctx, h, mode):
    """(entries counted, the gathered buffer as the host sees it: INDEX_PARTS slices of INDEX_CAP slots)"""
    import torch
    S = ctx.seqs_from_list([index_text()])
    allent = torch.zeros(ci.INDEX_PARTS * INDEX_CAP, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    total = 0
    for part in range(ci.INDEX_PARTS):
        sl = allent[part * INDEX_CAP:(part + 1) * INDEX_CAP]
        h.produce(lambda: sl.fill_(-1))
        total += h.call(ctx.index_scan, S, 0, index_mask(), mode, part, ci.INDEX_PARTS, sl.data_ptr(), INDEX_CAP)
    out = total, host_u64(allent).copy()
    S.close()
    return out


def dump_of(ix, mode):
    """(keys, positions, entries, and what test_index_scan_gather_build_equals_direct_build compares of a head / tail index)"""
    k, p = ix.dump()
    return k.tolist(), p.tolist(), int(ix.entries), int(ix.visited) if mode == PBA_INDEX_HEAD_TAIL else None


def hand_index_from_entries(ctx, h, mode, gathered):
    import torch
    stage = dev(gathered)
    buf = torch.full((gathered.size,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h.produce(lambda: buf.copy_(stage))
    ix = h.call(ctx.index_from_entries, buf.data_ptr(), buf.numel(), index_mask(), mode, ci.INDEX_TEXT_LEN)
    out = dump_of(ix, mode)
    ix.close()
    return out


def hand_overlap_probes(ctx, h):
    """(entries counted, the buffer as the host sees it: n * 2 max_trial slots and a guard of eight)"""
    import torch
    texts, _, mask, mt, _ = ovl_params()
    D = ctx.seqs_from_list(texts, strict_acgt=True)
    cap = len(texts) * 2 * mt
    buf = torch.zeros(cap + 8, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h.produce(lambda: buf.fill_(-1))
    cnt = h.call(ctx.overlap_probes, D, 0, len(texts), mask, mt, buf.data_ptr(), cap)
    out = cnt, host_u64(buf).copy()
    D.close()
    return out


def pending_probes(h, slots):
    """a device buffer of all-ones with the copy of `slots` over it pending"""
    import torch
    stage = dev(slots)
    buf = torch.full((slots.size,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    h.produce(lambda: buf.copy_(stage))
    return buf


STAT_KEYS = ("n_probe_entries", "n_candidates", "n_pairs", "n_overlaps")


def hand_overlap_all_probes(ctx, h, slots):
    texts, Rr, mask, mt, om = ovl_params()
    D = ctx.seqs_from_list(texts, strict_acgt=True)
    buf = pending_probes(h, slots)
    got, st = h.call(ctx.overlap_all_probes, D, buf.data_ptr(), buf.numel(), mask, Rr, mt, om, kernel=PBA_KERNEL_BITVEC)
    D.close()
    return got, st


def hand_probe_table_create(ctx, h, slots):
    texts, Rr, mask, mt, om = ovl_params()
    D = ctx.seqs_from_list(texts, strict_acgt=True)
    buf = pending_probes(h, slots)
    table = h.call(ProbeTable, ctx, buf.data_ptr(), buf.numel(), mask, mt)
    entries = int(table.entries)
    got, st = ctx.overlap_all_table(D, table, Rr, om, kernel=PBA_KERNEL_BITVEC)
    table.close()
    D.close()
    return entries, got, st


def hand_census_mask_probes(ctx, h):
    texts, mask, slots, _, _ = census_inputs()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    cen = ctx.census(S, mask)
    buf = pending_probes(h, slots)
    n_masked = h.call(cen.mask_probes, buf.data_ptr(), buf.numel(), cr.PLANTED["max_occ"])
    out = n_masked, host_u64(buf).copy()
    cen.close()
    S.close()
    return out


def both_ways(ctx, sleep, fn, *args):
    """(what fn gives synchronised on the ctx's own stream, what it gives on a caller's stream with its producer pending)"""
    import torch
    want = fn(ctx, Hand(None), *args)
    s = torch.cuda.Stream()
    with on_stream(ctx, s), torch.cuda.stream(s):
        h = Hand(sleep, s)
        got = fn(ctx, h, *args)
    print(fn.__name__, [(n, round(ms, 3)) for n, ms in h.times])
    return want, got


def sorted_slices(buf, width):
    return np.sort(buf.reshape(-1, width), axis=1)


def same_overlaps(got, want):
    from test_gpu_overlap_edges import rows_of
    assert rows_of(got[0]) == rows_of(want[0]) and {k: got[1][k] for k in STAT_KEYS} == {k: want[1][k] for k in STAT_KEYS}


@pytest.mark.parametrize("name", sorted(ci.HANDOFFS))
def test_handoff_with_the_producer_still_pending(ctx, oracle, sleep, name):
    globals()["check_" + name](ctx, oracle, sleep)


def check_pba_seqs_from_device_text(ctx, oracle, sleep):
    want, got = both_ways(ctx, sleep, hand_seqs_from_device_text)
    host = ctx.seqs_from_list(seq_texts())                            # the host path, as test_seqs_from_device_text_matches_host_path
    assert want == (list(ci.SEQ_LENGTHS), [host.get_text(i) for i in range(host.count)]) == (list(ci.SEQ_LENGTHS), seq_texts())
    assert got == want


def check_pba_seqs_export(ctx, oracle, sleep):
    want, got = both_ways(ctx, sleep, hand_seqs_export)
    pk, offs, image = want
    codec = host_packed(seq_texts(), offs)
    assert codec.size == pk and image[:pk] == codec.tobytes() and image[pk:] == b"\xff" * 32      # the caller's fill behind the arena
    assert got == want


def check_pba_seqs_from_device_packed(ctx, oracle, sleep):
    want, got = both_ways(ctx, sleep, hand_seqs_from_device_packed)
    assert want == (list(ci.SEQ_LENGTHS), seq_texts())
    assert got == want


def direct_index(ctx, mode):
    S = ctx.seqs_from_list([index_text()])
    ix = ctx.index_build(S, 0, index_mask(), mode)
    out = dump_of(ix, mode)
    ix.close()
    S.close()
    return out


def check_pba_index_scan(ctx, oracle, sleep):
    for mode in INDEX_MODES:
        (wn, wbuf), (gn, gbuf) = both_ways(ctx, sleep, hand_index_scan, mode)
        direct = direct_index(ctx, mode)
        assert wn == direct[2] == int((wbuf != ALL_ONES).sum()) and wn > ci.INDEX_TEXT_LEN // 2, mode
        assert hand_index_from_entries(ctx, Hand(None), mode, wbuf) == direct, mode      # the reference run is a scan of this index
        assert gn == wn and (sorted_slices(gbuf, INDEX_CAP) == sorted_slices(wbuf, INDEX_CAP)).all(), mode


def check_pba_index_from_entries(ctx, oracle, sleep):
    for mode in INDEX_MODES:
        _, gathered = hand_index_scan(ctx, Hand(None), mode)
        want, got = both_ways(ctx, sleep, hand_index_from_entries, mode, gathered)
        assert want == direct_index(ctx, mode) and want[2] > ci.INDEX_TEXT_LEN // 2, mode
        assert got == want, mode


def check_pba_overlap_probes(ctx, oracle, sleep):
    texts, _, mask, mt, _ = ovl_params()
    (wn, wbuf), (gn, gbuf) = both_ways(ctx, sleep, hand_overlap_probes)
    model = orf.probe_entries(texts, mask, mt)
    assert wn == model.size > 0 and (np.sort(wbuf[:wn]) == model).all() and (wbuf[wn:] == ALL_ONES).all()
    assert gn == wn and (np.sort(gbuf[:gn]) == model).all() and (gbuf[gn:] == ALL_ONES).all()


def probe_slots(ctx):
    _, slots = hand_overlap_probes(ctx, Hand(None))
    return slots


def whole_overlap(ctx, oracle):
    """pba_overlap_all on the same set, held to the model"""
    from test_gpu_overlap_edges import check
    texts, Rr, mask, mt, om = ovl_params()
    W = oi.expected(oracle, OVL_CASE)
    D = ctx.seqs_from_list(texts, strict_acgt=True)
    got, st = ctx.overlap_all(D, mask, Rr, mt, om, kernel=PBA_KERNEL_BITVEC)
    D.close()
    check(got, st, W, PBA_KERNEL_BITVEC, "caller stream short")
    assert len(got) >= 10
    return got, st


def check_pba_overlap_all_probes(ctx, oracle, sleep):
    whole = whole_overlap(ctx, oracle)
    want, got = both_ways(ctx, sleep, hand_overlap_all_probes, probe_slots(ctx))
    same_overlaps(want, whole)
    same_overlaps(got, whole)


def check_pba_probe_table_create(ctx, oracle, sleep):
    whole = whole_overlap(ctx, oracle)
    want, got = both_ways(ctx, sleep, hand_probe_table_create, probe_slots(ctx))
    assert want[0] == got[0] == whole[1]["n_probe_entries"] > 0
    same_overlaps(want[1:], whole)
    same_overlaps(got[1:], whole)


def check_pba_census_mask_probes(ctx, oracle, sleep):
    _, _, slots, left, n_masked = census_inputs()
    assert 0 < n_masked < left.size                                   # (the poison's answer is 0 masked and nothing left)
    for n, buf in both_ways(ctx, sleep, hand_census_mask_probes):
        assert n == n_masked and (np.sort(buf[buf != ALL_ONES]) == left).all() and buf.size == slots.size


# ----------------------------------------------------------------------------- b. every family behind a busy stream
@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_entry_points_behind_a_busy_stream(ctx, oracle, sleep, case):
    import torch
    ctx.trim()
    s = torch.cuda.Stream()
    with on_stream(ctx, s), torch.cuda.stream(s), delayed_lib(ctx, lambda: sleep(s, D_SHORT_MS)):
        case.run(ctx, oracle)
    ctx.trim()


# ----------------------------------------------------------------------------- c. the streaming objects
BATCHES = (37, 1, 64)                                                 # three batches through two slots: the first slot is used twice


def three_batches(reads):
    at, out = 0, []
    for n in BATCHES:
        out.append(reads[at:at + n])
        at += n
    return out


def test_loc_stream_on_a_caller_owned_stream(ctx, world, sleep):
    import torch
    s = torch.cuda.Stream()
    with on_stream(ctx, s), torch.cuda.stream(s), delayed_lib(ctx, lambda: sleep(s, D_SHORT_MS)):
        st = ctx.locate_stream(world["ix"], world["T"], 0, R, TRIALS, MIN_LEN, kernel=PBA_KERNEL_BITVEC, slot_bytes=64 * 1400, slot_reads=64)
        rows, _ = run_pipelined(st, three_batches(world["reads"]))
        st.close()
    want, _ = world["resident"][PBA_KERNEL_BITVEC]
    got = np.concatenate(rows)
    assert [len(r) for r in rows] == list(BATCHES)
    rows_equal(got, want[:sum(BATCHES)])
    assert int(got["found"].sum()) > 40


def test_map_stream_on_a_caller_owned_stream(ctx, mw, sleep):
    import torch
    s = torch.cuda.Stream()
    with on_stream(ctx, s), torch.cuda.stream(s), delayed_lib(ctx, lambda: sleep(s, D_SHORT_MS)):
        st = ctx.map_stream(mw["ix"], mw["T"], MAP_R, MAP_TRIALS, MAP_MIN_LEN, kernel=PBA_KERNEL_BITVEC, strands=3, slot_bytes=64 * 1400,
                            slot_reads=64)
        rows, stats = run_pipelined(st, three_batches(mw["reads"]))
        st.close()
    want, _ = mw["resident"][(PBA_KERNEL_BITVEC, 3)]
    got = np.concatenate(rows)
    assert [len(r) for r in rows] == list(BATCHES)
    all_cols_equal(got, want[:sum(BATCHES)])
    assert int(got["found"].sum()) > 40 and sum_stats(stats)["n_second_walk"] > 0 and set(got["strand"][got["found"] == 1].tolist()) == {1, -1}


def refused(fn, *args):
    """a call refused with PBA_E_INVALID for the stream it is made on"""
    with pytest.raises(PbaError) as e:
        fn(*args)
    assert e.value.status == -1 and "another stream" in str(e.value), e.value


@pytest.mark.parametrize("kind", ("loc", "map"))
def test_stream_object_holds_the_stream_it_was_made_on(ctx, request, kind):
    """created on stream A: with the ctx on B, submit, pending and collect return PBA_E_INVALID, enqueue nothing and leave the
    object usable -- free or with a batch pending; back on A the batch goes through with the resident rows; destroy with the ctx
    on B and a batch pending returns, and the ctx works afterwards"""
    import torch
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    w = request.getfixturevalue("world" if kind == "loc" else "mw")
    reads = w["reads"]
    try:
        ctx.set_stream(A.cuda_stream)
        if kind == "loc":
            st = ctx.locate_stream(w["ix"], w["T"], 0, R, TRIALS, MIN_LEN, kernel=PBA_KERNEL_BITVEC, slot_bytes=64 * 1400, slot_reads=64)
            want, same = w["resident"][PBA_KERNEL_BITVEC][0], rows_equal
        else:
            st = ctx.map_stream(w["ix"], w["T"], MAP_R, MAP_TRIALS, MAP_MIN_LEN, kernel=PBA_KERNEL_BITVEC, strands=3, slot_bytes=64 * 1400,
                                slot_reads=64)
            want, same = w["resident"][(PBA_KERNEL_BITVEC, 3)][0], all_cols_equal
        ctx.set_stream(B.cuda_stream)
        refused(st.submit_reads, reads[:37])
        ctx.set_stream(A.cuda_stream)
        with pytest.raises(PbaError) as e:                            # the refused submit left nothing pending
            st.collect()
        assert e.value.status == -1
        st.submit_reads(reads[:37])
        ctx.set_stream(B.cuda_stream)
        refused(st.collect)
        refused(st.pending)
        ctx.set_stream(None)                                          # (the ctx's own stream is another stream too)
        refused(st.collect)
        ctx.set_stream(A.cuda_stream)
        rows, _ = st.collect()                                        # ... and the batch was still pending
        same(rows, want[:37])
        st.submit_reads(reads[37:38])
        ctx.set_stream(B.cuda_stream)
        st.close()
        if kind == "loc":
            Rd = ctx.seqs_from_list(reads[:5], strict_acgt=True)
            again, _ = ctx.locate(w["ix"], w["T"], 0, Rd, R, TRIALS, MIN_LEN, kernel=PBA_KERNEL_BITVEC)
        else:
            Rd = ctx.seqs_from_list(reads[:5], strict_acgt=True)
            again, _ = ctx.map_reads(w["ix"], w["T"], Rd, MAP_R, MAP_TRIALS, MAP_MIN_LEN, kernel=PBA_KERNEL_BITVEC, strands=3)
        same(again, want[:5])
        Rd.close()
    finally:
        ctx.set_stream(None)
