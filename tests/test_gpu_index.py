"""The seed-hit index in every build regime of index_levels, against the numpy reference (tests/index_ref.py).

Device order is witnessed through pba_index_find over ALL distinct keys of the reference in one call: np.diff(hit_off)
must be the reference's per-key counts and hit_pos the reference's whole position array.  SeedIndex.dump() merges on the
host, so it is compared too but only pins the position mapping.  Every case asserts, from the reference and from the
constants parsed out of the sources, the property of its input that puts it in the regime it is named for.
Needs a real MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLD, MASK_PAT
from index_ref import define as _define, first_n_with_levels, levels_of, logp_of, np_index, runs, tile_switch as _tile_switch
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL, PbaError

pytestmark = pytest.mark.gpu

MODES = {"all": PBA_INDEX_ALL, "head_tail": PBA_INDEX_HEAD_TAIL}


# ----------------------------------------------------------------------------- the builder's constants, from its sources
PART_AVG = _define("PBA_IX_PART_AVG")
LVL_BITS = _define("PBA_IX_LVL_BITS")
MAX_LOGP = _define("PBA_IX_MAX_LOGP")
LDS_SORT_CAP = _define("PBA_IX_LDS_SORT_CAP")
SS_EPT = _define("PBA_SS_EPT")
SS_AVG = _define("PBA_SS_AVG")
SS_MAXBKT = _define("PBA_SS_MAXBKT")
TILE_SWITCH = _tile_switch()                       # n_upper <= this: tiles of 4 096 in the generic level kernels
WAVE = 64


B2, B3 = first_n_with_levels(2), first_n_with_levels(3)
SEED_MASKS = [l.strip() for l in open(f"{GOLD}/seeds.txt") if l.strip()]


def test_boundaries_follow_the_constants():
    assert logp_of(PART_AVG) == 0 and logp_of(PART_AVG + 1) == 1
    assert (levels_of(B2 - 1), levels_of(B2)) == (1, 2) and (levels_of(B3 - 1), levels_of(B3)) == (2, 3)
    assert B2 < 5_000_000 < TILE_SWITCH < B3 and LDS_SORT_CAP == 1024 * SS_EPT and len(SEED_MASKS) == 8


# ----------------------------------------------------------------------------- inputs
def rand_text(n: int, seed: int) -> bytes:
    return np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(seed).randint(0, 4, n, dtype=np.uint8)].tobytes()


def repeat_text(unit: bytes, n: int) -> bytes:
    return (unit * (n // len(unit) + 1))[:n]


def stock_mask() -> int:
    return eng.mask_from_pattern(MASK_PAT)


# ----------------------------------------------------------------------------- the check
def expected(ref, Q):
    """(hit_off, hit_pos) the reference gives for the probe keys Q, by array operations only."""
    keys, pos, _ = ref
    Q = np.asarray(Q, np.uint32)
    lo, hi = np.searchsorted(keys, Q, "left"), np.searchsorted(keys, Q, "right")
    cnt = np.where(Q == 0, 0, hi - lo).astype(np.int64)               # (zero keys are never indexed)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
    total = int(off[-1])
    idx = np.repeat(lo - off[:-1].astype(np.int64), cnt) + np.arange(total, dtype=np.int64)
    return off, pos[idx]


def compare_find(name, ref, Q, off, got, what):
    Q = np.asarray(Q, np.uint32)
    w_off, w_pos = expected(ref, Q)
    w_cnt, g_cnt = np.diff(w_off.astype(np.int64)), np.diff(off.astype(np.int64))
    assert off.size == Q.size + 1 and off[0] == 0, (name, what)
    bad = np.flatnonzero(w_cnt != g_cnt)
    if bad.size:
        q = int(bad[0])
        pytest.fail(f"{name} [{what}]: {bad.size} of {Q.size} keys with a wrong count; first: probe {q} key {int(Q[q]):#010x} "
                    f"has a run of {int(w_cnt[q])} in the reference, find returned {int(g_cnt[q])}")
    assert got.size == w_pos.size, (name, what, got.size, w_pos.size)
    bad = np.flatnonzero(got != w_pos)
    if bad.size:
        j = int(bad[0])
        q = int(np.searchsorted(w_off, j, "right")) - 1
        a, b = int(w_off[q]), int(w_off[q + 1])
        pytest.fail(f"{name} [{what}]: {bad.size} of {got.size} positions differ; first at hit {j}: probe {q} key {int(Q[q]):#010x}, "
                    f"run of {b - a} in the reference, entry {j - a} of it: reference {w_pos[a:b][:12].tolist()}..., "
                    f"find returned {got[a:b][:12].tolist()}...")
    return w_pos


def check_index(ix, ref, mask, name):
    """The whole of one built index against the reference (keys, pos, visited)."""
    keys, pos, visited = ref
    assert ix.entries == keys.size, (name, "entries", ix.entries, keys.size)
    assert ix.visited == visited, (name, "visited", ix.visited, visited)
    U, cnt = runs(keys)
    # every distinct key in one call: the counts, and the positions as the reference's whole array
    off, got = ix.find(U)
    w_pos = compare_find(name, ref, U, off, got, "all distinct keys")
    assert np.array_equal(np.diff(off.astype(np.int64)), cnt) and w_pos is not None and np.array_equal(got, pos), name
    # absent keys (random ones, the masked neighbours of present ones), 0 and all-ones, duplicates inside one call
    rng = np.random.RandomState(keys.size % 9973 + 11)
    r = rng.randint(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    Us = U if U.size <= (1 << 21) else U[np.linspace(0, U.size - 1, 1 << 21).astype(np.int64)]
    cand = np.concatenate([r, r & np.uint32(mask), (Us + np.uint32(1)) & np.uint32(mask), (Us - np.uint32(1)) & np.uint32(mask)])
    at = np.minimum(np.searchsorted(U, cand), max(U.size - 1, 0))
    absent = cand[(U[at] != cand) if U.size else np.ones(cand.size, bool)]
    off, got = ix.find(absent)
    compare_find(name, ref, absent, off, got, "absent keys")
    assert off[-1] == 0 and got.size == 0, (name, "an absent key was found")
    dup = np.zeros(0, np.uint32)
    if U.size:
        pick = U[rng.randint(0, U.size, 512)]
        c = np.diff(expected(ref, pick)[0].astype(np.int64))
        pick = pick[:max(1, int(np.searchsorted(np.cumsum(c), 2_000_000)))]          # (bounded output for very long runs)
        dup = np.concatenate([pick, U[:1], pick[::-1], U[-1:], U[:1], pick])
    Q = np.concatenate([np.array([0, 0xFFFFFFFF], np.uint32), dup, absent[:64], np.array([0xFFFFFFFF, 0], np.uint32)])
    off, got = ix.find(Q)
    compare_find(name, ref, Q, off, got, "0, all-ones, duplicates")
    # dump(): the position mapping of pba_index_dump (it sorts on the host: no witness of device order)
    k, p = ix.dump()
    assert k.size == keys.size and np.array_equal(k, keys), (name, "dump keys")
    assert np.array_equal(p, pos), (name, "dump positions")


def build_and_check(ctx, text, mask, mode, name, seqs=None, seq=0, ref=None):
    ref = ref if ref is not None else np_index(text, mask, mode)
    S = ctx.seqs_from_list(seqs if seqs is not None else [text])
    ix = ctx.index_build(S, seq, mask, MODES[mode])
    try:
        check_index(ix, ref, mask, name)
    finally:
        ix.close()
    return ref


def run_lengths(ref):
    return runs(ref[0])[1]


def largest_partition(ref, n_upper: int) -> int:
    """Entries of the fullest hash partition (ix_part: the top logP bits of key * 0x9E3779B1): what launch_seg_sort picks
    k_seg_sort<256> or k_seg_sort<1024> by."""
    lp = logp_of(n_upper)
    if lp == 0 or ref[0].size == 0:
        return int(ref[0].size)
    part = ((ref[0].astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - lp)
    return int(np.bincount(part.astype(np.int64), minlength=1 << lp).max())


# ----------------------------------------------------------------------------- sizes, ALL mode, random ACGT, stock mask
SIZES = [("n1", 1), ("n15", 15), ("n16", 16), ("n17", 17),
         ("logP0_below_avg", PART_AVG - 1), ("logP0_last", PART_AVG), ("logP1_first", PART_AVG + 1), ("logP1_last", 2 * PART_AVG + 1),
         ("one_level_last", B2 - 1), ("two_level_first", B2), ("two_level_bench_shape", 5_000_000),
         ("tile_switch_small_tiles_last", TILE_SWITCH), ("tile_switch_big_tiles_first", TILE_SWITCH + 1),
         ("three_level", B3 + 1000)]


@pytest.mark.parametrize("name,n", SIZES, ids=[s[0] for s in SIZES])
def test_sizes(ctx, name, n):
    want = {"logP0_below_avg": (0, 1), "logP0_last": (0, 1), "logP1_first": (1, 1), "logP1_last": (1, 1), "one_level_last": (LVL_BITS, 1),
            "two_level_first": (LVL_BITS + 1, 2), "three_level": (2 * LVL_BITS + 1, 3)}
    if name in want:
        assert (logp_of(n), levels_of(n)) == want[name], name
    if name.startswith("tile_switch") or name == "two_level_bench_shape":
        assert levels_of(n) == 2 and (n <= TILE_SWITCH) == (name != "tile_switch_big_tiles_first"), name   # (even levels: the index keeps the second buffer)
    ref = build_and_check(ctx, rand_text(n, n % 1000 + 1), stock_mask(), "all", f"sizes/{name}")
    if n >= 4096:
        assert run_lengths(ref).max() <= WAVE * 4               # (random text: nothing for the fallbacks; k_seg_sort alone sorts it)
        assert largest_partition(ref, n) <= 256 * SS_EPT        # ... in its 256-thread form


# ----------------------------------------------------------------------------- HEAD_TAIL
HT = [16, 17, 20015, 20016, 20017, 20036, 40015, 40016, 40017, 1_000_000]


@pytest.mark.parametrize("n", HT)
def test_head_tail(ctx, n):
    ref = build_and_check(ctx, rand_text(n, n % 1000 + 2), stock_mask(), "head_tail", f"head_tail/{n}")
    assert ref[2] == max(min(n - 16, 20000), 0) + max(min(n - 20016, 20000), 0)


def test_head_tail_key_in_head_and_tail_lists_head_first(ctx):
    n, w = 60000, b"GATTACAGATTACAGG"
    t = bytearray(rand_text(n, 77))
    at = [100, 19000, n - 16 - 5, n - 16 - 700]
    for a in at:
        t[a:a + 16] = w
    ref = np_index(bytes(t), 0xFFFFFFFF, "head_tail")
    key = (ref[0][ref[1] == 100])[0]
    assert ref[1][ref[0] == key].tolist() == at                      # head ascending, then the tail DEscending
    build_and_check(ctx, bytes(t), 0xFFFFFFFF, "head_tail", "head_tail/planted", ref=ref)
    build_and_check(ctx, bytes(t), stock_mask(), "head_tail", "head_tail/planted_stock_mask")


# ----------------------------------------------------------------------------- masks
def all_masks():
    return ([(f"seed{i}", eng.mask_from_pattern(p)) for i, p in enumerate(SEED_MASKS)] +
            [("all_ones", 0xFFFFFFFF), ("one_byte", 0x000000FF), ("two_ends", 0xC0000003), ("one_care_pair", 0x00000300), ("zero", 0)])


MASK_NAMES = [f"seed{i}" for i in range(8)] + ["all_ones", "one_byte", "two_ends", "one_care_pair", "zero"]
SPARSE = ("one_byte", "two_ends", "one_care_pair")


@pytest.mark.parametrize("size", ["one_level", "two_level"])
@pytest.mark.parametrize("mname", MASK_NAMES)
def test_masks(ctx, mname, size):
    n = {"one_level": 100_000, "two_level": B2 + 75_000}[size]
    assert levels_of(n) == (1 if size == "one_level" else 2) and logp_of(n) > 0
    mask = dict(all_masks())[mname]
    ref = build_and_check(ctx, rand_text(n, 5), mask, "all", f"masks/{mname}/{size}")
    rl = run_lengths(ref)
    if mname == "zero":
        assert ref[0].size == 0 and n > 0                     # nothing indexed while n_upper > 0
    if mname in SPARSE:
        # few distinct keys, every one a run beyond a bucket's 256: every partition that holds anything is oversize
        assert rl.size <= 255 and rl.min() > 4 * WAVE, (mname, rl.size, rl.min())
    if mname == "one_care_pair":
        assert rl.max() > LDS_SORT_CAP                        # ... and beyond one workgroup's sort as a whole


# ----------------------------------------------------------------------------- low complexity
def lowc_cases():
    return {
        # name: (text, mask, property of the reference's run lengths / entry count)
        "run_65_256_wave_sort256": (rand_text(1200, 31) + repeat_text(b"ACGGT", 500), 0xFFFFFFFF,
                                    lambda rl, n: n <= PART_AVG and WAVE < rl.max() <= 4 * WAVE),
        "run_over_256_bucket_fallback": (rand_text(3000, 32) + repeat_text(b"ACGGT", 1500), 0xFFFFFFFF,
                                         lambda rl, n: rl.max() > 4 * WAVE and n <= LDS_SORT_CAP),
        "run_over_16384_partition_fallback": (rand_text(5000, 33) + repeat_text(b"ACGGT", 100_000) + rand_text(5000, 34), stock_mask(),
                                              lambda rl, n: rl.max() > LDS_SORT_CAP),
        "homopolymer_T": (b"T" * 100_000, 0xFFFFFFFF, lambda rl, n: rl.size == 1 and rl[0] == 100_000 > LDS_SORT_CAP),
        "homopolymer_C_stock": (b"C" * 70_001, stock_mask(), lambda rl, n: rl.max() > LDS_SORT_CAP),
        "homopolymer_A_no_entries": (b"A" * 5000, 0xFFFFFFFF, lambda rl, n: rl.sum() == 15),      # only the padded tail windows
        "acggt_40000": (repeat_text(b"ACGGT", 40_000), stock_mask(),
                        lambda rl, n: 4 * WAVE < np.sort(rl)[-5] and 256 * SS_EPT < rl.max() <= LDS_SORT_CAP),
        # one partition beyond k_seg_sort<256>'s 4 096 entries makes the whole launch k_seg_sort<1024>: the partitions of the
        # random part (short runs, nothing oversize in them) are then sorted by its sixteen wavefronts
        "seg_sort_1024_one_long_run_among_random": (rand_text(60_000, 38) + b"G" * 6000 + rand_text(60_000, 39), 0xFFFFFFFF,
                                                    lambda rl, n: 256 * SS_EPT < rl.max() <= LDS_SORT_CAP and np.sort(rl)[-2] <= WAVE
                                                    and rl.size > 100_000),
        "acggt_3000000": (repeat_text(b"ACGGT", 3_000_000), stock_mask(), lambda rl, n: np.sort(rl)[-5] > LDS_SORT_CAP and levels_of(n) == 2),
        "tandem_5000_unit_20M": (repeat_text(rand_text(5000, 35), 20_000_000), stock_mask(),
                                 lambda rl, n: np.count_nonzero(rl > 4 * WAVE) >= 2000 and rl.max() <= LDS_SORT_CAP and levels_of(n) == 2),
        "ends_in_T_run_all_ones": (rand_text(3000, 36) + b"T" * 40, 0xFFFFFFFF, None),
        "ends_in_T_run_stock": (rand_text(700_000, 37) + b"T" * 300, stock_mask(), None),
    }


LOWC = ["run_65_256_wave_sort256", "run_over_256_bucket_fallback", "run_over_16384_partition_fallback", "homopolymer_T",
        "homopolymer_C_stock", "homopolymer_A_no_entries", "acggt_40000", "seg_sort_1024_one_long_run_among_random",
        "acggt_3000000", "tandem_5000_unit_20M",
        "ends_in_T_run_all_ones", "ends_in_T_run_stock"]


@pytest.mark.parametrize("name", LOWC)
def test_low_complexity(ctx, name):
    text, mask, prop = lowc_cases()[name]
    ref = np_index(text, mask, "all")
    if prop is not None:
        assert prop(run_lengths(ref), len(text)), (name, np.sort(run_lengths(ref))[-6:].tolist(), len(text))
    else:
        # the key of an all-T window is listed for real windows and for tail-padded ones alike
        p = ref[1][ref[0] == np.uint32(0xFFFFFFFF & mask)]
        assert (p <= len(text) - 16).sum() >= 20 and (p > len(text) - 16).sum() == 15, name
    if name in ("acggt_40000", "seg_sort_1024_one_long_run_among_random"):
        assert 256 * SS_EPT < largest_partition(ref, len(text)) <= LDS_SORT_CAP, name      # k_seg_sort<1024>, no partition beyond it
    build_and_check(ctx, text, mask, "all", f"low_complexity/{name}", ref=ref)


# ----------------------------------------------------------------------------- oversize-list overflow at P = 1
def compress(x: int, m: int) -> int:               # the bits of x under m, gathered (seg_bkt_key / k_seg_sort's bucket())
    r = k = 0
    for b in range(32):
        if m >> b & 1:
            r |= (x >> b & 1) << k
            k += 1
    return r


@pytest.mark.parametrize("mask", [0xFFFFFFFF, 0xC0000003], ids=["all_ones", "two_ends"])
def test_oversize_list_overflow_one_partition(ctx, mask):
    """One partition (ov_cap = 1) whose oversize buckets are sorted by different wavefronts of the workgroup: each reports
    the partition, the count passes the list's capacity, and the host has to take the 'check them all' branch.  (The
    branch is not observable through the ABI; a build in which it does nothing fails both cases here.)"""
    text = b"C" * 600 + b"G" * 600 + b"T" * 600
    ref = np_index(text, mask, "all")
    U, cnt = runs(ref[0])
    n = ref[0].size
    assert logp_of(len(text)) == 0 and min(1 << logp_of(len(text)), 4096) == 1
    assert 2 <= n <= 256 * SS_EPT                                    # k_seg_sort<256>, not reported as a whole
    threads, nbkt = 256, 1
    while nbkt < SS_MAXBKT and nbkt * SS_AVG < n:
        nbkt <<= 1
    lg, care = nbkt.bit_length() - 1, bin(mask).count("1")
    bucket = np.array([0 if lg == 0 else (compress(int(k), mask) >> (care - lg) if care > lg else compress(int(k), mask)) for k in U])
    occupancy = np.bincount(bucket, weights=cnt, minlength=nbkt)
    waves = {int(b) % (threads // WAVE) for b in np.flatnonzero(occupancy > 4 * WAVE)}
    assert len(waves) > min(1 << logp_of(len(text)), 4096), (waves, occupancy.max())   # more reports than ov_cap slots
    build_and_check(ctx, text, mask, "all", f"oversize_overflow_P1/{mask:#x}", ref=ref)


# ----------------------------------------------------------------------------- neighbours and alignment
@pytest.mark.parametrize("n", [3001, 3002, 3003, 2049 + 14, B2 + 7])
@pytest.mark.parametrize("mode", ["all", "head_tail"])
def test_middle_of_three_sequences(ctx, n, mode):
    """The indexed sequence lies between two all-A ones and ends inside a byte / a 16-base chunk: a base leaking in
    instead of the code-3 padding changes the keys of the last 15 windows."""
    assert n % 4 != 0 and n % 16 != 0
    text = rand_text(n, n % 100 + 3)
    for mask in (stock_mask(), 0xFFFFFFFF):
        build_and_check(ctx, text, mask, mode, f"middle_of_three/{n}/{mode}/{mask:#x}", seqs=[b"A" * 37, text, b"A" * 21], seq=1)


@pytest.mark.parametrize("mode", ["all", "head_tail"])
def test_bytes_outside_acgt(ctx, mode):
    text = repeat_text(b"ACGTNacgtRYKM-*", 30_011) + b"NNNNNNNNNNNNNNNNNNNN" + rand_text(20_002, 9) + b"acgtn"
    S_seqs = [b"A" * 5, text, b"A" * 19]
    for mask in (stock_mask(), 0xFFFFFFFF, 0x000000FF):
        build_and_check(ctx, text, mask, mode, f"non_acgt/{mode}/{mask:#x}", seqs=S_seqs, seq=1)


# ----------------------------------------------------------------------------- the exchange form
def from_entries(ctx, text, mask, mode, nparts, cap=None):
    """(index built by pba_index_from_entries from nparts scanned slices in a buffer pre-filled with all-ones, slots, the buffer)."""
    import torch
    S = ctx.seqs_from_list([text])
    cap = len(text) // nparts + 64 if cap is None else cap
    buf = torch.full((nparts * cap,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    total = 0
    for part in range(nparts):
        total += ctx.index_scan(S, 0, mask, MODES[mode], part, nparts, buf[part * cap:(part + 1) * cap].data_ptr(), cap)
    torch.cuda.synchronize()
    return ctx.index_from_entries(buf.data_ptr(), nparts * cap, mask, MODES[mode], len(text)), nparts * cap, total, buf


EXCHANGE = [("both_one_level", B2 - 600, "all"), ("slots_two_level_entries_one_level", B2 - 100, "all"),
            ("both_two_level", B2 + 4000, "all"), ("two_level_head_tail", B2 + 4000, "head_tail"),
            ("logP0", 1500, "all"), ("head_tail_50000", 50_000, "head_tail")]


@pytest.mark.parametrize("nparts", [1, 2, 3, 7, 8])
@pytest.mark.parametrize("name,n,mode", EXCHANGE, ids=[e[0] for e in EXCHANGE])
def test_exchange_form(ctx, name, n, mode, nparts):
    text, mask = rand_text(n, 41), stock_mask()
    ref = np_index(text, mask, mode)
    ix, slots, total, buf = from_entries(ctx, text, mask, mode, nparts)
    try:
        assert total == ref[0].size and slots == nparts * (n // nparts + 64) and slots > total       # padding counts in n_upper
        if name == "both_one_level":
            assert levels_of(slots) == 1 and levels_of(total) == 1 and B2 - slots < 600
        if name == "slots_two_level_entries_one_level":
            # the slot count decides: beyond the boundary for every nparts but 1, while the entries stay below it
            assert levels_of(total) == 1 and levels_of(n) == 1 and levels_of(slots) == (1 if nparts == 1 else 2), (slots, B2)
        if name in ("both_two_level", "two_level_head_tail"):
            assert levels_of(slots) == 2 and (mode == "all" or levels_of(total) == 1)
        check_index(ix, ref, mask, f"exchange/{name}/{nparts}")
    finally:
        ix.close()
        del buf


def test_exchange_slice_buffer_one_slot_too_small(ctx):
    import torch
    text, mask = rand_text(30_000, 42), stock_mask()
    n = np_index(text, mask, "all")[0].size
    S = ctx.seqs_from_list([text])
    buf = torch.full((n + 8,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(PbaError) as e:
        ctx.index_scan(S, 0, mask, PBA_INDEX_ALL, 0, 1, buf.data_ptr(), n - 1)
    assert e.value.status == -1                                       # PBA_E_INVALID; the buffer is not read afterwards
    assert ctx.index_scan(S, 0, mask, PBA_INDEX_ALL, 0, 1, buf.data_ptr(), n) == n


# ----------------------------------------------------------------------------- the ctx's one-deep cache of index arrays
def test_cache_reuse_sequence(ctx):
    """Build / destroy in an order that hands a small index the stale buffers of a large one (and a two-level build the
    buffers of a one-level one), then the same order with the previous index still alive (the cache empty)."""
    m1, m2 = stock_mask(), eng.mask_from_pattern(SEED_MASKS[3])
    steps = [("two_level_5M", 5_000_000, m1, "all", False), ("one_level_3000", 3000, m2, "all", False), ("logP0_1500", 1500, m1, "all", False),
             ("two_level_from_entries", B2 + 9000, m1, "all", True), ("head_tail_50000", 50_000, m2, "head_tail", False),
             ("one_level_100000", 100_000, m1, "all", False), ("two_level_5M_again", 5_000_000, m1, "all", False)]
    assert [levels_of(s[1]) for s in steps[:4]] == [2, 1, 1, 2] and logp_of(1500) == 0 < logp_of(3000)
    made = {}

    def make(step):
        name, n, mask, mode, exch = step
        if (n, mask, mode) not in made:
            text = rand_text(n, 51)
            made[(n, mask, mode)] = (text, np_index(text, mask, mode))
        text, ref = made[(n, mask, mode)]
        if exch:
            ix, _, _, buf = from_entries(ctx, text, mask, mode, 3)
            del buf
        else:
            ix = ctx.index_build(ctx.seqs_from_list([text]), 0, mask, MODES[mode])
        return ix, ref, mask

    for step in steps:                                               # each index destroyed before the next build
        ix, ref, mask = make(step)
        try:
            check_index(ix, ref, mask, f"cache/serial/{step[0]}")
        finally:
            ix.close()
    prev = None
    for step in steps:                                               # two alive at once: the second finds the cache empty
        ix, ref, mask = make(step)
        try:
            check_index(ix, ref, mask, f"cache/overlapped/{step[0]}")
            if prev is not None:
                check_index(prev[0], prev[1], prev[2], f"cache/overlapped/previous_of_{step[0]}")
        except BaseException:
            ix.close()                                               # (a failing check leaves neither index open)
            raise
        finally:
            if prev is not None:
                prev[0].close()
        prev = (ix, ref, mask)
    prev[0].close()


# ----------------------------------------------------------------------------- find itself
@pytest.fixture(scope="module")
def built(ctx):
    text, mask = rand_text(5_000_000, 61), stock_mask()
    ref = np_index(text, mask, "all")
    ix = ctx.index_build(ctx.seqs_from_list([text]), 0, mask, PBA_INDEX_ALL)
    yield ix, ref
    ix.close()


def raw_find(ctx, ix, Q, pos_buf, cap):
    Q = np.ascontiguousarray(Q, np.uint32)
    off = np.full(Q.size + 1, 0xDEADBEEFDEADBEEF, np.uint64)
    kp = Q.ctypes.data_as(C.c_void_p) if Q.size else None
    pp = pos_buf.ctypes.data_as(C.c_void_p) if pos_buf is not None else None
    st = ctx.lib.pba_index_find(ctx.h, ix.h, kp, Q.size, off.ctypes.data_as(C.c_void_p), pp, cap)
    assert st == 0, st
    return off


def test_find_no_keys(ctx, built):
    ix, ref = built
    assert raw_find(ctx, ix, np.zeros(0, np.uint32), None, 0).tolist() == [0]
    off, pos = ix.find(np.zeros(0, np.uint32))
    assert off.tolist() == [0] and pos.size == 0


def test_find_counts_only_and_short_hit_buffer(ctx, built):
    ix, ref = built
    U, cnt = runs(ref[0])
    Q = U[::1000][:3000]
    w_off, w_pos = expected(ref, Q)
    assert np.array_equal(raw_find(ctx, ix, Q, None, 0), w_off)                       # hit_pos = NULL: the counts alone
    GUARD = np.int32(-0x5A5A5A5B)
    for cap in (0, 1, int(w_off[7]) + 1, w_pos.size // 2, w_pos.size - 1, w_pos.size):
        buf = np.full(w_pos.size + 64, GUARD, np.int32)
        off = raw_find(ctx, ix, Q, buf, cap)
        assert np.array_equal(off, w_off), cap                        # complete whatever the capacity
        assert np.array_equal(buf[:cap], w_pos[:cap]), cap
        assert (buf[cap:] == GUARD).all(), (cap, "written beyond hit_cap")


@pytest.mark.parametrize("nk", [1, 255, 256, 257, 3_000_000])
def test_find_block_edges_and_many_keys(ctx, built, nk):
    ix, ref = built
    U, _ = runs(ref[0])
    rng = np.random.RandomState(nk % 1000)
    Q = U[rng.randint(0, U.size, nk)]
    miss = rng.rand(nk) < 0.25
    Q[miss] = rng.randint(0, 2 ** 32, int(miss.sum()), dtype=np.uint64).astype(np.uint32)     # (mostly absent: non-care bits set)
    if nk > 1:
        Q[-1] = U[-1]                                                 # the launch's last thread has a present key
    off, pos = ix.find(Q)
    compare_find(f"find/{nk}_keys", ref, Q, off, pos, "mixed probe")


def test_find_long_run_ends_at_partition_end(ctx):
    """ix_run_end gallops: a run of thousands, and one partition that is a single run (its end is the partition's)."""
    text = b"T" * 9000
    ref = np_index(text, 0xFFFFFFFF, "all")
    assert runs(ref[0])[1].tolist() == [9000] and logp_of(9000) > 0      # one key: its partition IS the run, the others are empty
    build_and_check(ctx, text, 0xFFFFFFFF, "all", "find/run_is_the_partition", ref=ref)
    text = rand_text(40_000, 71) + b"G" * 4111 + rand_text(40_000, 72)
    ref = np_index(text, 0xFFFFFFFF, "all")
    assert run_lengths(ref).max() >= 4111 - 15
    build_and_check(ctx, text, 0xFFFFFFFF, "all", "find/long_run_inside_a_partition", ref=ref)
