"""csrc/index_plan.h alone -- what host and device agree on about a seed index before anything is launched -- as a stand-alone
host program (tests/cpp/index_plan_main.cpp, under ASan + UBSan where the compiler has the runtimes): the one statement of the
visiting rule (visit_rule: head, tail, ord_of / pos_of, the chunk numbering of its segments) and visit_plan over it against
index_ref.visit_order and its closed forms, at every length 0 .. 40 100 in both modes; ix_compress(x, compress_masks(mask)) against a
bit-by-bit gather; index_plan (compiled with seed_index.h's regime constants) against the regime rules restated in index_ref.py
and the sizes the build has always reserved in its two pooled arenas.  No GPU, nothing loaded into python."""
import os
import subprocess

import numpy as np
import pytest

from conftest import HERE, ROOT
from index_ref import (LVL_BITS, MAX_LOGP, MAX_READ_LEN, N_SEQ_WORD, PART_AVG, define, first_n_with_levels, levels_of, logp_of, tile_switch,
                       visit_order)
from overlap_ref import mask_of

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"]
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 20000, 20015, 20016, 20017, 20031, 20032, 40015, 40016, 40017, 100000]
MODES = {"all": 0, "head_tail": 1}                 # PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL (include/pba.h)
RULE_MAX = 40100                                   # the rule at EVERY length up to here: past the last length at which it changes (40 016)
ORD_LENS = LENS + [40100, 65535]
HUGE = (1 << 31) - 17, (1 << 31) + 20100           # ... and around 2^31, where len - 16 leaves the signed arithmetic the rule is written in
SEED_MASKS = [mask_of(ln.strip()) for ln in open(os.path.join(HERE, "golden", "seeds.txt")) if ln.strip()]
COMPRESS_MASKS = SEED_MASKS + [1, 0x80000000, 0xFFFFFFFF] + np.random.default_rng(11).integers(1, 1 << 32, 300, dtype=np.uint64).tolist()
SCAN_TILE = define("PBA_SCAN_TILE", "seed_index.h")
B2, B3 = first_n_with_levels(2), first_n_with_levels(3)
TILE_SWITCH = tile_switch()                        # (the tile is the builder's choice, not the plan's: its switch is a size like the others here)
N_UPPER = [0, 1, PART_AVG - 1, PART_AVG, PART_AVG + 1, B2 - 1, B2, 5_000_000, TILE_SWITCH, TILE_SWITCH + 1, B3 - 1, B3, 0xFFFFFFF0]


def scan_scratch_words(n: int) -> int:             # pba_host.h
    return (n + SCAN_TILE - 1) // SCAN_TILE + 1


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """the program, once: ({(len, mode): visit fields}, {n_upper: plan fields}, the constants line, the rule table -- one row per
    length 0 .. RULE_MAX, HUGE[0] .. HUGE[1] and 2^32 - 1 --, {(len, mode): ord fields}, {mask: compress fields})"""
    exe = str(tmp_path_factory.mktemp("index_plan") / "index_plan_main")
    consts = [f"-DPBA_IX_{k}={v}" for k, v in (("MAX_LOGP", MAX_LOGP), ("LVL_BITS", LVL_BITS), ("PART_AVG", PART_AVG))]   # seed_index.h's
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + consts + ["-I", os.path.join(ROOT, "pacbioassembly_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(HERE, "cpp", "index_plan_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    args = [f"v:{n}:{m}" for n in LENS for m in MODES.values()] + [f"p:{n}" for n in N_UPPER]
    extra = [f"r:0:{RULE_MAX}", f"r:{HUGE[0]}:{HUGE[1]}", f"r:{0xFFFFFFFF}:{0xFFFFFFFF}"] + [f"o:{n}:{m}" for n in ORD_LENS for m in MODES.values()] + [f"c:{m}" for m in COMPRESS_MASKS]
    p = subprocess.run([exe] + args + extra, capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode(errors="replace")[-4000:]
    lines = [ln.split() for ln in p.stdout.decode().splitlines()]
    assert lines[0][0] == "consts" and len(lines) == 1 + len(args) + RULE_MAX + (HUGE[1] - HUGE[0]) + len(extra)   # (an r: argument prints hi - lo + 1 lines)
    visits = {(int(ln[1]), int(ln[2])): [int(x) for x in ln[3:]] for ln in lines[1:] if ln[0] == "visit"}
    plans = {int(ln[1]): [int(x) for x in ln[2:]] for ln in lines[1:] if ln[0] == "plan"}
    assert len(visits) == 2 * len(LENS) and len(plans) == len(N_UPPER)
    rules = np.array([ln[1:] for ln in lines if ln[0] == "rule"], np.int64)
    want_len = np.concatenate([np.arange(RULE_MAX + 1), np.arange(HUGE[0], HUGE[1] + 1), [0xFFFFFFFF]])
    assert rules.shape == (want_len.size, 1 + 2 * 19) and np.array_equal(rules[:, 0], want_len)
    ords = {(int(ln[1]), int(ln[2])): [int(x) for x in ln[3:]] for ln in lines if ln[0] == "ord"}
    gathers = {int(ln[1]): [int(x) for x in ln[2:]] for ln in lines if ln[0] == "compress"}
    assert len(ords) == 2 * len(ORD_LENS) and len(gathers) == len(set(COMPRESS_MASKS))
    return visits, plans, [int(x) for x in lines[0][1:]], rules, ords, gathers


def test_constants(answers):
    assert answers[2] == [MAX_LOGP, LVL_BITS, PART_AVG]
    assert logp_of(PART_AVG) == 0 and logp_of(PART_AVG + 1) == 1
    assert (levels_of(B2 - 1), levels_of(B2)) == (1, 2) and (levels_of(B3 - 1), levels_of(B3)) == (2, 3)
    assert B2 < 5_000_000 < TILE_SWITCH < B3


@pytest.mark.parametrize("mode", ["all", "head_tail"])
def test_visit_plan_is_the_reference_order(answers, mode):
    for n in LENS:
        visited, nhead, tail_top, bad, nseg, *segs = answers[0][(n, MODES[mode])]
        want_pos, want_visited = visit_order(n, mode)
        assert len(segs) == 4 * nseg and nseg <= 2, (n, mode)
        got, ords = [], []
        for lo, hi, ord0, desc in zip(*[iter(segs)] * 4):
            assert lo < hi, (n, mode)
            p = np.arange(lo, hi, dtype=np.int64)
            got.append(p[::-1] if desc else p)
            ords.append(ord0 + np.arange(hi - lo))
        got = np.concatenate(got) if got else np.zeros(0, np.int64)
        assert np.array_equal(got, want_pos), (n, mode)
        assert np.array_equal(np.concatenate(ords) if ords else np.zeros(0, np.int64), np.arange(got.size)), (n, mode)   # ordinals: the place in the order
        assert visited == want_visited, (n, mode, visited, want_visited)
        assert bad == 0, (n, mode, "ix_ord_pos does not map an ordinal back to its position")
        if mode == "head_tail":
            assert nhead == max(min(n - 16, 20000), 0) and tail_top == n - 16, (n, nhead, tail_top)
    if mode == "head_tail":
        assert answers[0][(0, 1)][0] == 0xFFFFFFF0 and answers[0][(15, 1)][0] == 0xFFFFFFFF     # the negative head, added as it is


def closed_forms(n: np.ndarray, mode: str):
    """index_ref.visit_order as closed forms over an array of lengths: (nhead, tail_lo, tail_top, visited -- the clamped counts and
    the tail interval --, what the builder returns as visited)"""
    if mode == "all":
        return n, np.ones_like(n), np.zeros_like(n), n, n
    nh, nt = np.minimum(n - N_SEQ_WORD, MAX_READ_LEN), np.clip(n - MAX_READ_LEN - N_SEQ_WORD, 0, MAX_READ_LEN)
    top = n - N_SEQ_WORD
    return np.maximum(nh, 0), top - nt + 1, top, np.maximum(nh, 0) + nt, (nh + nt) & 0xFFFFFFFF


@pytest.mark.parametrize("mode", ["all", "head_tail"])
def test_the_rule_at_every_length(answers, mode):
    """visit_rule's fields and chunk numbering, and visit_plan over it, at every length 0 .. RULE_MAX, HUGE[0] .. HUGE[1] and at
    2^32 - 1 (tail_lo / tail_top as the int32 the program prints; the tail's first chunk only where there is a tail: without one it
    numbers nothing)"""
    n = answers[3][:, 0]
    i32 = lambda a: ((a + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    nhead, tail_lo, tail_top, visited, returned = closed_forms(n, mode)
    for k in sorted(set(LENS + [20000 + N_SEQ_WORD, 2 * MAX_READ_LEN + N_SEQ_WORD, RULE_MAX]) & set(n[:RULE_MAX + 1].tolist())):   # the closed forms are visit_order's
        pos, ret = visit_order(k, mode)
        assert (pos.size, ret) == (visited[k], returned[k]) and np.array_equal(pos[:nhead[k]], np.arange(nhead[k])), (k, mode)
        assert np.array_equal(pos[nhead[k]:], np.arange(tail_top[k], tail_lo[k] - 1, -1)), (k, mode)
    ntail = visited - nhead
    got = answers[3][:, 1 + 19 * MODES[mode]:][:, :19]
    r_nhead, r_lo, r_top, r_visited, head_chunks, tail_chunk0, tail_chunks, p_visited, p_nhead, p_top, nseg = got[:, :11].T
    for name, a, b in (("nhead", r_nhead, nhead), ("tail_lo", r_lo, i32(tail_lo)), ("tail_top", r_top, i32(tail_top)), ("visited", r_visited, visited),
                       ("head_chunks", head_chunks, (nhead + 15) // 16), ("tail_chunks", tail_chunks, np.where(ntail > 0, tail_top // 16 - tail_lo // 16 + 1, 0)),   # (the chunks: of the unsigned positions)
                       ("tail_chunk0", np.where(ntail > 0, tail_chunk0, 0), np.where(ntail > 0, tail_lo // 16, 0)),
                       ("visit_plan.visited", p_visited, returned), ("visit_plan.tail_top", p_top, i32(tail_top)),
                       ("visit_plan.nhead", p_nhead, nhead if mode == "head_tail" else np.full_like(n, 0xFFFFFFFF)),
                       ("visit_plan.nseg", nseg, (nhead > 0).astype(np.int64) + (ntail > 0))):
        assert np.array_equal(a, b), (mode, name, n[a != b][:8])
    zero = np.zeros_like(n)
    head = np.stack([zero, nhead, zero, zero], 1)
    tail = np.stack([tail_lo, tail_top + 1, nhead, zero + 1], 1)
    want0 = np.where((nhead > 0)[:, None], head, 0)                  # (a tail without a head does not exist: ntail > 0 needs len > 20 016)
    want1 = np.where((ntail > 0)[:, None], tail, 0)
    assert not (ntail[nhead == 0] > 0).any()
    assert np.array_equal(got[:, 11:15], want0) and np.array_equal(got[:, 15:19], want1), mode
    if mode == "head_tail":
        assert (p_visited[0], p_visited[15], p_visited[16]) == (0xFFFFFFF0, 0xFFFFFFFF, 0)     # the negative head, added as it is


@pytest.mark.parametrize("mode", ["all", "head_tail"])
def test_ord_of_inverts_pos_of_and_the_chunks_cover_the_visited_set_once(answers, mode):
    for n in ORD_LENS:
        visited, seen, bad_inverse, bad_cover = answers[4][(n, MODES[mode])]
        assert visited == seen == visit_order(n, mode)[0].size, (n, mode)       # ord_of >= 0 at exactly as many positions as are visited ...
        assert bad_inverse == 0, (n, mode)                                      # ... which are pos_of's: each maps back, and every ordinal has one
        assert bad_cover == 0, (n, mode)


def test_compress_is_the_bit_gather(answers):
    assert len(SEED_MASKS) >= 4 and all(bin(m).count("1") % 2 == 0 for m in SEED_MASKS)
    for mask in COMPRESS_MASKS:
        tried, bad = answers[5][mask]
        assert tried >= 256 and bad == 0, hex(mask)


@pytest.mark.parametrize("n", N_UPPER)
def test_index_plan_is_the_rules_and_the_sizes_reserved(answers, n):
    logP, n_levels, P, ov_cap, list_off, stat, ov, offs_words, cursor, tile_pre, scan, work_words, *lv = answers[1][n]
    bits, done, lvl_off = lv[0::3], lv[1::3], lv[2::3]
    assert (logP, n_levels, P) == (logp_of(n), levels_of(n), 1 << logp_of(n)) and len(bits) == n_levels
    assert ov_cap == min(P, 4096)
    # the bits: all of logP, no level beyond its LDS tables, the remaining bits split evenly level by level
    assert sum(bits) == logP and max(bits) <= LVL_BITS and max(bits) - min(bits) <= 1 and done == np.cumsum(bits).tolist()
    assert bits == [(logP - (done[k] - bits[k]) + (n_levels - k) - 1) // (n_levels - k) for k in range(n_levels)]
    # offsets arena: the levels' offsets, {0, n}, the three totals, the oversize list (count first): disjoint, inside, in this order
    level_words = [(1 << d) + 1 for d in done]
    regions = [(lvl_off[k], level_words[k]) for k in range(n_levels)] + [(list_off, 2), (stat, 3), (ov, 1 + ov_cap)]
    for (a, na), (b, _) in zip(regions, regions[1:]):
        assert a + na <= b, (regions, n)
    assert lvl_off[0] == 0 and ov + 1 + ov_cap <= offs_words
    assert lvl_off[-1] + level_words[-1] == sum(level_words) <= list_off
    assert offs_words == 2 * P + 2 * n_levels + 8 + 4 + 1 + ov_cap
    # work arena: a cursor per bin of the widest level, a tile count per group of the level before it and one in front, the scan's scratch
    groups = 1 << (done[-2] if n_levels > 1 else 0)
    assert cursor == 0 and cursor + P <= tile_pre and tile_pre + groups + 1 <= scan
    assert scan + scan_scratch_words(P) <= work_words == 3 * P + 64
