"""csrc/index_plan.h alone -- what the host decides about a seed index before anything is launched -- as a stand-alone host
program (tests/cpp/index_plan_main.cpp, under ASan + UBSan where the compiler has the runtimes): visit_plan against
index_ref.visit_order in both modes, index_plan (compiled with seed_index.h's regime constants) against the regime rules
restated in index_ref.py and the sizes the build has always reserved in its two pooled arenas.  No GPU, nothing loaded into python."""
import os
import subprocess

import numpy as np
import pytest

from conftest import HERE, ROOT
from index_ref import LVL_BITS, MAX_LOGP, PART_AVG, define, first_n_with_levels, levels_of, logp_of, tile_switch, visit_order

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"]
LENS = [0, 1, 15, 16, 17, 31, 32, 33, 20000, 20015, 20016, 20017, 20031, 20032, 40015, 40016, 40017, 100000]
MODES = {"all": 0, "head_tail": 1}                 # PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL (include/pba.h)
SCAN_TILE = define("PBA_SCAN_TILE", "seed_index.h")
B2, B3 = first_n_with_levels(2), first_n_with_levels(3)
TILE_SWITCH = tile_switch()                        # (the tile is the builder's choice, not the plan's: its switch is a size like the others here)
N_UPPER = [0, 1, PART_AVG - 1, PART_AVG, PART_AVG + 1, B2 - 1, B2, 5_000_000, TILE_SWITCH, TILE_SWITCH + 1, B3 - 1, B3, 0xFFFFFFF0]


def scan_scratch_words(n: int) -> int:             # pba_host.h
    return (n + SCAN_TILE - 1) // SCAN_TILE + 1


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """the program, once: ({(len, mode): visit fields}, {n_upper: plan fields}, the constants line)"""
    exe = str(tmp_path_factory.mktemp("index_plan") / "index_plan_main")
    consts = [f"-DPBA_IX_{k}={v}" for k, v in (("MAX_LOGP", MAX_LOGP), ("LVL_BITS", LVL_BITS), ("PART_AVG", PART_AVG))]   # seed_index.h's
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + consts + ["-I", os.path.join(ROOT, "pacbioassembly_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
           os.path.join(HERE, "cpp", "index_plan_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    args = [f"v:{n}:{m}" for n in LENS for m in MODES.values()] + [f"p:{n}" for n in N_UPPER]
    p = subprocess.run([exe] + args, capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode(errors="replace")[-4000:]
    lines = [ln.split() for ln in p.stdout.decode().splitlines()]
    assert lines[0][0] == "consts" and len(lines) == 1 + len(args)
    visits = {(int(ln[1]), int(ln[2])): [int(x) for x in ln[3:]] for ln in lines[1:] if ln[0] == "visit"}
    plans = {int(ln[1]): [int(x) for x in ln[2:]] for ln in lines[1:] if ln[0] == "plan"}
    assert len(visits) == 2 * len(LENS) and len(plans) == len(N_UPPER)
    return visits, plans, [int(x) for x in lines[0][1:]]


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
