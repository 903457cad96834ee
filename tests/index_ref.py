"""The seed-hit index as plain numpy, independent of the engine and of the C oracle.

np_index(text, mask, mode) restates hash_table = hash_map<unsigned, list<int>> as locator.cpp:62-66 ("all") and
ref_seq::get_seedmap (ref_seq.h:291-311, "head_tail") fill it: one (key, position) pair per visited position whose
masked key is not zero, sorted by key, and inside a key in visiting order -- the order a list<int> hands back.
tests/test_index_ref_cpu.py pins it to Oracle.index.  It is the reference for checking a device index through
pba_index_find over all distinct keys at once (SeedIndex.dump() sorts on the host and cannot witness device order):
runs() gives the distinct keys and the per-key counts to compare np.diff(hit_off) and hit_pos with.
Also here, restated once for the tests: the regime rules of csrc/index_plan.h (logp_of, levels_of, first_n_with_levels) over the
constants read from the sources (define, tile_switch).
"""
import os
import re

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pacbioassembly_amd", "csrc")


def define(name: str, header: str = "seed_index.h") -> int:
    """a numeric #define of one of the builder's headers: the regime boundaries of the index tests are computed from them"""
    m = re.search(r"^#define[ \t]+%s[ \t]+(\d+)\b" % name, open(os.path.join(CSRC, header)).read(), re.M)
    assert m, f"#define {name} <number> not found in {header}: the regime boundaries of the index tests are computed from it"
    return int(m.group(1))


def tile_switch() -> int:
    """n_upper <= this: tiles of 4 096 entries in the generic level kernels (index_small_tiles, pba_core.hip)"""
    src = open(os.path.join(CSRC, "pba_core.hip")).read()
    m = re.search(r"index_small_tiles\(uint64_t n_upper\)\s*\{\s*return n_upper <= \((\d+)ull << (\d+)\);", src)
    assert m, "index_small_tiles(n_upper) { return n_upper <= (Aull << B); } not found in pba_core.hip"
    return int(m.group(1)) << int(m.group(2))


# ----------------------------------------------------------------------------- the regime rules of index_plan.h, restated
PART_AVG = define("PBA_IX_PART_AVG", "seed_index.h")
LVL_BITS = define("PBA_IX_LVL_BITS", "seed_index.h")
MAX_LOGP = define("PBA_IX_MAX_LOGP", "seed_index.h")


def logp_of(n_upper: int) -> int:                  # index_logp
    lp = 0
    while lp < MAX_LOGP and (n_upper >> lp) > PART_AVG:
        lp += 1
    return lp


def levels_of(n_upper: int) -> int:
    return max(1, -(-logp_of(n_upper) // LVL_BITS))


def first_n_with_levels(k: int) -> int:            # the smallest n_upper that takes k partition levels
    return 1 if k == 1 else (PART_AVG + 1) << ((k - 1) * LVL_BITS)


MAX_READ_LEN = 20000      # common.h:33
N_SEQ_WORD = 16           # dna_seq.h:26

_LUT = np.full(256, 3, np.uint8)              # C2I (dna_seq.h:21): A 0, C 1, G 2, everything else 3
_LUT[ord("A")], _LUT[ord("C")], _LUT[ord("G")] = 0, 1, 2


def np_keys(text: bytes) -> np.ndarray:
    """encode16 of the window at every position of text (u32[len]); windows past the end are padded with code 3.
    Byte k of a key holds bases 4k .. 4k+3, the first base in bits 7:6 (dna_seq.h:86-95)."""
    n = len(text)
    c = np.full(n + 15, 3, np.uint8)
    c[:n] = _LUT[np.frombuffer(text, np.uint8)]
    m = n + 12                                 # bytes of four bases starting at every position
    b4 = (c[0:m] << 6) | (c[1:m + 1] << 4) | (c[2:m + 2] << 2) | c[3:m + 3]
    del c
    key = b4[0:n].astype(np.uint32)
    for k in (1, 2, 3):
        key |= b4[4 * k:4 * k + n].astype(np.uint32) << np.uint32(8 * k)
    return key


def visit_order(n: int, mode: str):
    """(positions in visiting order, what the builder returns as `visited`)."""
    if mode == "all":
        return np.arange(n, dtype=np.int64), n
    nh = min(n - N_SEQ_WORD, MAX_READ_LEN)
    nt = min(n - MAX_READ_LEN - N_SEQ_WORD, MAX_READ_LEN)
    head = np.arange(max(nh, 0), dtype=np.int64)
    tail = n - N_SEQ_WORD - np.arange(max(nt, 0), dtype=np.int64)
    # ref_seq.h:310 returns nhead + (ntail < 0 ? 0 : ntail) as an unsigned: a negative nhead wraps
    return np.concatenate([head, tail]), (nh + max(nt, 0)) & 0xFFFFFFFF


def np_index(text: bytes, mask: int, mode: str = "all"):
    """(keys u32, pos i32, visited): the index entries sorted by key, visiting order kept inside a key."""
    assert mode in ("all", "head_tail")
    order, visited = visit_order(len(text), mode)
    key = np_keys(text)
    if mode != "all":
        key = key[order]
    key &= np.uint32(mask)
    ords = np.flatnonzero(key)                                     # zero keys are dropped
    # sorting (key, visiting ordinal) as one 64-bit number IS the stable sort by key
    e = (key[ords].astype(np.uint64) << np.uint64(32)) | ords.astype(np.uint64)
    del key, ords
    e.sort()
    keys = (e >> np.uint64(32)).astype(np.uint32)
    o = (e & np.uint64(0xFFFFFFFF)).astype(np.int64)
    del e
    pos = o.astype(np.int32) if mode == "all" else order[o].astype(np.int32)
    return keys, pos, visited


def runs(keys: np.ndarray):
    """(distinct keys ascending, entries of each) of a sorted key array."""
    if keys.size == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.int64)
    start = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
    return keys[start], np.diff(np.concatenate([start, [keys.size]])).astype(np.int64)
