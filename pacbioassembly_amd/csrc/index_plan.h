// index_plan.h -- what the host decides about a seed index before anything is launched: the reference's visiting order as
// position segments (visit_plan), the partition regime of a build and where its tables lie in the two pooled arenas
// (index_plan; the tile of the generic level kernels stays the builder's choice: pba_core.hip, index_small_tiles), and the
// ordinal -> position mapping both sides read an entry through (ix_ord_pos).  Plain C++ without HIP: a host program can compile
// it alone (tests/test_index_plan_cpu.py does).  seed_index.h includes it for the kernels.
#ifndef PBA_INDEX_PLAN_H
#define PBA_INDEX_PLAN_H

#include <algorithm>
#include <cstdint>

#include "pba.h"

#if defined(__HIPCC__)
#define PBA_IX_HD __host__ __device__ static inline
#else
#define PBA_IX_HD static inline
#endif

// The regime constants are seed_index.h's, which defines them and then includes this header; a host program that compiles the
// header alone passes the same values with -D.
#if !defined(PBA_IX_MAX_LOGP) || !defined(PBA_IX_LVL_BITS) || !defined(PBA_IX_PART_AVG)
#error "index_plan.h needs PBA_IX_MAX_LOGP, PBA_IX_LVL_BITS and PBA_IX_PART_AVG (seed_index.h)"
#endif

// ord -> position (ref_seq.h:297-308): the head ascending from 0, then the tail descending from tail_top
PBA_IX_HD int32_t ix_ord_pos(uint32_t nhead, int32_t tail_top, uint32_t ord) {
    return ord < nhead ? (int32_t)ord : tail_top - (int32_t)(ord - nhead);
}

// One scan segment: positions [lo, hi) of a sequence, visited ascending (ord = ord0 + pos - lo)
// or descending (ord = ord0 + hi - 1 - pos).
struct ScanSeg {
    uint32_t lo, hi, ord0;
    int descending;
};

// the reference's visiting order as at most two position segments (+ what get_seedmap returns)
struct VisitPlan {
    ScanSeg segs[2];
    int nseg;
    uint32_t visited, nhead;
    int32_t tail_top;
};

static inline VisitPlan visit_plan(uint32_t len, int mode) {
    VisitPlan v;
    v.nseg = 0; v.visited = 0; v.nhead = 0xFFFFFFFFu; v.tail_top = 0;
    if (mode == PBA_INDEX_ALL) {                       // locator.cpp:62: for i in [0, len)
        if (len) v.segs[v.nseg++] = ScanSeg{0, len, 0, 0};
        v.visited = len;
    } else {                                           // ref_seq.h:291-311, MAX_READ_LEN = 20000, N_SEQ_WORD = 16
        const long long L = len, nmax = L - 16;
        const long long nh = std::min(nmax, 20000ll);
        const long long nt = std::min(L - 20000 - 16, 20000ll);
        v.nhead = nh > 0 ? (uint32_t)nh : 0;
        v.tail_top = (int32_t)(L - 16);
        if (nh > 0) v.segs[v.nseg++] = ScanSeg{0, (uint32_t)nh, 0, 0};
        if (nt > 0) v.segs[v.nseg++] = ScanSeg{(uint32_t)(L - 16 - nt + 1), (uint32_t)(L - 16 + 1), v.nhead, 1};
        v.visited = (uint32_t)(nh + (nt < 0 ? 0 : nt));   // ref_seq.h:310 (a negative nhead is added as it is)
    }
    return v;
}

// partitions of 1 024 .. 2 048 entries on average
static inline int index_logp(uint64_t n) {
    int logP = 0;
    while (logP < PBA_IX_MAX_LOGP && (n >> logP) > PBA_IX_PART_AVG) ++logP;
    return logP;
}

// The partition regime of a build of at most n_upper entries (positions visited / slots of a gathered list) and the places of
// its tables, in u32 words, inside the two pooled arenas.
//   offsets arena   the offsets of every level (2^done[k] + 1 words each, sum < 2 P + levels), {0, n} of a gathered list, then
//                   what the build wants zero at its start beside them -- stat: largest partition, partitions beyond the LDS
//                   sort, entries; ov: the sort's oversize list (count, then ov_cap partitions) -- all offs_words zeroed by ONE
//                   memset (a fill per array and level was 30 us of a 330 us build at 5 Mb)
//   work arena      cursor | tile_pre | scan scratch
struct IndexPlan {
    int logP, n_levels;
    uint64_t P;
    int bits[PBA_IX_MAX_LOGP];              // hash bits level k resolves: the remaining bits, split evenly
    int done[PBA_IX_MAX_LOGP];              // ... and the bits resolved once it has run (level k has 2^done[k] bins)
    uint32_t ov_cap;
    uint64_t lvl_off[PBA_IX_MAX_LOGP], list_off, stat, ov, offs_words;
    uint64_t cursor, tile_pre, scan, work_words;
};

static inline IndexPlan index_plan(uint64_t n_upper) {
    IndexPlan p = {};
    p.logP = index_logp(n_upper);
    p.n_levels = std::max(1, (p.logP + PBA_IX_LVL_BITS - 1) / PBA_IX_LVL_BITS);
    p.P = 1ull << p.logP;
    uint64_t at = 0;
    for (int k = 0, done = 0; k < p.n_levels; ++k) {
        p.bits[k] = (p.logP - done + (p.n_levels - k) - 1) / (p.n_levels - k);
        p.done[k] = done += p.bits[k];
        p.lvl_off[k] = at;
        at += (1ull << done) + 1;
    }
    p.ov_cap = (uint32_t)std::min<uint64_t>(p.P, 4096);
    p.list_off = 2 * p.P + 2 * (uint64_t)p.n_levels + 4;
    p.stat = p.list_off + 4;
    p.ov = p.stat + 4;
    p.offs_words = p.ov + 1 + p.ov_cap;
    p.cursor = 0;
    p.tile_pre = p.P + 8;
    p.scan = 2 * (p.P + 8);
    p.work_words = 3 * p.P + 64;
    return p;
}

#endif
