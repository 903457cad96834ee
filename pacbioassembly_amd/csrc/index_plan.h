// index_plan.h -- what host and device agree on about a seed index before anything is launched.  The reference's visiting rule,
// stated ONCE (visit_rule -> VisitRule: head, tail, ordinal <-> position, the position segments and their 16-position chunks): the
// index build reads it through visit_plan, the overlap and census kernels directly.  The bit gather ix_compress(x, mv) of the probe
// table, the census and the segment sort, beside its host half compress_masks.  The partition regime of a build and where its
// tables lie in the two pooled arenas (index_plan; the tile of the generic level kernels stays the builder's choice: pba_core.hip,
// index_small_tiles).  Plain C++ without HIP: tests/test_index_plan_cpu.py compiles it alone.  seed_index.h includes it for the kernels.
#ifndef PBA_INDEX_PLAN_H
#define PBA_INDEX_PLAN_H

#include <algorithm>
#include <cstdint>

#include "pba.h"

#if defined(__HIPCC__)
#define PBA_IX_HD __host__ __device__ inline
#else
#define PBA_IX_HD inline
#endif

// The regime constants (index_plan below) are seed_index.h's, which defines them and then includes this header; a host program
// that compiles the header alone passes the same values with -D.
#if !defined(PBA_IX_MAX_LOGP) || !defined(PBA_IX_LVL_BITS) || !defined(PBA_IX_PART_AVG)
#error "index_plan.h needs PBA_IX_MAX_LOGP, PBA_IX_LVL_BITS and PBA_IX_PART_AVG (seed_index.h)"
#endif

// ord -> position (ref_seq.h:297-308): the head ascending from 0, then the tail descending from tail_top.  The one
// implementation: an index keeps (nhead, tail_top) and reads its entries through it, VisitRule::pos_of is it.
PBA_IX_HD int32_t ix_ord_pos(uint32_t nhead, int32_t tail_top, uint32_t ord) {
    return ord < nhead ? (int32_t)ord : tail_top - (int32_t)(ord - nhead);
}

// The visiting rule: which positions of a sequence of `len` bases the seed index visits, and in which order.  PBA_INDEX_ALL: every
// position, ascending (locator.cpp:62).  PBA_INDEX_HEAD_TAIL: ref_seq::get_seedmap (ref_seq.h:291-311; W, M below): the head,
// positions 0 .. min(len - W, M) - 1 ascending, then the tail, min(len - M - W, M) positions descending from len - W; a count
// below 0 visits nothing.  Scalar fields and ternaries only: the same code on both sides, kept in registers by a kernel.
#define PBA_VISIT_WORD 16           // N_SEQ_WORD (dna_seq.h:26): the bases of a seed window
#define PBA_VISIT_MAX_READ 20000    // MAX_READ_LEN (common.h:33)
struct VisitRule {
    uint32_t nhead;                 // the head: positions [0, nhead), ordinals 0 .. nhead - 1 (a negative count clamped to 0)
    int32_t tail_lo, tail_top;      // the tail: positions tail_top down to tail_lo, ordinals from nhead on; none: tail_lo == tail_top + 1
    uint32_t visited;               // positions really visited: nhead + ntail() (NOT what get_seedmap returns below W bases: visit_plan)

    PBA_IX_HD uint32_t ntail() const { return visited - nhead; }
    PBA_IX_HD int32_t pos_of(uint32_t ord) const { return ix_ord_pos(nhead, tail_top, ord); }
    PBA_IX_HD int32_t ord_of(int32_t pos) const {              // -1: not visited (positions below 2^31)
        return (uint32_t)pos < nhead ? pos : (pos >= tail_lo && pos <= tail_top ? (int32_t)nhead + (tail_top - pos) : -1);
    }
    // the position segments: [0, nhead), ascending, and [tail_begin(), tail_end()), descending; an empty one has begin == end
    PBA_IX_HD uint32_t tail_begin() const { return (uint32_t)tail_lo; }
    PBA_IX_HD uint32_t tail_end() const { return (uint32_t)tail_top + 1u; }
    // The aligned chunks of 16 positions (seed_index.h: chunk_bits) that cover a segment, numbered segment after segment: the head
    // takes chunks 0 .. head_chunks() - 1, the tail tail_chunk0() .. tail_chunk0() + tail_chunks() - 1.  A chunk may reach beyond
    // its segment (the one at the seam belongs to both): a walk keeps the positions inside the segment it took the chunk for.
    PBA_IX_HD uint32_t head_chunks() const { return nhead ? ((nhead - 1u) >> 4) + 1u : 0u; }
    PBA_IX_HD uint32_t tail_chunk0() const { return tail_begin() >> 4; }
    PBA_IX_HD uint32_t tail_chunks() const { return ntail() ? ((uint32_t)tail_top >> 4) - tail_chunk0() + 1u : 0u; }
    PBA_IX_HD uint32_t chunks() const { return head_chunks() + tail_chunks(); }
};

PBA_IX_HD VisitRule visit_rule(uint32_t len, int mode) {
    // Signed, min first and the clamp at 0 after it, as the reference writes it: for a caller that knows len >= 0 (overlap.h:
    // k_ovl_walk) each clamp is the one v_med3_i32 that kernel has always had.  huge: len - W does not fit that arithmetic; both counts are M.
    const int32_t W = PBA_VISIT_WORD, M = PBA_VISIT_MAX_READ;
    const bool all = mode == PBA_INDEX_ALL, huge = len > 0x7FFFFFFFu;
    const int32_t top = huge ? 0 : (int32_t)len - W;
    const int32_t nh = top < M ? top : M, nt = top - M < M ? top - M : M;
    const uint32_t ntail = all ? 0u : (huge ? (uint32_t)M : (nt > 0 ? (uint32_t)nt : 0u));
    VisitRule r;
    r.nhead = all ? len : (huge ? (uint32_t)M : (nh > 0 ? (uint32_t)nh : 0u));
    r.tail_top = all ? 0 : (int32_t)(len - (uint32_t)W);
    r.tail_lo = (int32_t)((uint32_t)r.tail_top - ntail + 1u);
    r.visited = r.nhead + ntail;
    return r;
}

// One scan segment: positions [lo, hi) of a sequence, visited ascending (ord = ord0 + pos - lo)
// or descending (ord = ord0 + hi - 1 - pos).
struct ScanSeg {
    uint32_t lo, hi, ord0;
    int descending;
};

// What the index build takes from the rule: the segments with their first ordinals; `visited` as get_seedmap returns it (the
// reference's unsigned sum, ref_seq.h:310: a negative head count is added as it is, len - W wrapped below a window); (nhead,
// tail_top) as an index keeps them for ix_ord_pos (PBA_INDEX_ALL: every ordinal its position, a set's global ones beyond len too).
struct VisitPlan {
    ScanSeg segs[2];
    int nseg;
    uint32_t visited, nhead;
    int32_t tail_top;
};

static inline VisitPlan visit_plan(uint32_t len, int mode) {
    const VisitRule r = visit_rule(len, mode);
    const bool all = mode == PBA_INDEX_ALL;
    VisitPlan v;
    v.nseg = 0;
    if (r.nhead) v.segs[v.nseg++] = ScanSeg{0, r.nhead, 0, 0};
    if (r.ntail()) v.segs[v.nseg++] = ScanSeg{r.tail_begin(), r.tail_end(), r.nhead, 1};
    v.visited = !all && len < PBA_VISIT_WORD ? len - PBA_VISIT_WORD : r.visited;
    v.nhead = all ? 0xFFFFFFFFu : r.nhead;
    v.tail_top = r.tail_top;
    return v;
}

// ix_compress: compress(x, mask) of Hacker's Delight 7-4, the bits of x under `mask` gathered into a number, lowest first.  x holds
// no bit outside the mask.  The host derives the five move masks once per mask (compress_masks), a kernel applies them.
static inline void compress_masks(uint32_t mask, uint32_t mv[5]) {
    uint32_t m = mask, mk = ~m << 1;
    for (int i = 0; i < 5; ++i) {
        uint32_t mp = mk ^ (mk << 1);
        mp ^= mp << 2; mp ^= mp << 4; mp ^= mp << 8; mp ^= mp << 16;
        const uint32_t mvi = mp & m;
        mv[i] = mvi;
        m = (m ^ mvi) | (mvi >> (1 << i));
        mk &= ~mp;
    }
}
PBA_IX_HD uint32_t ix_compress(uint32_t x, const uint32_t (&mv)[5]) {
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 0; i < 5; ++i) { const uint32_t t = x & mv[i]; x = (x ^ t) | (t >> (1 << i)); }
    return x;
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
