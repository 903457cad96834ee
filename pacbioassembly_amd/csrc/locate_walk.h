// locate_walk.h -- the slot arithmetic of k_locate's lane-parallel candidate walk (pba_drivers.hip), stated once for the
// kernel and for a host program.  Plain C++ without HIP: a host program can compile it alone (tests/test_locate_walk_cpu.py
// does).
//
// A read's probes are taken in lane blocks of 64 (probe j = j0 + l in lane l).  Every probe of a block has a run of hits in
// the index (its count may be 0); the runs, probe after probe, form ONE list in the reference's order (locator.cpp:74-79: j
// ascending, inside a probe the index's run order), and the kernel takes that list 64 slots at a time, one slot per lane.
// What is arithmetic about that is here: where a probe's run starts in the list, which (probe, hit) a slot is, and how many
// probes count as "hit" when the walk stops at a given probe.
// The list's length is a 64-bit number: one key of a repeat-rich target can have millions of hits, a set index holds up to
// 2^32 positions, and a block has 64 probes.
#ifndef PBA_LOCATE_WALK_H
#define PBA_LOCATE_WALK_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PBA_LW_FN __host__ __device__ __forceinline__
#else
#define PBA_LW_FN static inline
#endif

#define PBA_LW_PROBES 64                        // probes of a lane block

// where probe l's run starts in the block's list: the exclusive prefix sum of the counts (l = 64: the list's length)
PBA_LW_FN uint64_t lw_offset(const uint32_t *cnt, int l) {
    uint64_t s = 0;
    for (int p = 0; p < l; ++p) s += cnt[p];
    return s;
}

// all 64 of them; returns the list's length
PBA_LW_FN uint64_t lw_offsets(const uint32_t *cnt, uint64_t *off) {
    uint64_t s = 0;
    for (int p = 0; p < PBA_LW_PROBES; ++p) {
        off[p] = s;
        s += cnt[p];
    }
    return s;
}

// The probe list slot s (< the list's length) belongs to: the last p with off[p] <= s.  Its count is not 0 -- a probe
// without hits shares its offset with the next one that has some, and that one comes later.  The hit within the probe's
// run is s - off[p].
PBA_LW_FN int lw_slot_probe(const uint64_t *off, uint64_t s) {
    int p = 0;
    for (int d = PBA_LW_PROBES / 2; d; d >>= 1)
        if (off[p + d] <= s) p += d;
    return p;
}

// probes of the block that found their key (bit l of hitmask: probe l has hits), up to and including probe p
PBA_LW_FN int lw_hits_upto(uint64_t hitmask, int p) {
    return __builtin_popcountll(p >= PBA_LW_PROBES - 1 ? hitmask : hitmask & ((2ull << p) - 1ull));
}

#endif
