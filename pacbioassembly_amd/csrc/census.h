// census.h -- device side of the seed-key census (pba_census_*): how often every masked seed key occurs among the
// positions the seed index visits, counted into the probe table's own direct addressing (one u32 per bucket
// ix_compress(key, mv): the function overlap.h's pt_bucket<false> calls, index_plan.h), and what is read off the counters: a
// histogram, a batch of look-ups, the probe entries of over-frequent keys overwritten with the all-ones padding k_pt_count /
// k_pt_fill skip, and a per-sequence repeat profile.  Plain HIP: vector stores and global atomics only.
//
// The positions of a sequence are the index's own: the two position segments of its visiting rule (index_plan.h: VisitRule),
// walked in the aligned chunks of 16 positions the rule numbers segment after segment (one 8-byte load of packed bases per
// chunk, seed_index.h: chunk_bits / chunk_key); a position outside the chunk's segment is skipped.  A tile is
// CENSUS_TILE_CHUNKS consecutive chunk numbers of ONE sequence, the tiles of all sequences of
// a call are numbered flat (the host prefix-sums the per-sequence tile counts from the lengths) and a workgroup finds the
// sequence of its tile by bisection: one long contig and many short reads both fill the chip.
#ifndef PBA_CENSUS_H
#define PBA_CENSUS_H

#include "dev_common.h"
#include "pba.h"
#include "seed_index.h"

#define CENSUS_THREADS 256
#define CENSUS_ITERS 4                                          // chunks a thread takes
#define CENSUS_TILE_CHUNKS (CENSUS_THREADS * CENSUS_ITERS)      // 16 384 positions per workgroup
#define CENSUS_HIST_LDS 4096                                    // histogram slots a workgroup keeps in LDS

struct CensusDev {
    uint32_t *count;            // 2^bits counters
    uint32_t mask, mv[5];       // compress_masks(mask)
};
__device__ __forceinline__ uint32_t census_bucket(const CensusDev &C, uint32_t key) { return ix_compress(key, C.mv); }

// tiles of a sequence: host (the tile offsets) and device agree on them through the rule's chunk numbering
static inline uint32_t census_tiles_of(const VisitRule &w) { return (w.chunks() + CENSUS_TILE_CHUNKS - 1) / CENSUS_TILE_CHUNKS; }

// the sequence (relative to the call's first) whose tiles hold tile `b`: the last one that begins at or before it; sequences
// without tiles share their offset with the sequence after them.  tile_at: n_seqs + 1 offsets, tile_at[n_seqs] > b.
__device__ __forceinline__ uint32_t census_seq_of(const uint32_t *tile_at, uint32_t n_seqs, uint32_t b) {
    uint32_t l = 0, r = n_seqs;
    while (r - l > 1) {
        const uint32_t m = l + ((r - l) >> 1);
        if (tile_at[m] <= b) l = m; else r = m;
    }
    return l;
}

// One thread's share of a tile: f(key) for every visited position of its CENSUS_ITERS chunks, key = window & mask (0 included).
template <int MODE, class F>
__device__ __forceinline__ void census_walk_tile(const SeqSetDev &S, uint32_t seq, uint32_t tile, uint32_t mask, F f) {
    const uint32_t len = S.len[seq];
    const uint8_t *p = S.packed + S.off[seq];
    const VisitRule w = visit_rule(len, MODE);
    const uint32_t n0 = w.head_chunks(), nchunks = w.chunks();
    uint64_t be[CENSUS_ITERS];
    uint32_t c[CENSUS_ITERS], lo[CENSUS_ITERS], hi[CENSUS_ITERS];
#pragma unroll
    for (int it = 0; it < CENSUS_ITERS; ++it) {                 // all loads of the thread in flight before the first key is used
        const uint32_t u = tile * CENSUS_TILE_CHUNKS + it * CENSUS_THREADS + threadIdx.x;
        const bool live = u < nchunks;
        const bool tail = u >= n0;
        c[it] = tail ? w.tail_chunk0() + (u - n0) : u;
        lo[it] = live ? (tail ? w.tail_begin() : 0u) : 1u;      // (not live: an empty interval)
        hi[it] = live ? (tail ? w.tail_end() : w.nhead) : 0u;
        be[it] = live ? chunk_bits(p, c[it]) : 0ull;
    }
#pragma unroll
    for (int it = 0; it < CENSUS_ITERS; ++it) {
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) {
            const uint32_t pos = 16 * c[it] + k;
            if (pos >= lo[it] && pos < hi[it]) f(chunk_key(be[it], k, pos, len, mask));
        }
    }
}

// count[bucket(key)] += 1 for every visited position with a nonzero key; tot[0] += those positions, tot[1] += the visited
// positions whose key is zero (one atomic each per wavefront).
// CENSUS_COMBINE_RUNS: a thread adds a RUN of equal keys at the positions it walks one after another with one atomic (a homopolymer or any text of
// period 1 under the mask: every position of it has the same key).  Measured on an MI355X: adds spread over the
// table go at the rate of the position walk either way, adds that all meet one counter are what the plain form cannot do.
// Keys that repeat with a longer period (a satellite) are not combined.
#ifndef CENSUS_COMBINE_RUNS
#define CENSUS_COMBINE_RUNS 1                                    // tuning hook
#endif
template <int MODE>
static __global__ void __launch_bounds__(CENSUS_THREADS)
k_census_count(SeqSetDev S, uint32_t seq_lo, uint32_t n_seqs, const uint32_t *tile_at, CensusDev C, unsigned long long *tot) {
    const uint32_t b = blockIdx.x;
    const uint32_t s = census_seq_of(tile_at, n_seqs, b);
    int counted = 0, zero = 0;
    uint32_t run_key = 0, run_n = 0;                             // (a zero key is never added: an empty run)
    census_walk_tile<MODE>(S, seq_lo + s, b - tile_at[s], C.mask, [&](uint32_t key) {
        counted += key != 0u; zero += key == 0u;                     // (two sums, not a branch: the compiler kept "one of two counters" in scratch)
#if CENSUS_COMBINE_RUNS
        if (key == run_key) { ++run_n; return; }
        if (run_key) atomicAdd(C.count + census_bucket(C, run_key), run_n);   // (no value returned: a fire-and-forget add)
        run_key = key; run_n = 1;
#else
        if (key) atomicAdd(C.count + census_bucket(C, key), 1u);
#endif
    });
    if (CENSUS_COMBINE_RUNS && run_key) atomicAdd(C.count + census_bucket(C, run_key), run_n);
    counted = wave_sum_i32(counted); zero = wave_sum_i32(zero);
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0) {
        if (counted) atomicAdd(tot, (unsigned long long)counted);
        if (zero) atomicAdd(tot + 1, (unsigned long long)zero);
    }
}

// The same walk with a classify instead of an add: out[seq] += visited << 32 | over, over = the visited positions whose key is
// nonzero with count > max_occ -- one u64 atomic per wavefront (over <= visited < 2^32 per sequence: the halves never carry)
template <int MODE>
static __global__ void __launch_bounds__(CENSUS_THREADS)
k_census_repeats(SeqSetDev S, uint32_t n_seqs, const uint32_t *tile_at, CensusDev C, uint32_t max_occ, unsigned long long *out) {
    const uint32_t b = blockIdx.x;
    const uint32_t s = census_seq_of(tile_at, n_seqs, b);
    int visited = 0, over = 0;
    census_walk_tile<MODE>(S, s, b - tile_at[s], C.mask, [&](uint32_t key) {
        ++visited;
        if (key && C.count[census_bucket(C, key)] > max_occ) ++over;
    });
    visited = wave_sum_i32(visited); over = wave_sum_i32(over);
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0 && visited)
        atomicAdd(out + s, (unsigned long long)(uint32_t)visited << 32 | (unsigned long long)(uint32_t)over);
}

// hist[min(count, cap - 1)] += 1 over the buckets with a nonzero count (hist[0] is the host's: 2^bits - n_distinct); the slots
// below CENSUS_HIST_LDS are gathered in LDS per workgroup, the rest go to the global u64 slots one by one.
// res[0] += buckets counted (n_distinct), res[1] = max(count).
static __global__ void __launch_bounds__(256)
k_census_hist(const uint32_t *count, uint64_t n_buckets, uint32_t cap, unsigned long long *hist, unsigned long long *res) {
    __shared__ uint32_t h[CENSUS_HIST_LDS];
    for (uint32_t i = threadIdx.x; i < CENSUS_HIST_LDS; i += blockDim.x) h[i] = 0;
    __syncthreads();
    int distinct = 0;
    uint32_t top = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_buckets; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = count[i];
        if (!c) continue;
        ++distinct;
        top = max(top, c);
        const uint32_t slot = min(c, cap - 1);
        if (slot < CENSUS_HIST_LDS) atomicAdd(&h[slot], 1u);
        else atomicAdd(hist + slot, 1ull);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < CENSUS_HIST_LDS && i < cap; i += blockDim.x)
        if (h[i]) atomicAdd(hist + i, (unsigned long long)h[i]);
    distinct = wave_sum_i32(distinct);
#pragma unroll
    for (int d = 1; d < PBA_WAVE; d <<= 1) top = max(top, (uint32_t)__shfl_xor((int)top, d, PBA_WAVE));
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0 && distinct) {
        atomicAdd(res, (unsigned long long)distinct);
        atomicMax(res + 1, (unsigned long long)top);
    }
}

// counts[i] = count[bucket(keys[i] & mask)], 0 for a key whose masked value is zero
static __global__ void __launch_bounds__(256)
k_census_lookup(CensusDev C, const uint32_t *keys, uint32_t n, uint32_t *counts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = keys[i] & C.mask;
    counts[i] = key ? C.count[census_bucket(C, key)] : 0u;
}

// an entry (key << 32 | probe id) that is not all-ones and whose key has count > max_occ becomes all-ones; *n_masked += the
// entries changed (a ballot per step, one atomic per wavefront)
static __global__ void __launch_bounds__(256)
k_census_mask(CensusDev C, uint64_t *ent, uint64_t n, uint32_t max_occ, unsigned long long *n_masked) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t steps = (n + stride - 1) / stride;           // every lane runs every step: the ballot needs the whole wavefront
    uint32_t changed = 0;                                       // wave-uniform
    for (uint64_t st = 0; st < steps; ++st) {
        const uint64_t i = st * stride + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        bool hit = false;
        if (i < n) {
            const uint64_t e = ent[i];
            const uint32_t key = (uint32_t)(e >> 32) & C.mask;
            hit = e != ~0ull && key != 0u && C.count[census_bucket(C, key)] > max_occ;
            if (hit) ent[i] = ~0ull;
        }
        changed += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(hit));
    }
    if (changed && (threadIdx.x & (PBA_WAVE - 1)) == 0) atomicAdd(n_masked, (unsigned long long)changed);
}

#endif
