// align_cigar.h -- run-length alignments straight from the traceback walk (align_bvtrace.h): a third sink beside OpSink
// (bytes) and VoteSink (votes).  Every diagonal move is told apart as `=` or `X` from the two elements it consumes, 64 ops
// at a time are run-length encoded with ballots, and runs (len << 4 | op, BAM's numbering: include/pba.h) go to memory
// instead of bytes.  No script exists anywhere.
//
// The reference's ops in the CIGAR's words, a = query and b = reference (the default):
//   MATCH  at (i, j): a-element i-1 against b-element j-1     -> `=` or `X`
//   INSERT at (i, j): consumes b-element j-1 only              -> D   (I under PBA_CIG_B_IS_QUERY)
//   DELETE at (i, j): consumes a-element i-1 only              -> I   (D under PBA_CIG_B_IS_QUERY)
#ifndef PBA_ALIGN_CIGAR_H
#define PBA_ALIGN_CIGAR_H

#include "align_bvtrace.h"

struct CigarSink {
    PackedFetch fa, fb;         // element i-1 of a, j-1 of b, direction included
    uint32_t *tmp;              // this wavefront's closed runs, goal-first
    uint32_t tmp_cap;           // runs tmp holds: a run beyond it is counted, not written
    bool b_is_query;
    int k;                      // ops taken so far
    int p_i, p_j;               // this lane's pending op: its cell
    uint32_t p_op;
    // wave-uniform: the open run carried from the group before, the closed runs so far, the four counters
    uint32_t c_op, c_len, n_runs;
    int n_eq, n_x, n_ins, n_del;

    __device__ __forceinline__ void init(const PackedFetch &a, const PackedFetch &b, uint32_t *t, uint32_t cap, bool swap) {
        fa = a; fb = b; tmp = t; tmp_cap = cap; b_is_query = swap;
        k = 0; p_i = 0; p_j = 0; p_op = 0u; c_op = 0u; c_len = 0u; n_runs = 0u; n_eq = 0; n_x = 0; n_ins = 0; n_del = 0;
    }
    // lanes 0 .. cnt-1 hold an op each: classify, find the run boundaries, write the runs that close, keep the last one open
    __device__ __forceinline__ void flush(int cnt) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        uint32_t code = 0u;
        if (lane < cnt) {
            if (p_op == 1u) code = fa(p_i - 1) == fb(p_j - 1) ? (uint32_t)PBA_CIG_EQ : (uint32_t)PBA_CIG_X;   // per element, never per run
            else code = ((p_op == 2u) != b_is_query) ? (uint32_t)PBA_CIG_DEL : (uint32_t)PBA_CIG_INS;
        }
        n_eq += __builtin_popcountll(__builtin_amdgcn_ballot_w64(code == (uint32_t)PBA_CIG_EQ));
        n_x += __builtin_popcountll(__builtin_amdgcn_ballot_w64(code == (uint32_t)PBA_CIG_X));
        n_ins += __builtin_popcountll(__builtin_amdgcn_ballot_w64(code == (uint32_t)PBA_CIG_INS));
        n_del += __builtin_popcountll(__builtin_amdgcn_ballot_w64(code == (uint32_t)PBA_CIG_DEL));
        const uint32_t up = (uint32_t)__shfl_up((int)code, 1, PBA_WAVE);
        const uint32_t before = lane == 0 ? c_op : up;                          // lane 0 looks at the carried run
        const uint64_t B = __builtin_amdgcn_ballot_w64(lane < cnt && code != before);
        if (B == 0ull) { c_len += (uint32_t)cnt; return; }                      // the whole group continues the open run
        const int first = (int)__builtin_ctzll(B), last = 63 - (int)__builtin_clzll(B);
        uint32_t base = n_runs;
        if (c_op) {                                                             // the carried run closes at the first boundary
            if (lane == 0 && base < tmp_cap) tmp[base] = ((c_len + (uint32_t)first) << 4) | c_op;
            ++base;
        }
        if ((B >> lane) & 1ull) {
            const uint64_t above = lane == PBA_WAVE - 1 ? 0ull : B >> (lane + 1);
            if (above) {                                                        // closed inside this group: up to the next boundary
                const uint32_t len = (uint32_t)__builtin_ctzll(above) + 1u;
                const uint32_t slot = base + (uint32_t)__builtin_popcountll(B & ((1ull << lane) - 1ull));
                if (slot < tmp_cap) tmp[slot] = (len << 4) | code;
            }
        }
        n_runs = base + (uint32_t)__builtin_popcountll(B) - 1u;
        c_op = (uint32_t)__builtin_amdgcn_readlane((int)code, last);
        c_len = (uint32_t)(cnt - last);
    }
    __device__ __forceinline__ void put(int op, int i, int j) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        if (lane == (k & (PBA_WAVE - 1))) { p_op = (uint32_t)op; p_i = i; p_j = j; }
        ++k;
        if ((k & (PBA_WAVE - 1)) == 0) flush(PBA_WAVE);
    }
    // n MATCH ops down a diagonal from cell (i, j): op k + r is the MATCH at (i - r, j - r)
    __device__ __forceinline__ void put_run(int n, int i, int j) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        while (n > 0) {
            const int at = k & (PBA_WAVE - 1), take = min(n, PBA_WAVE - at);
            if (lane >= at && lane < at + take) { p_op = 1u; p_i = i - (lane - at); p_j = j - (lane - at); }
            k += take; n -= take; i -= take; j -= take;
            if ((k & (PBA_WAVE - 1)) == 0) flush(PBA_WAVE);
        }
    }
    // Closes the open run; out receives the runs origin-first (the order of edits[]) or, reversed, goal-first as they lie --
    // only when all of them fit `cap` slots; returns the number of runs either way.  Lane 0 writes the counts.
    __device__ __forceinline__ int finish(uint32_t *out, uint64_t cap, bool reversed, pba_aln_counts *counts) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        if (k & (PBA_WAVE - 1)) flush(k & (PBA_WAVE - 1));
        if (c_op) {
            if (lane == 0 && n_runs < tmp_cap) tmp[n_runs] = (c_len << 4) | c_op;
            ++n_runs;
        }
        wave_mem_fence();
        if (n_runs <= tmp_cap && (uint64_t)n_runs <= cap)
            for (uint32_t x = (uint32_t)lane; x < n_runs; x += PBA_WAVE)
                out[x] = __hip_atomic_load(tmp + (reversed ? x : n_runs - 1u - x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (lane == 0) { counts->n_eq = n_eq; counts->n_x = n_x; counts->n_ins = n_ins; counts->n_del = n_del; }
        return (int)n_runs;
    }
};

#endif
