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

// Where a batch of walks leaves its runs or its per-window counts (align_windows.h): one bounded slot per pair.  All pointers:
// device, owned by the caller, who copies them back once trace_batch has returned (synchronised).  Pair q's slot is
// slot[off[q] .. off[q + 1]) in elements (a run: uint32_t; a window: pba_aln_counts); n[q] receives what the pair has,
// counts[q] its totals.
struct SlotsInto {
    void *slot;
    const uint64_t *off;
    int32_t *n;
    pba_aln_counts *counts;
    const uint32_t *pair_flags;           // PBA_CIG_* per pair; nullable: `flags` for every pair
    uint32_t flags;
    uint64_t run_max;                     // runs: the widest slot any pair may fill, sizes the wavefronts' goal-first temporaries
    int W;                                // windows: the window size on a's own coordinates, >= 1
    __device__ __forceinline__ uint32_t flags_of(uint32_t q) const {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)(pair_flags ? pair_flags[q] : flags));
    }
    // what a pair whose path was not walked leaves: no elements, zero totals
    __device__ __forceinline__ void close(uint32_t q, bool walked, int have) const {
        if ((threadIdx.x & (PBA_WAVE - 1)) != 0) return;
        if (!walked) counts[q] = pba_aln_counts{0, 0, 0, 0};
        n[q] = have;
    }
};

// The op every lane below cnt holds, in the CIGAR's words, for the sinks that tell `=` from `X`: the element pair, the
// naming of the gaps, the pair's running totals.  classify() returns the lane's code (0 beyond cnt) and the four ballots.
struct OpBallots { uint64_t E, X, I, D; };
struct OpClasses {
    PackedFetch fa, fb;         // element i-1 of a, j-1 of b, direction included
    bool b_is_query;
    int n_eq, n_x, n_ins, n_del;            // wave-uniform: the pair's totals
    __device__ __forceinline__ void init(const PackedFetch &a, const PackedFetch &b, bool swap) {
        fa = a; fb = b; b_is_query = swap; n_eq = 0; n_x = 0; n_ins = 0; n_del = 0;
    }
    __device__ __forceinline__ uint32_t classify(uint32_t op, int i, int j, int cnt, OpBallots &b) {
        uint32_t code = 0u;
        if ((int)(threadIdx.x & (PBA_WAVE - 1)) < cnt) {
            if (op == 1u) code = fa(i - 1) == fb(j - 1) ? (uint32_t)PBA_CIG_EQ : (uint32_t)PBA_CIG_X;   // per element, never per run
            else code = ((op == 2u) != b_is_query) ? (uint32_t)PBA_CIG_DEL : (uint32_t)PBA_CIG_INS;
        }
        b.E = __builtin_amdgcn_ballot_w64(code == (uint32_t)PBA_CIG_EQ); b.X = __builtin_amdgcn_ballot_w64(code == (uint32_t)PBA_CIG_X);
        b.I = __builtin_amdgcn_ballot_w64(code == (uint32_t)PBA_CIG_INS); b.D = __builtin_amdgcn_ballot_w64(code == (uint32_t)PBA_CIG_DEL);
        n_eq += __builtin_popcountll(b.E); n_x += __builtin_popcountll(b.X); n_ins += __builtin_popcountll(b.I); n_del += __builtin_popcountll(b.D);
        return code;
    }
    __device__ __forceinline__ void store(pba_aln_counts *counts) const {       // by one lane
        counts->n_eq = n_eq; counts->n_x = n_x; counts->n_ins = n_ins; counts->n_del = n_del;
    }
};

struct CigarSink : GroupQueue<CigarSink> {
    OpClasses cls;
    uint32_t *tmp;              // this wavefront's closed runs, goal-first
    uint32_t tmp_cap;           // runs tmp holds: a run beyond it is counted, not written
    bool reversed;              // the runs are wanted goal-first, as they lie
    // wave-uniform: the open run carried from the group before, the closed runs so far
    uint32_t c_op, c_len, n_runs;

    __device__ __forceinline__ void init(const PackedFetch &a, const PackedFetch &b, uint32_t *t, uint32_t cap, bool swap, bool rev) {
        cls.init(a, b, swap); tmp = t; tmp_cap = cap; reversed = rev;
        reset(); c_op = 0u; c_len = 0u; n_runs = 0u;
    }
    // lanes 0 .. cnt-1 hold an op each: classify, find the run boundaries, write the runs that close, keep the last one open
    __device__ __forceinline__ void flush(int cnt) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        OpBallots ob;
        const uint32_t code = cls.classify(p_op, p_i, p_j, cnt, ob);
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
    // Closes the open run; out receives the runs origin-first (the order of edits[]) or, reversed, goal-first as they lie --
    // only when all of them fit `cap` slots; returns the number of runs either way.  Lane 0 writes the counts.
    __device__ __forceinline__ int finish(uint32_t *out, uint64_t cap, pba_aln_counts *counts) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        flush_tail();
        if (c_op) {
            if (lane == 0 && n_runs < tmp_cap) tmp[n_runs] = (c_len << 4) | c_op;
            ++n_runs;
        }
        wave_mem_fence();
        if (n_runs <= tmp_cap && (uint64_t)n_runs <= cap)
            for (uint32_t x = (uint32_t)lane; x < n_runs; x += PBA_WAVE)
                out[x] = __hip_atomic_load(tmp + (reversed ? x : n_runs - 1u - x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (lane == 0) cls.store(counts);
        return (int)n_runs;
    }
};

// runs: pair q's to its slot, their number to n[q], the bases of each kind to counts[q].  The wavefront's goal-first temporary
// sits behind cap_words, as OpSink's does: one run per word.
struct CigarJob {
    using Sink = CigarSink;
    SlotsInto s;
    __device__ __forceinline__ void open(CigarSink &k, uint32_t q, const pba_pair &, const PackedFetch &fa, const PackedFetch &fb,
                                         const SeqSetDev &, uint32_t *tmp, uint64_t tmp_words) const {
        const uint32_t fl = s.flags_of(q);
        k.init(fa, fb, tmp, (uint32_t)tmp_words, (fl & PBA_CIG_B_IS_QUERY) != 0, (fl & PBA_CIG_REVERSED) != 0);
    }
    __device__ __forceinline__ int overlap_min() const { return 0; }
    __device__ __forceinline__ void close(CigarSink &k, uint32_t q, bool walked) const {
        const uint64_t o0 = s.off[q], o1 = s.off[q + 1];
        s.close(q, walked, walked ? k.finish((uint32_t *)s.slot + o0, o1 - o0, s.counts + q) : 0);
    }
};

#endif
