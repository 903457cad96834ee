// align_alleles.h -- every row's allele at the selection sites of its target, straight from the traceback walk
// (align_bvtrace.h): a fifth sink beside OpSink (bytes), VoteSink (votes), CigarSink (runs) and WindowSink (per-window
// counts); the op queue is GroupQueue's.  a is the target, the side the vote boxes belong to, exactly as in VoteSink; the
// sites are a pba_sites' (pba_sites.hip): one bit per box of the arena its sites were read from, the arena word of target t's
// position x being that of box_off[t - t_lo] + x.
//   MATCH  at (i, j): a-element i-1 at x = a_pos +/- (i-1), the allele is b-element j-1 (0..3)
//   DELETE at (i, j): a-element i-1, the allele is 4 (DEL)
//   INSERT at (i, j): no a-element: nothing
// A lane whose x has its bit set in the SEL bitmap emits one pba_allele.  SUP sites get no per-row record: a row can supply
// one box several times, and which of its INSERTs speaks for the row is left for later.
//
// Placement.  Every a-element of [0, matlen_a) is consumed by exactly one MATCH or DELETE of the path, so a pair has exactly
// one record per SEL site inside the a-interval its path covers: n = rank(hi + 1) - rank(lo), rank(b) = the SEL sites of the
// arena below box b (the scanned per-word counts plus a popcount of the word's low bits).  matlen_a is the i of the first op
// the walk puts -- it sits at the goal cell --, so n is known from two rank lookups before any record is written.  The walk
// meets the a-elements, and so the sites, monotonically; the record of the site of SEL rank r goes straight to slot
// r - rank(lo): ascending site order for forward and backward accessors alike.  n[q] is that number.  No temporary and no
// compaction exist.
#ifndef PBA_ALIGN_ALLELES_H
#define PBA_ALIGN_ALLELES_H

#include "align_cigar.h"

// The sites as the sink sees them (all pointers: device, owned by the pba_sites).  bm has a zero word behind the arena's
// last, so rank(n_boxes) reads inside; rank[w] = SEL sites of words 0 .. w (inclusive scan); sel[r] = { record index, own |
// major << 4 | minor << 8 } of the SEL site of rank r.
struct AllelesInto {
    const unsigned long long *bm;
    const uint32_t *rank;
    const uint2 *sel;
    const unsigned long long *box_off;
    uint32_t t_lo;
    unsigned long long n_boxes;
    __device__ __forceinline__ uint32_t rank_below(unsigned long long box) const {
        const unsigned long long w = box >> 6;
        const uint32_t before = w ? rank[w - 1] : 0u;
        return before + (uint32_t)__builtin_popcountll(bm[w] & ((1ull << (box & 63ull)) - 1ull));
    }
};

struct AlleleSink : GroupQueue<AlleleSink> {
    AllelesInto S;
    PackedFetch fb;             // the row's side (b)
    pba_allele *out;            // this pair's slot
    uint64_t cap;               // records the slot holds: with fewer than n_rec nothing is written
    unsigned long long seg;     // the arena box of the target's position 0
    int a_pos, a_step, a_len;   // x(e) = a_pos + a_step * e; the target's length
    // wave-uniform: the records of the pair (-1 before the first op), the SEL rank of its first, the pair's totals
    int n_rec;
    uint32_t r0;
    int t_own, t_major, t_minor, t_other;

    __device__ __forceinline__ void init(const AllelesInto &s, const PackedFetch &b, unsigned long long seg0, int len, int pos, bool a_backward,
                                         pba_allele *slot, uint64_t slot_cap) {
        S = s; fb = b; out = slot; cap = slot_cap; seg = seg0; a_len = len; a_pos = pos; a_step = a_backward ? -1 : 1;
        reset(); n_rec = -1; r0 = 0u;
        t_own = 0; t_major = 0; t_minor = 0; t_other = 0;
    }
    // the first op sits at the goal cell: its i is matlen_a, and the covered a-interval gives the number of records
    __device__ __forceinline__ void open_span(int matlen_a) {
        n_rec = 0;
        if (matlen_a < 1) return;
        const int last = a_pos + a_step * (matlen_a - 1);
        const int lo = min(a_pos, last), hi = max(a_pos, last);
        if (lo < 0 || hi >= a_len || seg + (unsigned long long)hi >= S.n_boxes) return;      // (the host checked the accessor: never)
        r0 = S.rank_below(seg + (unsigned long long)lo);
        n_rec = (int)(S.rank_below(seg + (unsigned long long)hi + 1ull) - r0);
    }
    // lanes 0 .. cnt-1 hold an op each: the lanes on a SEL site write their record at its final place
    __device__ __forceinline__ void flush(int cnt) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        if (n_rec < 0) open_span(__builtin_amdgcn_readfirstlane(p_i));
        bool hit = false;
        uint32_t allele = 0u, pack = 0u;
        if (lane < cnt && p_op != 2u && n_rec > 0) {
            const int x = a_pos + a_step * (p_i - 1);
            if (x >= 0 && x < a_len) {
                const unsigned long long box = seg + (unsigned long long)x;
                if ((S.bm[box >> 6] >> (box & 63ull)) & 1ull) {
                    const uint32_t r = S.rank_below(box);
                    const uint2 s = S.sel[r];
                    const uint32_t at = r - r0;
                    allele = p_op == 1u ? (uint32_t)fb(p_j - 1) : 4u;
                    pack = s.y;
                    hit = true;
                    if ((uint64_t)n_rec <= cap && at < (uint32_t)n_rec) *(uint2 *)(out + at) = make_uint2(s.x, allele);   // never outside the slot
                }
            }
        }
        const uint64_t H = __builtin_amdgcn_ballot_w64(hit);
        if (H == 0ull) return;
        const bool is_major = allele == ((pack >> 4) & 15u), is_minor = allele == ((pack >> 8) & 15u);
        t_own += __builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && allele == (pack & 15u)));
        t_major += __builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && is_major));
        t_minor += __builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && is_minor));
        t_other += __builtin_popcountll(__builtin_amdgcn_ballot_w64(hit && !is_major && !is_minor));
    }
    // returns the number of records (a path without ops: none); lane 0 writes the totals (n_own, n_major, n_minor, n_other
    // in the four ints of a pba_aln_counts: the slot runner's record; n_sites is n[q])
    __device__ __forceinline__ int finish(pba_aln_counts *counts) {
        flush_tail();
        if (n_rec < 0) n_rec = 0;
        if ((threadIdx.x & (PBA_WAVE - 1)) == 0) *(int4 *)counts = make_int4(t_own, t_major, t_minor, t_other);
        return n_rec;
    }
};

// alleles: pair q's records to its slot, their number to n[q], the totals to counts[q]; gated like a vote (gate: the
// smallest matlen_a that is walked; 0: none).
struct AlleleJob {
    using Sink = AlleleSink;
    SlotsInto s;
    AllelesInto S;
    int gate;
    __device__ __forceinline__ void open(AlleleSink &k, uint32_t q, const pba_pair &pr, const PackedFetch &, const PackedFetch &fb,
                                         const SeqSetDev &A, uint32_t *, uint64_t) const {
        const uint64_t o0 = s.off[q], o1 = s.off[q + 1];
        k.init(S, fb, S.box_off[pr.a_seq - S.t_lo], (int)A.len[pr.a_seq], pr.a_pos, (pr.flags & PBA_A_BACKWARD) != 0, (pba_allele *)s.slot + o0,
               o1 - o0);
    }
    __device__ __forceinline__ int overlap_min() const { return gate; }
    __device__ __forceinline__ void close(AlleleSink &k, uint32_t q, bool walked) const {
        s.close(q, walked, walked ? k.finish(s.counts + q) : 0);
    }
};

#endif
