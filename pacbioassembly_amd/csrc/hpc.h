// hpc.h -- the kernels of pba_hpc_* (DESIGN §5.9): homopolymer-compressed sequence sets and rows lifted back.
//
// Position p of a sequence is a run head iff p == 0 or base p differs from base p - 1; hpc(x) is the bases at the heads and
// S[k] the position of head k (S[H] = L).  Everything is read from the bit planes (dev_common.h: 32 bases a word, LSB first,
// plane[2w] low and plane[2w + 1] high, every sequence on whole words), so a set of either layout compresses the same way.
// A chunk is a range [s_lo, s_hi) of sequences, its words [w0, w0 + n_words) of the planes; a tile is HPC_TILE_WORDS words.
//   k_hpc_heads          a lane per plane word: the popcount of its heads, reduced to one count per tile
//   k_hpc_emit           the heads again and a scan in the block on top of the scanned tile counts: every lane writes its
//                        heads' ASCII bases and their positions at their global rank, and the rank of a sequence's first head
//   k_hpc_lift_overlaps  a lane per pba_strand_overlap row: four look-ups in S and the row's arithmetic
//   k_hpc_lift_map_rows  the same for pba_map_row, the read's and the contig's ends through two maps
// Plain C++ and vector stores; no workgroup waits on another.
#ifndef PBA_HPC_H
#define PBA_HPC_H

#include "dev_common.h"
#include "pba.h"

#define HPC_THREADS 256
#define HPC_TILE_WORDS HPC_THREADS                            // one plane word per lane
#define HPC_TILE (HPC_TILE_WORDS * 32)                        // bases one workgroup takes (tests/hpc_ref.py: TILE)

// the sequence of [s_lo, s_hi) that owns plane word w, poff[s_lo] <= w < poff[s_hi]: the last one that begins at or before w
// (empty sequences share their offset with the sequence after them, so the last one is the one with words)
static __device__ __forceinline__ uint32_t hpc_seq_of(const uint64_t *poff, uint32_t s_lo, uint32_t s_hi, uint64_t w) {
    uint32_t lo = s_lo, hi = s_hi;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (poff[mid] <= w) lo = mid; else hi = mid;
    }
    return lo;
}

// What a lane knows of its plane word: the heads among its 32 bases, the two plane words, its sequence and the position of
// its bit 0 inside that sequence.  A word of another lane's sequence is never read: the carry of a sequence's first word is
// replaced by a forced head at bit 0, and the bits at and beyond L -- zero, which is code A -- are masked off.
struct HpcWord { uint32_t heads, lo, hi, seq, p0; bool first; };
static __device__ __forceinline__ HpcWord hpc_word(const SeqSetDev &S, uint32_t s_lo, uint32_t s_hi, uint64_t w) {
    HpcWord o;
    o.seq = hpc_seq_of(S.poff, s_lo, s_hi, w);
    const uint64_t w_first = S.poff[o.seq];
    o.first = w == w_first;
    o.p0 = (uint32_t)(w - w_first) * 32u;
    o.lo = S.plane[2 * w]; o.hi = S.plane[2 * w + 1];
    uint32_t cl = 0, ch = 0;
    if (!o.first) { cl = S.plane[2 * w - 2] >> 31; ch = S.plane[2 * w - 1] >> 31; }
    o.heads = (o.lo ^ (o.lo << 1 | cl)) | (o.hi ^ (o.hi << 1 | ch));
    if (o.first) o.heads |= 1u;
    const uint32_t rem = S.len[o.seq] - o.p0;                 // >= 1: the word is the sequence's
    if (rem < 32) o.heads &= (1u << rem) - 1u;
    return o;
}

static __global__ void __launch_bounds__(HPC_THREADS)
k_hpc_heads(SeqSetDev S, uint32_t s_lo, uint32_t s_hi, uint64_t w0, uint32_t n_words, uint32_t *tile_count) {
    __shared__ int wsum[HPC_THREADS / PBA_WAVE];
    const uint32_t wi = blockIdx.x * HPC_TILE_WORDS + threadIdx.x;
    int cnt = 0;
    if (wi < n_words) cnt = __popc(hpc_word(S, s_lo, s_hi, w0 + wi).heads);
    const int sum = wave_sum_i32(cnt);                        // (every lane is here)
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0) wsum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int k = 0; k < HPC_THREADS / PBA_WAVE; ++k) t += wsum[k];
        tile_count[blockIdx.x] = (uint32_t)t;
    }
}

// tile_incl: the tile counts of the chunk after their inclusive scan; rank0: the heads of the chunks before this one.
// text / starts: one entry per head of the whole set, at its global rank; first[s]: the rank of sequence s's first head
// (written for the sequences that have a base; the host fills in the empty ones from their neighbours).
static __global__ void __launch_bounds__(HPC_THREADS)
k_hpc_emit(SeqSetDev S, uint32_t s_lo, uint32_t s_hi, uint64_t w0, uint32_t n_words, const uint32_t *tile_incl,
           unsigned long long rank0, char *text, uint32_t *starts, unsigned long long *first) {
    __shared__ uint32_t wsum[HPC_THREADS / PBA_WAVE];
    const uint32_t wi = blockIdx.x * HPC_TILE_WORDS + threadIdx.x;
    const int lane = threadIdx.x & (PBA_WAVE - 1), wv = threadIdx.x >> 6;
    HpcWord x;
    x.heads = 0; x.first = false;
    if (wi < n_words) x = hpc_word(S, s_lo, s_hi, w0 + wi);
    const uint32_t cnt = (uint32_t)__popc(x.heads);
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < PBA_WAVE; d <<= 1) { const uint32_t t = __shfl_up(inc, d, PBA_WAVE); if (lane >= d) inc += t; }
    if (lane == PBA_WAVE - 1) wsum[wv] = inc;
    __syncthreads();
    uint32_t before = inc - cnt;
#pragma unroll
    for (int k = 0; k < HPC_THREADS / PBA_WAVE; ++k) if (k < wv) before += wsum[k];
    if (wi >= n_words) return;
    unsigned long long rank = rank0 + (blockIdx.x ? tile_incl[blockIdx.x - 1] : 0u) + before;
    if (x.first) first[x.seq] = rank;
    uint32_t h = x.heads;
    while (h) {
        const int b = __ffs((int)h) - 1;
        h &= h - 1;
        const uint32_t code = ((x.lo >> b) & 1u) | (((x.hi >> b) & 1u) << 1);
        text[rank] = (char)((0x54474341u >> (8 * code)) & 0xFFu);                   // "ACGT"
        starts[rank] = x.p0 + (uint32_t)b;
        ++rank;
    }
}

// One compression as the lift kernels see it: sequence s owns starts[hoff[s] .. hoff[s + 1]), its S[0 .. H); S[H] = len_in[s].
struct HpcMapDev {
    const unsigned long long *hoff;
    const uint32_t *starts;
    const uint32_t *len_in;      // uploaded with the rows: the map itself keeps the lengths on the host
};
// S[k] of sequence s, 0 <= k <= H (checked on the host)
static __device__ __forceinline__ int hpc_lift(const HpcMapDev &m, int s, int k) {
    const unsigned long long o = m.hoff[s];
    const uint32_t H = (uint32_t)(m.hoff[s + 1] - o);
    return (uint32_t)k >= H ? (int)m.len_in[s] : (int)m.starts[o + (uint32_t)k];
}

// rows -> out, which may be the same array: a lane reads its row before it writes it
static __global__ void __launch_bounds__(256)
k_hpc_lift_overlaps(const pba_strand_overlap *rows, uint64_t n, HpcMapDev m, pba_strand_overlap *out) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        pba_strand_overlap r = rows[k];
        const int lq = (int)m.len_in[r.query];
        r.t_beg = hpc_lift(m, r.target, r.t_beg); r.t_end = hpc_lift(m, r.target, r.t_end);
        r.q_beg = hpc_lift(m, r.query, r.q_beg); r.q_end = hpc_lift(m, r.query, r.q_end);
        r.matlen_a = r.t_end - r.t_beg; r.matlen_b = r.q_end - r.q_beg;
        r.ref_pos = r.dir > 0 ? r.t_beg : r.t_end - 16;
        const int qb = r.strand > 0 ? r.q_beg : lq - r.q_end, qe = r.strand > 0 ? r.q_end : lq - r.q_beg;   // the walked text's
        r.j = r.dir > 0 ? qb : lq - qe;
        out[k] = r;
    }
}

static __global__ void __launch_bounds__(256)
k_hpc_lift_map_rows(const pba_map_row *rows, uint64_t n, HpcMapDev reads, HpcMapDev target, pba_map_row *out) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        pba_map_row r = rows[k];
        if (r.found) {
            const int lr = (int)reads.len_in[r.read];
            r.r_beg = hpc_lift(reads, r.read, r.r_beg); r.r_end = hpc_lift(reads, r.read, r.r_end);
            r.c_beg = hpc_lift(target, r.contig, r.c_beg); r.c_end = hpc_lift(target, r.contig, r.c_end);
            r.pos = r.c_beg;
            r.matlen_b = r.c_end - r.c_beg; r.matlen_a = r.r_end - r.r_beg;
            r.j = r.strand > 0 ? r.r_beg : lr - r.r_end;
            r.seglen = lr - r.j;
        }
        out[k] = r;
    }
}

#endif
