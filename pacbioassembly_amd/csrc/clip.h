// clip.h -- the kernels of pba_clip_* (DESIGN §5.8): reads clipped to the span their overlap rows support.
//
// Every read owns clip_entries(L) consecutive int32 entries of a difference arena: entry p counts the intervals whose
// shrunk form [b + m, e - m) begins at p minus those that end there, so the running sum up to p is cov[p], the number of
// counted intervals that span p with at least m bases on both sides.  The -1 of an interval that reaches the read's end
// with m == 0 lands on entry L; the entries are rounded up to a multiple of 4 so that every read begins on a 16-byte line.
//   k_clip_events   a lane per row: +1 / -1 into the arena for each counted role whose read lies in the chunk's range
//   k_clip_sweep    a workgroup per read: the running sum and the runs of positions with cov >= min_cov, CLIP_STEP positions
//                   a step; lane 0 writes the read's pba_clip_row
//   k_clip_gather   a lane per 16 output bases: ASCII of the kept intervals from the packed arena
// Plain C++, vector stores and global atomics; the sweep's scan and reduction go through lane shuffles and LDS.
#ifndef PBA_CLIP_H
#define PBA_CLIP_H

#include "dev_common.h"
#include "pba.h"

#define CLIP_THREADS 256
#define CLIP_PER_LANE 4
#define CLIP_STEP (CLIP_THREADS * CLIP_PER_LANE)              // positions one workgroup takes per step (tests/clip_ref.py: STEP)

enum { CC_IV = 0, CC_SHORT, CC_DROPPED, CC_WHOLE, CC_CUT, CC_MULTI, CC_UNSEEN, CC_COUNT };   // CC_DROPPED + state: a read's state

// arena entries of a read of L bases
static __host__ __device__ __forceinline__ uint64_t clip_entries(uint64_t L) { return (L + 1 + 3) & ~3ull; }

// the sum of a per-lane count over the wavefront, added once to counters[which] (every lane of the wavefront is here)
static __device__ __forceinline__ void clip_count(unsigned long long *counters, int which, int mine) {
    const int w = wave_sum_i32(mine);
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0 && w) atomicAdd(&counters[which], (unsigned long long)w);
}

// cum[r]: the entries of the reads before r (cum[n]: of all); the chunk holds reads [r_lo, r_hi), its arena begins at cum[r_lo]
static __global__ void __launch_bounds__(256)
k_clip_events(const pba_strand_overlap *rows, uint64_t n_rows, const unsigned long long *cum, uint32_t r_lo, uint32_t r_hi, int m,
              uint32_t flags, int *arena, int *niv, unsigned long long *counters) {
    int n_iv = 0, n_short = 0;
    const unsigned long long org = cum[r_lo];
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_rows; k += (uint64_t)gridDim.x * blockDim.x) {
        const pba_strand_overlap r = rows[k];
        for (int role = 0; role < 2; ++role) {
            if (!(flags & (role ? PBA_CLIP_QUERIES : PBA_CLIP_TARGETS))) continue;
            const uint32_t read = (uint32_t)(role ? r.query : r.target);
            if (read < r_lo || read >= r_hi) continue;
            const int b = role ? r.q_beg : r.t_beg, e = role ? r.q_end : r.t_end;
            ++n_iv;
            atomicAdd(&niv[read], 1);
            if ((long long)e - b <= 2ll * m) { ++n_short; continue; }
            int *at = arena + (cum[read] - org);              // b + m < e - m <= L: both entries are the read's own
            atomicAdd(at + b + m, 1);
            atomicAdd(at + e - m, -1);
        }
    }
    clip_count(counters, CC_IV, n_iv);
    clip_count(counters, CC_SHORT, n_short);
}

// What the sweep knows of a stretch [beg, beg + len) of positions: the covered run at its front (pre) and at its back (suf),
// its longest covered run (best, starting at best_at: the first of the longest), its maximal runs, its covered positions and
// its largest coverage.  join(a, b), b following a, is associative; len == 0 is the identity.
struct ClipRun { int beg, len, pre, suf, best, best_at, runs, covered, mx; };

static __device__ __forceinline__ ClipRun clip_none() { return ClipRun{0, 0, 0, 0, 0, 0, 0, 0, 0}; }
static __device__ __forceinline__ ClipRun clip_one(int p, int cov, int c) {
    const int in = cov >= c;
    return ClipRun{p, 1, in, in, in, p, in, in, cov};
}
static __device__ __forceinline__ ClipRun clip_join(const ClipRun &a, const ClipRun &b) {
    if (a.len == 0) return b;
    if (b.len == 0) return a;
    ClipRun o;
    o.beg = a.beg; o.len = a.len + b.len;
    o.pre = a.pre == a.len ? a.len + b.pre : a.pre;
    o.suf = b.suf == b.len ? b.len + a.suf : b.suf;
    o.runs = a.runs + b.runs - (a.suf > 0 && b.pre > 0 ? 1 : 0);
    o.covered = a.covered + b.covered;
    o.mx = max(a.mx, b.mx);
    // the longest, then the smallest start: a's own, the run across the seam, b's own -- in order of their starts
    o.best = a.best; o.best_at = a.best_at;
    const int seam = a.suf + b.pre;
    if (seam > o.best) { o.best = seam; o.best_at = b.beg - a.suf; }
    if (b.best > o.best) { o.best = b.best; o.best_at = b.best_at; }
    return o;
}
static __device__ __forceinline__ ClipRun clip_shfl_down(const ClipRun &v, int d) {
    ClipRun o;
    o.beg = __shfl_down(v.beg, d, PBA_WAVE); o.len = __shfl_down(v.len, d, PBA_WAVE); o.pre = __shfl_down(v.pre, d, PBA_WAVE);
    o.suf = __shfl_down(v.suf, d, PBA_WAVE); o.best = __shfl_down(v.best, d, PBA_WAVE); o.best_at = __shfl_down(v.best_at, d, PBA_WAVE);
    o.runs = __shfl_down(v.runs, d, PBA_WAVE); o.covered = __shfl_down(v.covered, d, PBA_WAVE); o.mx = __shfl_down(v.mx, d, PBA_WAVE);
    return o;
}

// One workgroup per read: read `first + blockIdx.x`.  A step is CLIP_STEP positions, 4 consecutive entries per lane (one
// 16-byte load); the lanes' sums are scanned through shuffles and four LDS words, the carry of the running sum passes from
// step to step in a register every lane keeps, the carry of the runs in thread 0's.  A read of any length is swept by its
// one workgroup, step after step: correct for a 70 001-base sequence, not fast.
// cov_out (nullable): cov[0 .. L) of the read, for pba_clip_coverage (a launch of one workgroup).
static __global__ void __launch_bounds__(CLIP_THREADS)
k_clip_sweep(const int *arena, const unsigned long long *cum, uint32_t r_lo, uint32_t first, const uint32_t *len, const int *niv, int m,
             int c, int min_len, uint32_t flags, pba_clip_row *table, unsigned long long *counters, int *cov_out) {
    __shared__ int wsum[CLIP_THREADS / PBA_WAVE];
    __shared__ ClipRun wrun[CLIP_THREADS / PBA_WAVE];
    const uint32_t read = first + blockIdx.x;
    const int L = (int)len[read];
    const int *d = arena + (cum[read] - cum[r_lo]);
    const int ent = (int)clip_entries((uint64_t)L);
    const int lane = threadIdx.x & (PBA_WAVE - 1), w = threadIdx.x >> 6;
    int carry = 0;
    ClipRun all = clip_none();                                // (thread 0's is the one that counts)
    for (int p0 = 0; p0 < L; p0 += CLIP_STEP) {
        const int p = p0 + CLIP_PER_LANE * (int)threadIdx.x;
        int4 v = make_int4(0, 0, 0, 0);
        if (p < ent) v = *reinterpret_cast<const int4 *>(d + p);        // (ent is a multiple of 4: the whole load is the read's)
        v.y += v.x; v.z += v.y; v.w += v.z;
        int inc = v.w;
#pragma unroll
        for (int k = 1; k < PBA_WAVE; k <<= 1) { const int t = __shfl_up(inc, k, PBA_WAVE); if (lane >= k) inc += t; }
        if (lane == PBA_WAVE - 1) wsum[w] = inc;
        __syncthreads();
        int before = carry + inc - v.w, total = 0;
#pragma unroll
        for (int k = 0; k < CLIP_THREADS / PBA_WAVE; ++k) { if (k < w) before += wsum[k]; total += wsum[k]; }
        carry += total;
        const int cov[4] = {before + v.x, before + v.y, before + v.z, before + v.w};
        ClipRun mine = clip_none();
#pragma unroll
        for (int k = 0; k < CLIP_PER_LANE; ++k)
            if (p + k < L) {
                mine = clip_join(mine, clip_one(p + k, cov[k], c));
                if (cov_out) cov_out[p + k] = cov[k];
            }
#pragma unroll
        for (int k = 1; k < PBA_WAVE; k <<= 1) mine = clip_join(mine, clip_shfl_down(mine, k));   // lane 0: its wavefront, in order
        if (lane == 0) wrun[w] = mine;
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < CLIP_THREADS / PBA_WAVE; ++k) all = clip_join(all, wrun[k]);
        __syncthreads();                                      // (wsum and wrun are written again in the next step)
    }
    if (threadIdx.x != 0) return;
    pba_clip_row o;
    o.read = (int32_t)read; o.n_iv = niv[read]; o.n_runs = all.runs; o.max_cov = all.mx; o.n_covered = all.covered;
    o.state = PBA_CLIP_DROPPED; o.beg = o.end = 0;
    const bool unseen = (flags & PBA_CLIP_KEEP_UNSEEN) && o.n_iv == 0;
    if (unseen) { o.state = PBA_CLIP_WHOLE; o.end = L; }
    else if (all.best > 0) {
        const long long s = all.best_at, e = s + all.best;
        const int kb = (int)max(s - m, 0ll), ke = (int)min(e + m, (long long)L);
        if (ke - kb >= min_len) { o.beg = kb; o.end = ke; o.state = kb == 0 && ke == L ? PBA_CLIP_WHOLE : PBA_CLIP_CUT; }
    }
    if (table) table[read] = o;
    if (counters) {
        atomicAdd(&counters[CC_DROPPED + o.state], 1ull);
        if (o.n_runs >= 2) atomicAdd(&counters[CC_MULTI], 1ull);
        if (unseen) atomicAdd(&counters[CC_UNSEEN], 1ull);
    }
}

// 16 output bases per lane.  toff[0 .. n] is non-decreasing and ends with `total`: the read that supplies base g is the last
// one with toff <= g (reads that keep nothing share their offset with the read after them).  A group that lies inside one
// read takes its 16 codes from 8 packed bytes at whatever 2-bit phase the kept interval begins.
static __global__ void __launch_bounds__(256)
k_clip_gather(SeqSetDev S, const pba_clip_row *table, const unsigned long long *toff, uint32_t n, unsigned long long total, char *text) {
    const unsigned long long groups = (total + 15) / 16;
    for (unsigned long long grp = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; grp < groups; grp += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long g0 = grp * 16;
        const int nb = (int)min(16ull, total - g0);
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (toff[mid] <= g0) lo = mid; else hi = mid;
        }
        uint32_t r = lo;
        unsigned long long r_beg = toff[r], r_end = toff[r + 1];
        const uint8_t *seq = S.packed + S.off[r];
        int from = table[r].beg;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (nb == 16 && g0 + 16 <= r_end) {                   // (g0 >= r_beg by the bisection)
            const uint32_t sp = (uint32_t)from + (uint32_t)(g0 - r_beg);
            const uint64_t be = __builtin_bswap64(ld_u64(seq + (sp >> 2)));     // (8 bytes: the set keeps slack behind its last byte)
            const uint32_t codes = (uint32_t)((be << (2 * (sp & 3))) >> 32);    // base sp in bits 31:30
#pragma unroll
            for (int k = 0; k < 16; ++k)
                w[k >> 2] |= ((0x54474341u >> (8 * ((codes >> (30 - 2 * k)) & 3))) & 0xFFu) << (8 * (k & 3));   // "ACGT"
        } else {
            for (int k = 0; k < nb; ++k) {
                const unsigned long long g = g0 + (unsigned long long)k;
                while (g >= r_end && r + 1 < n) {             // (ends before the bound: toff[n] = total > g)
                    ++r; r_beg = r_end; r_end = toff[r + 1];
                    seq = S.packed + S.off[r];
                    from = table[r].beg;
                }
                const int i = from + (int)(g - r_beg);        // < the kept end <= the read's length
                const int code = (seq[i >> 2] >> (6 - 2 * (i & 3))) & 3;
                w[k >> 2] |= (uint32_t)(uint8_t)"ACGT"[code] << (8 * (k & 3));
            }
        }
        if (nb == 16) *reinterpret_cast<uint4 *>(text + g0) = make_uint4(w[0], w[1], w[2], w[3]);
        else for (int k = 0; k < nb; ++k) text[g0 + k] = (char)(w[k >> 2] >> (8 * (k & 3)));
    }
}

#endif
