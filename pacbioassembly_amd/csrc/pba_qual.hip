// pba_qual.hip -- the per-base evidence of an evolved set as an object on the device (include/pba.h: pba_qual; qual.h; DESIGN
// §5.12): made by the evidence write passes of pba_pileup.hip (qual_adopt) or from host arrays (pba_qual_create), read back
// (pba_qual_get), reduced to one row per sequence (pba_qual_summary), searched for its low spans (pba_qual_low_spans) and
// written out with its set as FASTQ (pba_seqs_write_fastq).  Host side and kernels.
// Summary and spans walk the evidence in tiles of Q_TILE bases of one sequence, one workgroup of 256 threads per tile, 16
// consecutive bases per thread; tiles[]: (sequence, first base inside it), made by the host as pba_pileup.hip makes its own.
// A short sequence is one tile, a megabase contig some hundreds: nothing is swept serially.
//   summary   per tile: the thread's counts, summed over the workgroup, one set of atomics per tile on the sequence's row.  A
//             run of qv < qmin is counted at its head, which needs only its left neighbour: tiles are independent.
//   spans     k_span_count  heads and tails of every tile (a tail needs only its right neighbour), heads in cnt[0 .. T), tails in
//                           cnt[T .. 2T): ONE scan ranks both -- the k-th head and the k-th tail are the same run
//             k_span_emit   every head writes (seq, beg) of its run, every tail its end, every low base lowers its run's min_qv
//                           (the thread's own minimum first, one atomic per run and thread)
//             k_span_keep / k_span_compact   end - beg >= min_run, scanned, the kept runs in order at the front of the output
//   FASTQ     k_fq_write: the twin of k_fx_write (pba_fastx.hip) -- 64 bases of one sequence per thread, their quality
//             characters on the line below, the thread of a sequence's first chunk its three line ends and the '+'.
// The per-base arrays never cross to the host here.  Work buffers: per call, apart from the image (POOL_FX_IMG) and its
// tables (POOL_FX_RECS), whose owners are idle; nothing read from them was not written by the call itself.
#include "pba_host.h"
#include "qual.h"

#define Q_TILE 4096u
#define Q_RUN 16u
#define FQ_RUN 64                          // bases per thread of k_fq_write
static const uint32_t kQualSlice = 1u << 22;          // workgroups per launch (a launch's global size is a 32-bit number)
static const uint64_t kFqPiece = (uint64_t)1 << 30;

struct QTile { uint32_t seq, first; };
struct QualDev {
    const uint8_t *qv;
    const uint16_t *depth;
    const uint32_t *src;
    const unsigned long long *off;
};

static_assert(sizeof(pba_qual_row) == 56 && sizeof(pba_qual_span) == 16, "pba_qual_row / pba_qual_span layout");

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_qual_phred(const uint32_t *agree, const unsigned long long *n, uint64_t count, int qmax, uint8_t *qv) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (uint64_t)gridDim.x * blockDim.x)
        qv[i] = (uint8_t)qual_phred(agree[i], n[i], qmax);
}

__global__ void __launch_bounds__(256)
k_qual_rows_init(const unsigned long long *off, uint32_t n, pba_qual_row *rows) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    pba_qual_row r;
    memset(&r, 0, sizeof r);
    r.seq = (int32_t)s; r.len = (int32_t)(off[s + 1] - off[s]);
    r.min_qv = r.len ? 127 : -1;                               // (every qv is at most PBA_QUAL_QCAP)
    rows[s] = r;
}

// the lanes' values summed over the workgroup of 256, for every thread (part: LDS, 4 words; two barriers)
__device__ __forceinline__ uint32_t q_block_sum(uint32_t v, uint32_t *part) {
#pragma unroll
    for (int d = 32; d; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    __syncthreads();                                           // part[] of the call before has been read
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// the bases of tile t a thread owns: [*j, *end) inside the sequence that starts at *base and has *len bases
__device__ __forceinline__ void q_thread_range(const QualDev &Q, const QTile &t, unsigned long long *base, uint32_t *len, uint32_t *j, uint32_t *end) {
    *base = Q.off[t.seq];
    *len = (uint32_t)(Q.off[t.seq + 1] - *base);
    const uint32_t tile_end = min(*len, t.first + Q_TILE);     // (first + Q_TILE < 2^32: first is below the length, a u32)
    *j = min(tile_end, t.first + threadIdx.x * Q_RUN);
    *end = min(tile_end, *j + Q_RUN);
}

__global__ void __launch_bounds__(256)
k_qual_summary(QualDev Q, const QTile *tiles, uint32_t tile0, int qmin, pba_qual_row *rows) {
    __shared__ uint32_t part[4];
    const QTile t = tiles[tile0 + blockIdx.x];
    unsigned long long base;
    uint32_t len, j, end;
    q_thread_range(Q, t, &base, &len, &j, &end);
    uint32_t n_sup = 0, n_unvoted = 0, n_below = 0, n_heads = 0, sum_qv = 0, sum_depth = 0, n_mine = end - j;
    int mn = 127, mx = 0;
    bool prev_low = j > 0 && j < end && (int)Q.qv[base + j - 1] < qmin;
    for (; j < end; ++j) {
        const int q = Q.qv[base + j], d = Q.depth[base + j];
        const bool low = q < qmin;
        n_sup += Q.src[base + j] >> 31; n_unvoted += d == 0; n_below += low; n_heads += low && !prev_low;
        sum_qv += (uint32_t)q; sum_depth += (uint32_t)d;       // (a tile's sums: at most 4 096 x 65 535)
        mn = min(mn, q); mx = max(mx, d);
        prev_low = low;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) { mn = min(mn, __shfl_xor(mn, d, 64)); mx = max(mx, __shfl_xor(mx, d, 64)); }
    n_mine = q_block_sum(n_mine, part);
    n_sup = q_block_sum(n_sup, part); n_unvoted = q_block_sum(n_unvoted, part); n_below = q_block_sum(n_below, part);
    n_heads = q_block_sum(n_heads, part); sum_qv = q_block_sum(sum_qv, part); sum_depth = q_block_sum(sum_depth, part);
    pba_qual_row *r = rows + t.seq;
    if ((threadIdx.x & 63) == 0) { atomicMin(&r->min_qv, mn); atomicMax(&r->max_depth, mx); }
    if (threadIdx.x == 0) {
        atomicAdd(&r->n_sel, (int)(n_mine - n_sup)); atomicAdd(&r->n_sup, (int)n_sup); atomicAdd(&r->n_unvoted, (int)n_unvoted);
        atomicAdd(&r->n_below, (int)n_below); atomicAdd(&r->n_low_runs, (int)n_heads);
        atomicAdd((unsigned long long *)&r->sum_qv, (unsigned long long)sum_qv);
        atomicAdd((unsigned long long *)&r->sum_depth, (unsigned long long)sum_depth);
    }
}

// heads and tails among the thread's bases: bit k of *hm / *tm for base j + k
__device__ __forceinline__ void q_thread_flags(const QualDev &Q, unsigned long long base, uint32_t len, uint32_t j, uint32_t end, int qmin,
                                               uint32_t *hm, uint32_t *tm, uint32_t *lm) {
    uint32_t h = 0, t = 0, l = 0;
    if (j < end) {
        bool prev_low = j > 0 && (int)Q.qv[base + j - 1] < qmin;
        bool low = (int)Q.qv[base + j] < qmin;
        for (uint32_t k = 0; j + k < end; ++k) {
            const bool next_low = j + k + 1 < len && (int)Q.qv[base + j + k + 1] < qmin;
            if (low) { l |= 1u << k; if (!prev_low) h |= 1u << k; if (!next_low) t |= 1u << k; }
            prev_low = low; low = next_low;
        }
    }
    *hm = h; *tm = t; *lm = l;
}

__global__ void __launch_bounds__(256)
k_span_count(QualDev Q, const QTile *tiles, uint32_t tile0, uint32_t n_tiles, int qmin, uint32_t *cnt) {
    __shared__ uint32_t part[4];
    const QTile t = tiles[tile0 + blockIdx.x];
    unsigned long long base;
    uint32_t len, j, end, hm, tm, lm;
    q_thread_range(Q, t, &base, &len, &j, &end);
    q_thread_flags(Q, base, len, j, end, qmin, &hm, &tm, &lm);
    const uint32_t nh = q_block_sum(__popc(hm), part), nt = q_block_sum(__popc(tm), part);
    if (threadIdx.x == 0) { cnt[tile0 + blockIdx.x] = nh; cnt[n_tiles + tile0 + blockIdx.x] = nt; }
}

// what the lanes in front of this one hold, over the workgroup of 256 (wsum: LDS, 4 words; two barriers)
__device__ __forceinline__ uint32_t q_block_excl(uint32_t v, uint32_t *wsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t x = __shfl_up(inc, d, 64); if (lane >= d) inc += x; }
    __syncthreads();
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t carry = 0;
    for (int k = 0; k < w; ++k) carry += wsum[k];
    return carry + inc - v;
}

// cnt: the inclusive scan of k_span_count's counts; raw[r]: run r, min_qv preset to a value above every qv
__global__ void __launch_bounds__(256)
k_span_emit(QualDev Q, const QTile *tiles, uint32_t tile0, uint32_t n_tiles, int qmin, const uint32_t *cnt, pba_qual_span *raw) {
    __shared__ uint32_t wsum[4];
    const uint32_t ti = tile0 + blockIdx.x;
    const QTile t = tiles[ti];
    unsigned long long base;
    uint32_t len, j, end, hm, tm, lm;
    q_thread_range(Q, t, &base, &len, &j, &end);
    q_thread_flags(Q, base, len, j, end, qmin, &hm, &tm, &lm);
    const uint32_t n_runs = cnt[n_tiles - 1];
    uint32_t h = (ti ? cnt[ti - 1] : 0u) + q_block_excl(__popc(hm), wsum);             // heads in front of this thread's bases
    uint32_t tl = cnt[n_tiles + ti - 1] - n_runs + q_block_excl(__popc(tm), wsum);      // tails likewise
    int mn = 127;
    for (uint32_t k = 0; j + k < end; ++k) {
        if (!((lm >> k) & 1u)) continue;
        if ((hm >> k) & 1u) { raw[h].seq = (int32_t)t.seq; raw[h].beg = (int32_t)(j + k); ++h; mn = 127; }
        mn = min(mn, (int)Q.qv[base + j + k]);                 // (a low base lies in run h - 1: its head is the last one so far)
        if ((tm >> k) & 1u) { raw[tl].end = (int32_t)(j + k + 1); ++tl; }
        if (((tm >> k) & 1u) || j + k + 1 == end) atomicMin(&raw[h - 1].min_qv, mn);
    }
}

__global__ void __launch_bounds__(256)
k_span_keep(const pba_qual_span *raw, uint32_t n_runs, int min_run, uint32_t *keep) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r < n_runs) keep[r] = raw[r].end - raw[r].beg >= min_run ? 1u : 0u;
}

// keep: the inclusive scan of k_span_keep's flags
__global__ void __launch_bounds__(256)
k_span_compact(const pba_qual_span *raw, uint32_t n_runs, const uint32_t *keep, pba_qual_span *out, uint64_t cap) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t mine = keep[r], before = r ? keep[r - 1] : 0u;
    if (mine != before && before < cap) out[before] = raw[r];
}

// Thread t owns chunk t: FQ_RUN bases of sequence first + s, the last s with cpre[s] <= t (every sequence has one chunk at
// least).  body[s]: where its first base goes in the image; its quality line starts len + 3 further on.
__global__ void __launch_bounds__(256)
k_fq_write(const uint8_t *packed, const uint64_t *off, const uint32_t *len, const uint8_t *qv, const unsigned long long *qoff, uint32_t first,
           uint32_t n, const uint64_t *cpre, const uint64_t *body, uint64_t total_chunks, uint8_t *img) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_chunks; t += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cpre[mid] <= t) lo = mid; else hi = mid;
        }
        const uint32_t s = lo, L = len[first + s];
        const uint64_t j0 = (t - cpre[s]) * FQ_RUN;
        uint8_t *bases = img + body[s], *quals = bases + (uint64_t)L + 3;
        if (j0 == 0) { bases[L] = '\n'; bases[(uint64_t)L + 1] = '+'; bases[(uint64_t)L + 2] = '\n'; quals[L] = '\n'; }
        if (j0 >= L) continue;
        const uint8_t *src = packed + off[first + s], *q = qv + qoff[first + s];
        const uint32_t cnt = (uint32_t)min((uint64_t)FQ_RUN, (uint64_t)L - j0);
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t j = (uint32_t)j0 + k;
            const uint32_t code = (src[j >> 2] >> (6 - 2 * (j & 3))) & 3u;
            bases[j] = code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T';
            quals[j] = (uint8_t)('!' + q[j]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
static void qual_free(pba_qual *q) {
    for (void *p : {(void *)q->d_qv, (void *)q->d_depth, (void *)q->d_agree, (void *)q->d_src, (void *)q->d_off})
        if (p) (void)hipFree(p);
    delete q;
}

// the (sequence, first base) table of q's tiles, on the device; *n_tiles of them (none: no bases)
static int qual_tiles(pba_ctx *ctx, const pba_qual *q, DevBuf *d_tiles, uint32_t *n_tiles) {
    uint64_t nt = 0;
    for (uint32_t s = 0; s < q->n; ++s) nt += (q->h_off[s + 1] - q->h_off[s] + Q_TILE - 1) / Q_TILE;
    if (nt >= (1ull << 31)) PBA_FAIL(PBA_E_TOOLONG, "pba_qual: 2^31 tiles or more");
    *n_tiles = (uint32_t)nt;
    if (!nt) return PBA_OK;
    std::vector<QTile> tiles;
    tiles.reserve((size_t)nt);
    for (uint32_t s = 0; s < q->n; ++s)
        for (uint64_t at = 0, len = q->h_off[s + 1] - q->h_off[s]; at < len; at += Q_TILE) tiles.push_back(QTile{s, (uint32_t)at});
    HIPCHK(hipMalloc(&d_tiles->p, sizeof(QTile) * tiles.size()));
    HIPCHK(hipMemcpy(d_tiles->p, tiles.data(), sizeof(QTile) * tiles.size(), hipMemcpyHostToDevice));      // (tiles dies with this scope)
    return PBA_OK;
}

static QualDev qual_dev(const pba_qual *q) { return QualDev{q->d_qv, q->d_depth, q->d_src, q->d_off}; }

extern "C" {

int qual_adopt(pba_ctx *ctx, uint32_t n, const uint64_t *h_off, void *arr[4], pba_qual **out) {
    pba_qual *q = new (std::nothrow) pba_qual();
    if (!q) {
        for (int a = 0; a < 4; ++a) if (arr[a]) (void)hipFree(arr[a]);
        PBA_FAIL(PBA_E_NOMEM, "pba_qual");
    }
    q->device = ctx->device; q->n = n;
    q->d_qv = (uint8_t *)arr[0]; q->d_depth = (uint16_t *)arr[1]; q->d_agree = (uint16_t *)arr[2]; q->d_src = (uint32_t *)arr[3];
    q->d_off = nullptr;
    q->h_off.assign(h_off, h_off + (size_t)n + 1);
    hipError_t e = hipMalloc((void **)&q->d_off, sizeof(uint64_t) * ((size_t)n + 1));
    if (e == hipSuccess) e = hipMemcpy(q->d_off, q->h_off.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipGetLastError(); qual_free(q); return ctx_fail(ctx, PBA_E_NOMEM, "pba_qual: offsets", e); }
    *out = q;
    return PBA_OK;
}

int pba_qual_phred(uint32_t agree, uint64_t n, int qmax) {
    if (qmax < 0 || qmax > PBA_QUAL_QMAX) return -1;
    return qual_phred(agree, n, qmax);
}

int pba_qual_phred_device(pba_ctx *ctx, const uint32_t *agree, const uint64_t *n, uint64_t count, int qmax, uint8_t *qv) {
    if (!ctx || (count && (!agree || !n || !qv))) return PBA_E_INVALID;
    if (qmax < 0 || qmax > PBA_QUAL_QMAX) PBA_FAIL(PBA_E_INVALID, "pba_qual_phred_device: qmax must be in [0, 60]");
    if (!count) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_a, d_n, d_q;
    HIPCHK(hipMalloc(&d_a.p, count * 4));
    HIPCHK(hipMalloc(&d_n.p, count * 8));
    HIPCHK(hipMalloc(&d_q.p, count));
    HIPCHK(hipMemcpyAsync(d_a.p, agree, count * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_n.p, n, count * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_qual_phred, dim3(elem_grid(count, 256)), dim3(256), 0, ctx->stream, d_a.as<uint32_t>(), d_n.as<unsigned long long>(),
                       count, qmax, d_q.as<uint8_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(qv, d_q.p, count, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

int pba_qual_create(pba_ctx *ctx, const uint32_t *lengths, uint32_t n, const uint8_t *qv, const uint16_t *depth, const uint16_t *agree,
                    const uint32_t *src, pba_qual **out) {
    if (!ctx || !out || (n && !lengths)) return PBA_E_INVALID;
    *out = nullptr;
    std::vector<uint64_t> off((size_t)n + 1, 0);
    for (uint32_t s = 0; s < n; ++s) off[s + 1] = off[s] + lengths[s];
    const uint64_t total = off[n];
    if (total >= (1ull << 32)) PBA_FAIL(PBA_E_TOOLONG, "pba_qual_create: 2^32 bases or more");
    if (total && !qv) return PBA_E_INVALID;
    for (uint64_t i = 0; i < total; ++i)
        if (qv[i] > PBA_QUAL_QCAP) PBA_FAIL(PBA_E_INVALID, "pba_qual_create: a qv above 93");
    HIPCHK(hipSetDevice(ctx->device));
    static const size_t width[4] = {1, 2, 2, 4};
    DevBuf d[4];
    for (int a = 0; a < 4; ++a) HIPCHK(hipMalloc(&d[a].p, ((size_t)total + 16) * width[a]));
    std::vector<uint32_t> pos;                                 // src where the caller gives none: the position in its sequence
    if (!src && total) {
        pos.resize((size_t)total);
        for (uint32_t s = 0; s < n; ++s)
            for (uint32_t j = 0; j < lengths[s]; ++j) pos[(size_t)off[s] + j] = j;
    }
    const void *from[4] = {qv, depth, agree, src ? (const void *)src : (const void *)pos.data()};
    for (int a = 0; a < 4 && total; ++a) {
        if (from[a]) HIPCHK(hipMemcpyAsync(d[a].p, from[a], (size_t)total * width[a], hipMemcpyHostToDevice, ctx->stream));
        else HIPCHK(memset_big(d[a].p, 0, (size_t)total * width[a], ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));                 // (pos dies with this scope)
    void *arr[4] = {d[0].p, d[1].p, d[2].p, d[3].p};
    for (int a = 0; a < 4; ++a) d[a].p = nullptr;
    return qual_adopt(ctx, n, off.data(), arr, out);
}

uint32_t pba_qual_count(const pba_qual *q) { return q ? q->n : 0; }

int pba_qual_lengths(const pba_qual *q, uint32_t *len, uint32_t cap) {
    if (!q || (!len && q->n) || cap < q->n) return PBA_E_INVALID;
    for (uint32_t s = 0; s < q->n; ++s) len[s] = (uint32_t)(q->h_off[s + 1] - q->h_off[s]);
    return PBA_OK;
}

int pba_qual_get(pba_ctx *ctx, const pba_qual *q, uint32_t lo, uint32_t hi, uint8_t *qv, uint16_t *depth, uint16_t *agree, uint32_t *src,
                 uint64_t cap, uint64_t *n) {
    if (!ctx || !q || !n || lo > hi || hi > q->n) return PBA_E_INVALID;
    const uint64_t at = q->h_off[lo], cnt = q->h_off[hi] - at;
    *n = cnt;
    if (cap < cnt) PBA_FAIL(PBA_E_INVALID, "pba_qual_get: buffers smaller than the range");
    if (!cnt) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    if (qv) HIPCHK(hipMemcpyAsync(qv, q->d_qv + at, cnt, hipMemcpyDeviceToHost, ctx->stream));
    if (depth) HIPCHK(hipMemcpyAsync(depth, q->d_depth + at, cnt * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (agree) HIPCHK(hipMemcpyAsync(agree, q->d_agree + at, cnt * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (src) HIPCHK(hipMemcpyAsync(src, q->d_src + at, cnt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

int pba_qual_summary(pba_ctx *ctx, const pba_qual *q, int qmin, pba_qual_row *rows, uint32_t cap) {
    if (!ctx || !q || (!rows && q->n) || cap < q->n) return PBA_E_INVALID;
    if (qmin < 0 || qmin > PBA_QUAL_QCAP + 1) PBA_FAIL(PBA_E_INVALID, "pba_qual_summary: qmin must be in [0, 94]");
    if (!q->n) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_tiles, d_rows;
    uint32_t n_tiles = 0;
    PBA_TRY(qual_tiles(ctx, q, &d_tiles, &n_tiles));
    HIPCHK(hipMalloc(&d_rows.p, sizeof(pba_qual_row) * (size_t)q->n));
    hipLaunchKernelGGL(k_qual_rows_init, dim3((q->n + 255) / 256), dim3(256), 0, ctx->stream, q->d_off, q->n, d_rows.as<pba_qual_row>());
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += kQualSlice)
        hipLaunchKernelGGL(k_qual_summary, dim3(std::min(kQualSlice, n_tiles - t0)), dim3(256), 0, ctx->stream, qual_dev(q),
                           d_tiles.as<QTile>(), t0, qmin, d_rows.as<pba_qual_row>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rows, d_rows.p, sizeof(pba_qual_row) * (size_t)q->n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

int pba_qual_low_spans(pba_ctx *ctx, const pba_qual *q, int qmin, int min_run, pba_qual_span *out, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !q || !n_out || (!out && cap)) return PBA_E_INVALID;
    *n_out = 0;
    if (qmin < 0 || qmin > PBA_QUAL_QCAP + 1) PBA_FAIL(PBA_E_INVALID, "pba_qual_low_spans: qmin must be in [0, 94]");
    if (min_run < 1) PBA_FAIL(PBA_E_INVALID, "pba_qual_low_spans: min_run must be at least 1");
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_tiles, d_cnt, d_raw, d_keep, d_out;
    uint32_t n_tiles = 0;
    PBA_TRY(qual_tiles(ctx, q, &d_tiles, &n_tiles));
    if (!n_tiles) return PBA_OK;
    // ---- heads and tails per tile, one scan over both
    const uint64_t n_cnt = 2ull * n_tiles;
    HIPCHK(hipMalloc(&d_cnt.p, sizeof(uint32_t) * (n_cnt + scan_scratch_words(n_cnt))));
    uint32_t *cnt = d_cnt.as<uint32_t>();
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += kQualSlice)
        hipLaunchKernelGGL(k_span_count, dim3(std::min(kQualSlice, n_tiles - t0)), dim3(256), 0, ctx->stream, qual_dev(q), d_tiles.as<QTile>(),
                           t0, n_tiles, qmin, cnt);
    scan_inclusive(ctx, cnt, n_cnt, cnt + n_cnt);
    uint32_t n_runs = 0;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&n_runs, cnt + n_tiles - 1, sizeof n_runs, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!n_runs) return PBA_OK;
    // ---- every run's (seq, beg), end and smallest qv
    HIPCHK(hipMalloc(&d_raw.p, sizeof(pba_qual_span) * (size_t)n_runs));
    HIPCHK(memset_big(d_raw.p, 0x7F, sizeof(pba_qual_span) * (size_t)n_runs, ctx->stream));
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += kQualSlice)
        hipLaunchKernelGGL(k_span_emit, dim3(std::min(kQualSlice, n_tiles - t0)), dim3(256), 0, ctx->stream, qual_dev(q), d_tiles.as<QTile>(),
                           t0, n_tiles, qmin, cnt, d_raw.as<pba_qual_span>());
    // ---- the runs of min_run bases or more, in order
    HIPCHK(hipMalloc(&d_keep.p, sizeof(uint32_t) * ((size_t)n_runs + scan_scratch_words(n_runs))));
    uint32_t *keep = d_keep.as<uint32_t>();
    const uint64_t n_room = std::min<uint64_t>(cap, n_runs);
    HIPCHK(hipMalloc(&d_out.p, sizeof(pba_qual_span) * (size_t)std::max<uint64_t>(n_room, 1)));
    const dim3 run_grid((n_runs + 255) / 256);
    hipLaunchKernelGGL(k_span_keep, run_grid, dim3(256), 0, ctx->stream, d_raw.as<pba_qual_span>(), n_runs, min_run, keep);
    scan_inclusive(ctx, keep, n_runs, keep + n_runs);
    hipLaunchKernelGGL(k_span_compact, run_grid, dim3(256), 0, ctx->stream, d_raw.as<pba_qual_span>(), n_runs, keep, d_out.as<pba_qual_span>(),
                       n_room);
    HIPCHK(hipGetLastError());
    uint32_t n_kept = 0;
    HIPCHK(hipMemcpyAsync(&n_kept, keep + n_runs - 1, sizeof n_kept, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *n_out = n_kept;
    const uint64_t n_copy = std::min<uint64_t>(n_kept, cap);
    if (n_copy) {
        HIPCHK(hipMemcpyAsync(out, d_out.p, sizeof(pba_qual_span) * (size_t)n_copy, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return PBA_OK;
}

int pba_seqs_write_fastq(pba_ctx *ctx, const pba_seqs *s, const pba_qual *qual, uint32_t lo, uint32_t hi, const char *names,
                         const uint64_t *name_off, char *out, uint64_t cap, uint64_t *n_bytes) {
    if (!ctx || !s || !qual || !n_bytes || lo > hi || hi > s->n || (names == nullptr) != (name_off == nullptr)) return PBA_E_INVALID;
    *n_bytes = 0;
    bool same = qual->n == s->n;
    for (uint32_t k = 0; same && k < s->n; ++k) same = qual->h_off[k + 1] - qual->h_off[k] == s->h_len[k];
    if (!same) PBA_FAIL(PBA_E_INVALID, "pba_seqs_write_fastq: the evidence differs from the set in count or lengths");
    const uint32_t n = hi - lo;
    // the size, and where everything goes: host arithmetic from the lengths
    std::vector<uint64_t> cpre((size_t)n + 1), body((size_t)n + 1);
    uint64_t at = 0, chunks = 0;
    char num[16];
    for (uint32_t k = 0; k < n; ++k) {
        if (name_off && name_off[k + 1] < name_off[k]) PBA_FAIL(PBA_E_INVALID, "pba_seqs_write_fastq: name_off must be non-decreasing");
        const uint64_t nl = name_off ? name_off[k + 1] - name_off[k] : (uint64_t)snprintf(num, sizeof num, "%u", lo + k);
        const uint64_t L = s->h_len[lo + k];
        cpre[k] = chunks; body[k] = at + nl + 2;
        at = body[k] + 2 * L + 4;                                 // bases '\n' '+' '\n' quals '\n'
        chunks += std::max<uint64_t>(1, (L + FQ_RUN - 1) / FQ_RUN);
    }
    cpre[n] = chunks; body[n] = at;
    *n_bytes = at;
    if (!out) return PBA_OK;
    if (cap < at) PBA_FAIL(PBA_E_INVALID, "pba_seqs_write_fastq: buffer smaller than the image");
    if (!at) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t *img = nullptr;
    uint64_t *d_pre = nullptr;
    POOL(POOL_FX_IMG, at, img);
    POOL(POOL_FX_RECS, sizeof(uint64_t) * 2 * ((size_t)n + 1), d_pre);
    uint64_t *d_body = d_pre + n + 1;
    HIPCHK(hipMemcpyAsync(d_pre, cpre.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_body, body.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_fq_write, dim3(elem_grid(chunks, 256)), dim3(256), 0, ctx->stream, s->d_packed, s->d_off, s->d_len, qual->d_qv,
                       qual->d_off, lo, n, d_pre, d_body, chunks, img);
    HIPCHK(hipGetLastError());
    for (uint64_t p = 0; p < at; p += kFqPiece)                  // (one copy of the image, in pieces a copy call is known to take)
        HIPCHK(hipMemcpyAsync(out + p, img + p, std::min(kFqPiece, at - p), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (uint32_t k = 0; k < n; ++k) {                            // the header lines, into the gaps
        const uint64_t nl = name_off ? name_off[k + 1] - name_off[k] : (uint64_t)snprintf(num, sizeof num, "%u", lo + k);
        char *h = out + body[k] - nl - 2;
        h[0] = '@';
        memcpy(h + 1, name_off ? names + name_off[k] : num, nl);
        h[1 + nl] = '\n';
    }
    return PBA_OK;
}

void pba_qual_destroy(pba_qual *q) {
    if (!q) return;
    (void)hipSetDevice(q->device);
    qual_free(q);
}

}  // extern "C"
