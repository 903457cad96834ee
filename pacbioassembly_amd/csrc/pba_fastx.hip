// pba_fastx.hip -- FASTA / FASTQ into a sequence set, and a set back out as FASTA (include/pba.h).
// The file image goes up piece by piece as it is.  Per piece, on the device:
//   k_fx_count    the '\n' of every 4 KB tile (16 bytes per lane), scanned over the tiles (seed_index.h: k_scan_*)
//   k_fx_lines    the same bytes again, a workgroup scan of the lanes' counts: start[] of every line (u32, n_lines + 1 entries)
//   k_fx_classify one lane per line: header / sequence line / bytes of sequence, the last non-blank line (atomicMax);
//                 scanned: headers in front of a line (its record), sequence lines and bases in front of it
//   k_fx_check    one lane per line: the structural rules, the first offending line by atomicMin; FASTA: the header line of
//                 every record
//   k_fx_records  one lane per record: its pba_fastx_rec and its offset in the text
//   k_fx_gather   16 bases of the text per thread, its line by bisection over the bases in front of the lines, case folded
// The rules themselves are fastx_lines.h's.  The gathered text and its u64 offsets go to seqs_pack (pba_core.hip): the set is
// what pba_seqs_from_text makes of the same sequences, and there is no second packer.
// pba_seqs_write_fasta: k_fx_write puts bases and line ends of a range of sequences into a device image (64 bases of one
// sequence per thread, the sequence by bisection over a prefix of chunk counts), one copy brings it out, the host writes the
// header lines into the gaps.
#include "pba_host.h"
#include "fastx_lines.h"

#define FX_TILE 4096                       // bytes of the image per workgroup of k_fx_count / k_fx_lines: 256 lanes x 16
#define FX_RUN 64                          // bases per thread of k_fx_write
static const uint64_t kFxPiece = (uint64_t)1 << 30;   // the default piece, and the largest: counters inside a piece are 32-bit

static_assert(sizeof(pba_fastx_rec) == sizeof(FxRec) && sizeof(FxRec) == 40, "pba_fastx_rec is FxRec");

// ---------------------------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------------------------
// bit k set: byte pos + k of the image is '\n' (pos: a multiple of 16; the buffer is readable to the next multiple of 16 past n)
__device__ __forceinline__ uint32_t fx_nl_mask(const uint8_t *f, uint32_t pos, uint32_t n) {
    if (pos >= n) return 0;
    const uint4 v = *reinterpret_cast<const uint4 *>(f + pos);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x = w[k] ^ 0x0A0A0A0Au;
        uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
        t = ~(t | x | 0x7F7F7F7Fu);                              // 0x80 in every byte that was '\n', nowhere else
        m |= (((t >> 7) * 0x10204080u) >> 28) << (4 * k);         // bits 0, 8, 16, 24 -> 0 .. 3
    }
    if (n - pos < 16) m &= (1u << (n - pos)) - 1u;
    return m;
}

// the lanes' values summed over the workgroup of 256 (excl: what the lanes in front of this one hold)
__device__ __forceinline__ uint32_t fx_block_scan(uint32_t v, uint32_t *excl, uint32_t *wsum /* LDS, 4 */) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(inc, d, 64); if (lane >= d) inc += t; }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t carry = 0, total = 0;
    for (int k = 0; k < 4; ++k) { if (k < w) carry += wsum[k]; total += wsum[k]; }
    *excl = carry + inc - v;
    return total;
}

__global__ void __launch_bounds__(256)
k_fx_count(const uint8_t *f, uint32_t n, uint32_t *cnt1) {      // cnt1[t] = the '\n' of tile t
    __shared__ uint32_t wsum[4];
    const uint32_t pos = blockIdx.x * FX_TILE + threadIdx.x * 16;
    uint32_t excl;
    const uint32_t total = fx_block_scan(__popc(fx_nl_mask(f, pos, n)), &excl, wsum);
    if (threadIdx.x == 0) cnt1[blockIdx.x] = total;
}

// tile_excl[t] = the '\n' in front of tile t; start[0] = 0, start[k + 1] = the byte behind the k-th '\n', start[n_lines] = n
__global__ void __launch_bounds__(256)
k_fx_lines(const uint8_t *f, uint32_t n, const uint32_t *tile_excl, uint32_t n_lines, uint32_t *start) {
    __shared__ uint32_t wsum[4];
    const uint32_t pos = blockIdx.x * FX_TILE + threadIdx.x * 16;
    uint32_t m = fx_nl_mask(f, pos, n), excl;
    (void)fx_block_scan(__popc(m), &excl, wsum);
    uint32_t at = tile_excl[blockIdx.x] + excl + 1;
    while (m) {
        const int b = __ffs(m) - 1;
        m &= m - 1;
        if (at <= n_lines) start[at] = pos + b + 1;               // (at <= n_lines always: the guard costs nothing)
        ++at;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { start[0] = 0; start[n_lines] = n; }
}

// Arrays with one slot in front: x1[0] = 0, x1[L + 1] = line L's value; after the inclusive scan of x1 + 1, x1[L] is what
// lies in front of line L and x1[n_lines] the total.
__global__ void __launch_bounds__(256)
k_fx_classify(const uint8_t *f, const uint32_t *start, uint32_t n_lines, int format, uint32_t *hdr1, uint32_t *sq1, uint32_t *by1,
              uint32_t *last_nb1) {
    const uint32_t L = blockIdx.x * 256 + threadIdx.x;
    uint32_t nb = 0;
    if (L < n_lines) {
        const uint32_t s = start[L], clen = fx_content_len(f, s, start[L + 1]);
        if (format == FX_FASTA) {
            const int kind = fx_fasta_kind(f, s, clen);
            hdr1[L + 1] = kind == FX_HEADER;
            sq1[L + 1] = kind == FX_SEQ;
            by1[L + 1] = kind == FX_SEQ ? clen : 0u;
            if (L == 0) hdr1[0] = sq1[0] = 0;
        } else
            by1[L + 1] = (L & 3u) == 1u ? clen : 0u;
        if (L == 0) by1[0] = 0;
        if (clen) nb = L + 1;
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) nb = max(nb, (uint32_t)__shfl_xor((int)nb, d, 64));
    if ((threadIdx.x & 63) == 0 && nb) atomicMax(last_nb1, nb);
}

__global__ void __launch_bounds__(256)
k_fx_check(const uint8_t *f, const uint32_t *start, uint32_t n_lines, int format, const uint32_t *hdr1, uint32_t n_eff, uint32_t n_rec,
           uint32_t *rec_line, uint32_t *bad) {
    const uint32_t L = blockIdx.x * 256 + threadIdx.x;
    if (L == 0 && format == FX_FASTA) rec_line[n_rec] = n_lines;
    if (L >= n_lines) return;
    const uint32_t s = start[L], clen = fx_content_len(f, s, start[L + 1]);
    bool is_bad;
    if (format == FX_FASTA) {
        const int kind = fx_fasta_kind(f, s, clen);
        is_bad = fx_fasta_bad(kind, hdr1[L]);
        if (kind == FX_HEADER && hdr1[L] < n_rec) rec_line[hdr1[L]] = L;
    } else {
        if (L >= n_eff) return;
        const uint32_t seq_clen = (L & 3u) == 3u ? fx_content_len(f, start[L - 2], start[L - 1]) : 0u;
        is_bad = fx_fastq_bad(L & 3u, clen, clen ? f[s] : (uint8_t)0, seq_clen);
    }
    if (is_bad) atomicMin(bad, L);
}

// recs[r]: offsets made global by `base`; toff[r] = text_base + the bases in front of the record, toff[n_rec] the end
__global__ void __launch_bounds__(256)
k_fx_records(const uint8_t *f, const uint32_t *start, uint32_t n_lines, int format, const uint32_t *sq1, const uint32_t *by1,
             const uint32_t *rec_line, uint32_t n_rec, uint64_t base, uint64_t text_base, pba_fastx_rec *recs, uint64_t *toff) {
    const uint32_t r = blockIdx.x * 256 + threadIdx.x;
    if (r == 0) toff[n_rec] = text_base + by1[n_lines];
    if (r >= n_rec) return;
    FxRec x;
    uint32_t h;
    if (format == FX_FASTA) {
        h = rec_line[r];
        const uint32_t hn = rec_line[r + 1];
        x = fx_fasta_rec(f, start, h, hn, by1[hn] - by1[h], sq1[hn] - sq1[h]);
    } else {
        h = 4 * r;
        x = fx_fastq_rec(f, start, r);
        x.qual_off += base;
    }
    x.hdr_off += base; x.seq_off += base;
    pba_fastx_rec o;
    o.hdr_off = x.hdr_off; o.seq_off = x.seq_off; o.qual_off = x.qual_off;
    o.hdr_len = x.hdr_len; o.name_len = x.name_len; o.seq_len = x.seq_len; o.n_seq_lines = x.n_seq_lines;
    recs[r] = o;
    toff[r] = text_base + by1[h];
}

// Thread t owns the 16 bytes of the text at (text_base & ~15) + 16 t that lie in [text_base, text_base + nb): the piece's
// bases.  by1: the bases in front of every line (entry n_lines: nb).
__global__ void __launch_bounds__(256)
k_fx_gather(const uint8_t *f, const uint32_t *start, const uint32_t *by1, uint32_t n_lines, uint32_t nb, uint8_t *text, uint64_t text_base,
            int keep, uint32_t *folded) {
    const uint64_t g0 = (text_base & ~15ull) + ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const uint64_t glo = max(g0, text_base), ghi = min(g0 + 16, text_base + nb);
    uint32_t nf = 0;
    if (glo < ghi) {
        uint32_t b = (uint32_t)(glo - text_base);
        const uint32_t e = (uint32_t)(ghi - text_base);
        uint32_t lo = 0, hi = n_lines - 1;                        // the first line L with by1[L + 1] > b
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (by1[mid + 1] > b) hi = mid; else lo = mid + 1;
        }
        uint32_t L = lo, k = 0;
        uint64_t w0 = 0, w1 = 0;
        while (b < e) {
            const uint32_t in_line = b - by1[L], have = by1[L + 1] - by1[L] - in_line;
            if (!have) { ++L; continue; }
            const uint32_t take = min(have, e - b);
            const uint8_t *src = f + start[L] + in_line;
            for (uint32_t i = 0; i < take; ++i, ++k) {
                const uint64_t c = fx_fold(src[i], keep != 0, &nf);
                if (k < 8) w0 |= c << (8 * k); else w1 |= c << (8 * (k - 8));
            }
            b += take;
        }
        if (k == 16) {
            uint4 v;
            v.x = (uint32_t)w0; v.y = (uint32_t)(w0 >> 32); v.z = (uint32_t)w1; v.w = (uint32_t)(w1 >> 32);
            *reinterpret_cast<uint4 *>(text + g0) = v;            // (text: 256-byte aligned, g0 a multiple of 16)
        } else
            for (uint32_t i = 0; i < k; ++i) text[glo + i] = (uint8_t)((i < 8 ? w0 >> (8 * i) : w1 >> (8 * (i - 8))) & 0xFF);
    }
#pragma unroll
    for (int d = 32; d; d >>= 1) nf += (uint32_t)__shfl_xor((int)nf, d, 64);
    if ((threadIdx.x & 63) == 0 && nf) atomicAdd(folded, nf);
}

// Thread t owns chunk t: FX_RUN bases of one sequence of [lo, lo + n) -- sequence lo + s, the last s with cpre[s] <= t (cpre:
// the chunks in front of every sequence, entry n the total).  body[s]: where the sequence's first base goes in the image.
__global__ void __launch_bounds__(256)
k_fx_write(const uint8_t *packed, const uint64_t *off, const uint32_t *len, uint32_t first, uint32_t n, const uint64_t *cpre,
           const uint64_t *body, uint32_t width, uint64_t total_chunks, uint8_t *img) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_chunks; t += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cpre[mid] <= t) lo = mid; else hi = mid;
        }
        const uint32_t s = lo, L = len[first + s];
        const uint64_t j0 = (t - cpre[s]) * FX_RUN;
        if (j0 >= L) continue;
        const uint8_t *src = packed + off[first + s];
        const uint32_t cnt = (uint32_t)min((uint64_t)FX_RUN, (uint64_t)L - j0);
        uint32_t q = width ? (uint32_t)(j0 / width) : 0u, r = width ? (uint32_t)(j0 % width) : 0u;   // line and column of base j
        uint8_t *dst = img + body[s];
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t j = (uint32_t)j0 + k;
            const uint32_t code = (src[j >> 2] >> (6 - 2 * (j & 3))) & 3u;
            const uint64_t p = (uint64_t)j + q;
            dst[p] = code == 0 ? 'A' : code == 1 ? 'C' : code == 2 ? 'G' : 'T';
            bool eol = j == L - 1;
            if (width && ++r == width) { r = 0; ++q; eol = true; }
            if (eol) dst[p + 1] = '\n';
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
struct pba_fastx_index {
    std::vector<pba_fastx_rec> recs;
};

// the u64 text offsets of the records parsed so far, on the device: grown by doubling
struct FxOffsets {
    DevBuf buf;
    size_t cap = 0;
    int reserve(pba_ctx *ctx, size_t need) {
        if (need <= cap) return PBA_OK;
        const size_t want = std::max<size_t>(std::max<size_t>(need, cap * 2), 1024);
        void *p = nullptr;
        HIPCHK(hipMalloc(&p, want * sizeof(uint64_t)));
        hipError_t e = cap ? copy_d2d(p, buf.p, cap * sizeof(uint64_t), ctx->stream) : hipMemsetAsync(p, 0, sizeof(uint64_t), ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { (void)hipFree(p); return ctx_fail(ctx, PBA_E_HIP, "fastx offsets", e); }
        buf.reset();
        buf.p = p; cap = want;
        return PBA_OK;
    }
};

struct FxRun {                     // one parse
    pba_ctx *ctx;
    int format;                    // FX_FASTA / FX_FASTQ: the rules the kernels apply
    bool keep;
    StageClock clk;
    uint8_t *d_text;
    FxOffsets toff;
    pba_fastx_index *idx;
    pba_fastx_stats st;
    uint64_t text_base = 0, line_base = 0;
};

static int fx_invalid(pba_ctx *ctx, uint64_t line1, const char *what) {
    snprintf(ctx->err, sizeof ctx->err, "pba_seqs_from_fastx: line %llu: %s", (unsigned long long)line1, what);
    return PBA_E_INVALID;
}

// one piece: bytes [base, base + P) of the file, 0 < P <= kFxPiece; last: nothing of the file lies behind it
static int fx_piece(FxRun &R, const uint8_t *piece, uint32_t P, uint64_t base, bool last) {
    pba_ctx *ctx = R.ctx;
    const int format = R.format;
    uint8_t *d_file = nullptr;
    POOL(POOL_FX_FILE, ((size_t)P + 15) / 16 * 16 + 16, d_file);
    {
        auto sc = R.clk.time(ctx->stream, &R.st.h2d_ms);
        HIPCHK(hipMemcpyAsync(d_file, piece, P, hipMemcpyHostToDevice, ctx->stream));
    }
    auto sc = R.clk.time(ctx->stream, &R.st.parse_ms);
    // ---- the line table
    const uint32_t n_tiles = (P + FX_TILE - 1) / FX_TILE;
    uint32_t *cnt = nullptr;                                     // [n_tiles + 1] shifted counts, scan scratch, 4 words: last_nb1, bad, folded
    POOL(POOL_FX_TILES, sizeof(uint32_t) * ((size_t)n_tiles + 1 + scan_scratch_words(n_tiles) + 4), cnt);
    uint32_t *scr = cnt + n_tiles + 1, *small = scr + scan_scratch_words(n_tiles);
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(small, 0, 4 * sizeof(uint32_t), ctx->stream));
    HIPCHK(hipMemsetAsync(small + 1, 0xFF, sizeof(uint32_t), ctx->stream));      // FX_NO_LINE
    hipLaunchKernelGGL(k_fx_count, dim3(n_tiles), dim3(256), 0, ctx->stream, d_file, P, cnt + 1);
    scan_inclusive(ctx, cnt + 1, n_tiles, scr);
    uint32_t n_nl = 0;
    HIPCHK(hipMemcpyAsync(&n_nl, cnt + n_tiles, sizeof n_nl, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    const uint32_t n_lines = n_nl + (piece[P - 1] != '\n');     // a last line without '\n' is a line (P <= 2^30: no overflow)
    const size_t n1 = (size_t)n_lines + 1;
    uint32_t *start = nullptr;
    POOL(POOL_FX_LINES, sizeof(uint32_t) * (4 * n1 + scan_scratch_words(n_lines)), start);
    uint32_t *hdr1 = start + n1, *sq1 = hdr1 + n1, *by1 = sq1 + n1, *scr2 = by1 + n1;
    const uint32_t line_grid = (n_lines + 255) / 256;
    hipLaunchKernelGGL(k_fx_lines, dim3(n_tiles), dim3(256), 0, ctx->stream, d_file, P, cnt, n_lines, start);
    // ---- per line
    hipLaunchKernelGGL(k_fx_classify, dim3(line_grid), dim3(256), 0, ctx->stream, d_file, start, n_lines, format, hdr1, sq1, by1, small);
    if (format == FX_FASTA) { scan_inclusive(ctx, hdr1 + 1, n_lines, scr2); scan_inclusive(ctx, sq1 + 1, n_lines, scr2); }
    scan_inclusive(ctx, by1 + 1, n_lines, scr2);
    uint32_t n_hdr = 0, nb = 0, last_nb1 = 0;
    if (format == FX_FASTA) HIPCHK(hipMemcpyAsync(&n_hdr, hdr1 + n_lines, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&nb, by1 + n_lines, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&last_nb1, small, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    const uint32_t n_eff = format == FX_FASTQ ? fx_fastq_neff(last_nb1, n_lines, last) : n_lines;
    const uint32_t n_rec = format == FX_FASTQ ? n_eff / 4 : n_hdr;
    const uint32_t bad_host = format == FX_FASTQ ? fx_fastq_truncated(n_eff) : FX_NO_LINE;
    const size_t rec_base = R.idx->recs.size();
    if (rec_base + n_rec > 0x7FFFFFFFull) PBA_FAIL(PBA_E_TOOLONG, "pba_seqs_from_fastx: more than 0x7FFFFFFF records");
    if (R.text_base + nb > R.st.n_bytes) PBA_FAIL(PBA_E_HIP, "pba_seqs_from_fastx: more bases than bytes");   // (cannot happen: guards the text buffer)
    // ---- per record
    pba_fastx_rec *d_recs = nullptr;
    POOL(POOL_FX_RECS, sizeof(pba_fastx_rec) * (size_t)n_rec + sizeof(uint32_t) * ((size_t)n_rec + 1), d_recs);
    uint32_t *rec_line = (uint32_t *)(d_recs + n_rec);
    PBA_TRY(R.toff.reserve(ctx, rec_base + n_rec + 1));
    uint64_t *toff = R.toff.buf.as<uint64_t>() + rec_base;
    hipLaunchKernelGGL(k_fx_check, dim3(line_grid), dim3(256), 0, ctx->stream, d_file, start, n_lines, format, hdr1, n_eff, n_rec, rec_line,
                       small + 1);
    hipLaunchKernelGGL(k_fx_records, dim3(std::max(1u, (n_rec + 255) / 256)), dim3(256), 0, ctx->stream, d_file, start, n_lines, format, sq1,
                       by1, rec_line, n_rec, base, R.text_base, d_recs, toff);
    // ---- the bases
    if (nb) {
        const uint64_t chunks = ((R.text_base & 15) + nb + 15) / 16;
        hipLaunchKernelGGL(k_fx_gather, dim3((uint32_t)((chunks + 255) / 256)), dim3(256), 0, ctx->stream, d_file, start, by1, n_lines, nb,
                           R.d_text, R.text_base, R.keep ? 1 : 0, small + 2);
    }
    uint32_t got[4] = {0, 0, 0, 0};
    R.idx->recs.resize(rec_base + n_rec);
    HIPCHK(hipMemcpyAsync(got, small, sizeof got, hipMemcpyDeviceToHost, ctx->stream));
    if (n_rec) HIPCHK(hipMemcpyAsync(R.idx->recs.data() + rec_base, d_recs, sizeof(pba_fastx_rec) * (size_t)n_rec, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    const uint32_t bad = std::min(got[1], bad_host);
    if (bad != FX_NO_LINE) {
        const char *what = format == FX_FASTA ? "text before the first '>' header"
                           : bad >= n_eff     ? "the last record is truncated"
                           : (bad & 3u) == 0  ? "a record must start with '@' (blank lines only after the last record)"
                           : (bad & 3u) == 2  ? "the third line of a record must start with '+'"
                                              : "quality and sequence differ in length";
        return fx_invalid(ctx, R.line_base + bad + 1, what);
    }
    R.text_base += nb; R.line_base += n_lines;
    R.st.n_lines += n_lines; R.st.n_bases += nb; R.st.n_folded += got[2];
    ++R.st.n_pieces;
    return PBA_OK;
}

static int fx_parse(pba_ctx *ctx, const uint8_t *file, uint64_t file_len, int format, uint32_t flags, pba_seqs **out,
                    pba_fastx_index **index, pba_fastx_stats *stats, uint64_t max_piece) {
    if (format != PBA_FX_AUTO && format != PBA_FX_FASTA && format != PBA_FX_FASTQ) PBA_FAIL(PBA_E_INVALID, "pba_seqs_from_fastx: unknown format");
    if (flags & ~(PBA_FX_KEEP_CASE | PBA_FX_STRICT_ACGT)) PBA_FAIL(PBA_E_INVALID, "pba_seqs_from_fastx: unknown flag");
    HIPCHK(hipSetDevice(ctx->device));
    int fmt = format;
    if (fmt == PBA_FX_AUTO) {
        uint64_t line = 0;
        fmt = fx_sniff(file, file_len, nullptr, &line);
        if (fmt < 0) return fx_invalid(ctx, line + 1, "neither '>' nor '@' starts the first non-blank line");
    }
    const uint64_t budget = max_piece ? std::min(max_piece, kFxPiece) : kFxPiece;
    std::unique_ptr<pba_fastx_index> idx(new (std::nothrow) pba_fastx_index());
    if (!idx) PBA_FAIL(PBA_E_NOMEM, "pba_fastx_index");
    FxRun R;
    R.ctx = ctx; R.format = fmt ? fmt : FX_FASTA;                 // (no non-blank line: either format's rules find 0 records)
    R.keep = (flags & PBA_FX_KEEP_CASE) != 0;
    R.idx = idx.get();
    memset(&R.st, 0, sizeof R.st);
    R.st.format = fmt; R.st.n_bytes = file_len;
    if (!R.clk.init()) PBA_FAIL(PBA_E_HIP, "hipEventCreate");
    DevBuf text;                                                  // bases never outnumber file bytes
    HIPCHK(hipMalloc(&text.p, file_len + kSlack));
    R.d_text = text.as<uint8_t>();
    PBA_TRY(R.toff.reserve(ctx, 1));
    for (uint64_t pos = 0; pos < file_len;) {
        const uint64_t c = fx_cut(file + pos, file_len - pos, R.format, budget);
        if (!c) {
            uint64_t at = 0;
            (void)fx_sniff(file + pos, file_len - pos, &at);
            snprintf(ctx->err, sizeof ctx->err, "pba_seqs_from_fastx: the record at hdr_off %llu is longer than a piece of %llu bytes",
                     (unsigned long long)(pos + at), (unsigned long long)budget);
            return PBA_E_TOOLONG;
        }
        PBA_TRY(fx_piece(R, file + pos, (uint32_t)c, pos, pos + c == file_len));
        pos += c;
    }
    const size_t n = idx->recs.size();
    std::vector<uint64_t> h_toff(n + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        if (idx->recs[i].seq_len >= 0x7FFFFFF0u) PBA_FAIL(PBA_E_TOOLONG, "pba_seqs_from_fastx: a record of 0x7FFFFFF0 bases or more");
        h_toff[i + 1] = h_toff[i] + idx->recs[i].seq_len;
    }
    {
        auto sc = R.clk.time(ctx->stream, &R.st.pack_ms);
        const int st = seqs_pack(ctx, R.d_text, R.toff.buf.as<uint64_t>(), h_toff.data(), (uint32_t)n, (flags & PBA_FX_STRICT_ACGT) ? 1 : 0, out);
        if (st == PBA_E_ALPHABET) PBA_FAIL(PBA_E_ALPHABET, "pba_seqs_from_fastx: a base outside ACGT under PBA_FX_STRICT_ACGT");
        if (st != PBA_OK) return st;
    }
    R.st.n_records = (uint32_t)n; R.st.max_len = (*out)->max_len;
    if (stats) *stats = R.st;
    if (index) *index = idx.release();
    return PBA_OK;
}

extern "C" {

int pba_seqs_from_fastx_budget(pba_ctx *ctx, const void *file, uint64_t file_len, int format, uint32_t flags, pba_seqs **out,
                               pba_fastx_index **index, pba_fastx_stats *stats, uint64_t max_piece_bytes) {
    if (!ctx || !out || (!file && file_len)) return PBA_E_INVALID;
    *out = nullptr;
    if (index) *index = nullptr;
    if (stats) memset(stats, 0, sizeof *stats);
    return fx_parse(ctx, (const uint8_t *)file, file_len, format, flags, out, index, stats, max_piece_bytes);
}

int pba_seqs_from_fastx(pba_ctx *ctx, const void *file, uint64_t file_len, int format, uint32_t flags, pba_seqs **out,
                        pba_fastx_index **index, pba_fastx_stats *stats) {
    return pba_seqs_from_fastx_budget(ctx, file, file_len, format, flags, out, index, stats, 0);
}

uint32_t pba_fastx_index_count(const pba_fastx_index *index) { return index ? (uint32_t)index->recs.size() : 0; }

int pba_fastx_index_recs(const pba_fastx_index *index, pba_fastx_rec *out, uint32_t cap) {
    if (!index || (!out && !index->recs.empty()) || cap < index->recs.size()) return PBA_E_INVALID;
    if (!index->recs.empty()) memcpy(out, index->recs.data(), sizeof(pba_fastx_rec) * index->recs.size());
    return PBA_OK;
}

void pba_fastx_index_destroy(pba_fastx_index *index) { delete index; }

int pba_fastx_sniff(const void *file, uint64_t file_len) {
    if (!file && file_len) return PBA_E_INVALID;
    const int f = fx_sniff((const uint8_t *)file, file_len);
    return f < 0 ? PBA_E_INVALID : f;
}

int pba_fastx_cut(const void *file, uint64_t file_len, int format, uint64_t want, uint64_t *cut) {
    if (!cut || (!file && file_len) || (format != PBA_FX_AUTO && format != PBA_FX_FASTA && format != PBA_FX_FASTQ)) return PBA_E_INVALID;
    if (format == PBA_FX_AUTO) {
        format = fx_sniff((const uint8_t *)file, file_len);
        if (format < 0) return PBA_E_INVALID;
        if (!format) format = FX_FASTA;                           // no non-blank line: no '>' either
    }
    *cut = fx_cut((const uint8_t *)file, file_len, format, want);
    return PBA_OK;
}

int pba_seqs_write_fasta(pba_ctx *ctx, const pba_seqs *s, uint32_t lo, uint32_t hi, const char *names, const uint64_t *name_off,
                         uint32_t width, char *out, uint64_t cap, uint64_t *n_bytes) {
    if (!ctx || !s || !n_bytes || lo > hi || hi > s->n || (names == nullptr) != (name_off == nullptr)) return PBA_E_INVALID;
    const uint32_t n = hi - lo;
    // the size, and where everything goes: host arithmetic from the lengths
    std::vector<uint64_t> cpre((size_t)n + 1), body((size_t)n + 1);
    uint64_t at = 0, chunks = 0;
    char num[16];
    for (uint32_t k = 0; k < n; ++k) {
        if (name_off && name_off[k + 1] < name_off[k]) PBA_FAIL(PBA_E_INVALID, "pba_seqs_write_fasta: name_off must be non-decreasing");
        const uint64_t nl = name_off ? name_off[k + 1] - name_off[k] : (uint64_t)snprintf(num, sizeof num, "%u", lo + k);
        const uint64_t L = s->h_len[lo + k];
        cpre[k] = chunks; body[k] = at + nl + 2;
        at = body[k] + L + (width ? (L + width - 1) / width : (L ? 1 : 0));
        chunks += (L + FX_RUN - 1) / FX_RUN;
    }
    cpre[n] = chunks; body[n] = at;
    *n_bytes = at;
    if (!out) return PBA_OK;
    if (cap < at) PBA_FAIL(PBA_E_INVALID, "pba_seqs_write_fasta: buffer smaller than the image");
    if (!at) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    if (chunks) {
        uint8_t *img = nullptr;
        uint64_t *d_pre = nullptr;
        POOL(POOL_FX_IMG, at, img);
        POOL(POOL_FX_RECS, sizeof(uint64_t) * 2 * ((size_t)n + 1), d_pre);
        uint64_t *d_body = d_pre + n + 1;
        HIPCHK(hipMemcpyAsync(d_pre, cpre.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(d_body, body.data(), sizeof(uint64_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_fx_write, dim3(elem_grid(chunks, 256)), dim3(256), 0, ctx->stream, s->d_packed, s->d_off, s->d_len, lo, n, d_pre,
                           d_body, width, chunks, img);
        HIPCHK(hipGetLastError());
        for (uint64_t p = 0; p < at; p += kFxPiece)               // (one copy of the image, in pieces a copy call is known to take)
            HIPCHK(hipMemcpyAsync(out + p, img + p, std::min(kFxPiece, at - p), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    for (uint32_t k = 0; k < n; ++k) {                            // the header lines, into the gaps
        const uint64_t nl = name_off ? name_off[k + 1] - name_off[k] : (uint64_t)snprintf(num, sizeof num, "%u", lo + k);
        char *h = out + body[k] - nl - 2;
        h[0] = '>';
        memcpy(h + 1, name_off ? names + name_off[k] : num, nl);
        h[1 + nl] = '\n';
    }
    return PBA_OK;
}

}  // extern "C"
