// pba_clip.hip -- clipping: reads cut to the span their overlap rows support (pba_clip_*).  Host side; the
// kernels are in clip.h.  One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails
// loudly (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
//
// The reads are cut into consecutive ranges ("chunks") whose difference arenas fit a budget; the rows go to the device once
// (the pooled row buffer the layout uses) and every chunk's k_clip_events walks all of them, skipping the reads outside its
// range; k_clip_sweep then turns each read's arena into its pba_clip_row.  Coverage is a sum, so the answer does not depend
// on the cut.  pba_clip_apply writes the kept intervals as ASCII (k_clip_gather) and packs them as pba_layout_stitch packs
// its contigs.  The work arrays are pooled (POOL_CLIP_*); the object owns the per-read table on the device and its host copy.
#include "pba_host.h"

#include "clip.h"

extern "C" {

struct pba_clip {
    int device;
    uint32_t n;
    std::vector<uint32_t> h_len;
    std::vector<pba_clip_row> h_table;
    std::vector<uint64_t> h_toff;                // text offset of every clipped read, and the total
    DevBuf table;                                // a pba_clip_row per read: k_clip_gather reads the kept begins from it
    mutable pba_clip_stats stats;
};

static const uint64_t kClipMaxEntries = 0x7FFFFFF0ull;       // entries of one chunk's arena: an index inside it is an int

static int clip_check(pba_ctx *ctx, const char *who, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows, int margin,
                      uint32_t flags) {
    if (margin < 0) return ctx_fail_as(ctx, PBA_E_INVALID, who, "margin must be >= 0");
    if (!(flags & (PBA_CLIP_TARGETS | PBA_CLIP_QUERIES))) return ctx_fail_as(ctx, PBA_E_INVALID, who, "neither PBA_CLIP_TARGETS nor PBA_CLIP_QUERIES is set");
    if (flags & ~(PBA_CLIP_TARGETS | PBA_CLIP_QUERIES | PBA_CLIP_KEEP_UNSEEN)) return ctx_fail_as(ctx, PBA_E_INVALID, who, "unknown flag bits");
    return check_overlap_rows(ctx, who, reads, rows, n_rows, false, false);
}

// the entries one chunk's arena may hold: max_bases, or a quarter of the free device memory over 4 bytes an entry
static int clip_budget(pba_ctx *ctx, uint64_t max_bases, uint64_t *budget) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    free_b += ctx->pool[POOL_CLIP_ARENA].cap;                 // the arena kept from earlier calls is ours to reuse
    const uint64_t room = std::min<uint64_t>(kClipMaxEntries, (uint64_t)(free_b / 4) / 4);
    *budget = std::max<uint64_t>(4, max_bases ? std::min<uint64_t>(max_bases, kClipMaxEntries) : room);
    return PBA_OK;
}

static inline void clip_launch_sweep(hipStream_t st, const int *arena, const unsigned long long *cum, uint32_t r_lo, uint32_t r_hi,
                                     const uint32_t *len, const int *niv, int margin, int min_cov, int min_len, uint32_t flags,
                                     pba_clip_row *table, unsigned long long *cnt, int *cov_out) {
    const uint32_t per = 1u << 22;                            // (a launch's global size is a 32-bit number)
    for (uint64_t r = r_lo; r < r_hi; r += per)
        hipLaunchKernelGGL(k_clip_sweep, dim3((uint32_t)std::min<uint64_t>(per, r_hi - r)), dim3(CLIP_THREADS), 0, st, arena, cum, r_lo,
                           (uint32_t)r, len, niv, margin, min_cov, min_len, flags, table, cnt, cov_out);
}

int pba_clip_create(pba_ctx *ctx, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows, int margin, int min_cov,
                    int min_len, uint32_t flags, uint64_t max_bases, pba_clip **out, pba_clip_stats *stats) {
    if (!ctx || !reads || !out || (!rows && n_rows)) return PBA_E_INVALID;
    *out = nullptr;
    if (min_cov < 1) PBA_FAIL(PBA_E_INVALID, "pba_clip_create: min_cov must be >= 1");
    if (min_len < 0) PBA_FAIL(PBA_E_INVALID, "pba_clip_create: min_len must be >= 0");
    PBA_TRY(clip_check(ctx, "pba_clip_create", reads, rows, n_rows, margin, flags));
    HIPCHK(hipSetDevice(ctx->device));
    StageClock clk;
    if (!clk.init()) PBA_FAIL(PBA_E_HIP, "pba_clip_create: hipEventCreate");
    std::unique_ptr<pba_clip, void (*)(pba_clip *)> clip(new (std::nothrow) pba_clip(), pba_clip_destroy);
    if (!clip) PBA_FAIL(PBA_E_NOMEM, "pba_clip");
    const uint32_t n = reads->n;
    const size_t N = std::max<size_t>(n, 1);
    clip->device = ctx->device; clip->n = n;
    clip->h_len.assign(reads->h_len.begin(), reads->h_len.begin() + n);
    clip->h_table.resize(n);
    memset(&clip->stats, 0, sizeof clip->stats);
    pba_clip_stats &s = clip->stats;
    s.n_rows = n_rows;
    hipStream_t st = ctx->stream;

    std::vector<unsigned long long> h_cum((size_t)n + 1, 0ull);
    for (uint32_t r = 0; r < n; ++r) { h_cum[r + 1] = h_cum[r] + clip_entries(clip->h_len[r]); s.n_bases_in += clip->h_len[r]; }
    uint64_t budget = 0;
    PBA_TRY(clip_budget(ctx, max_bases, &budget));
    uint64_t widest = 4;                                      // the largest chunk: the cut is decided on the host, from the lengths
    std::vector<uint32_t> cuts(1, 0);
    for (uint32_t lo = 0; lo < n;) {
        uint32_t hi = lo + 1;
        while (hi < n && h_cum[hi + 1] - h_cum[lo] <= budget) ++hi;
        if (h_cum[hi] - h_cum[lo] > kClipMaxEntries) PBA_FAIL(PBA_E_TOOLONG, "pba_clip_create: a read of 0x7FFFFFF0 bases or more");
        widest = std::max<uint64_t>(widest, h_cum[hi] - h_cum[lo]);
        cuts.push_back(hi);
        lo = hi;
    }
    s.n_chunks = (uint32_t)cuts.size() - 1;

    size_t carve = 0;
    auto take = [&carve](size_t bytes) { const size_t at = carve; carve += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_cum = take(8 * (N + 1)), o_niv = take(4 * N), o_cnt = take(8 * CC_COUNT);
    uint8_t *work = nullptr, *d_rows = nullptr;
    int *arena = nullptr;
    POOL(POOL_CLIP_WORK, carve, work);
    POOL(POOL_CLIP_ARENA, 4 * (size_t)widest, arena);
    POOL(POOL_LAY_ROWS, std::max<size_t>(1, sizeof(pba_strand_overlap) * n_rows), d_rows);
    HIPCHK(hipMalloc(&clip->table.p, sizeof(pba_clip_row) * N));
    const pba_strand_overlap *R = (const pba_strand_overlap *)d_rows;
    unsigned long long *cum = (unsigned long long *)(work + o_cum), *cnt = (unsigned long long *)(work + o_cnt);
    int *niv = (int *)(work + o_niv);
    pba_clip_row *table = clip->table.as<pba_clip_row>();
    unsigned long long h_cnt[CC_COUNT];
    memset(h_cnt, 0, sizeof h_cnt);

    {   // rows and arena offsets up once
        const auto timed = clk.time(st, &s.events_ms);
        if (n_rows) HIPCHK(hipMemcpyAsync(d_rows, rows, sizeof(pba_strand_overlap) * n_rows, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(cum, h_cum.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(niv, 0, 4 * N, st));
        HIPCHK(hipMemsetAsync(cnt, 0, 8 * CC_COUNT, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    for (size_t k = 0; k + 1 < cuts.size(); ++k) {
        const uint32_t lo = cuts[k], hi = cuts[k + 1];
        {   // the chunk's arena cleared, then every row's events for the reads of [lo, hi)
            const auto timed = clk.time(st, &s.events_ms);
            HIPCHK(memset_big(arena, 0, 4 * (size_t)(h_cum[hi] - h_cum[lo]), st));
            if (n_rows) hipLaunchKernelGGL(k_clip_events, dim3(elem_grid(n_rows, 256)), dim3(256), 0, st, R, n_rows, cum, lo, hi, margin, flags,
                                           arena, niv, cnt);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
        }
        {
            const auto timed = clk.time(st, &s.sweep_ms);
            clip_launch_sweep(st, arena, cum, lo, hi, reads->d_len, niv, margin, min_cov, min_len, flags, table, cnt, nullptr);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    if (n) HIPCHK(hipMemcpyAsync(clip->h_table.data(), table, sizeof(pba_clip_row) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    clip->h_toff.assign((size_t)n + 1, 0);
    for (uint32_t r = 0; r < n; ++r) clip->h_toff[r + 1] = clip->h_toff[r] + (uint64_t)(clip->h_table[r].end - clip->h_table[r].beg);
    s.n_iv = h_cnt[CC_IV]; s.n_iv_short = h_cnt[CC_SHORT];
    s.n_dropped = (uint32_t)h_cnt[CC_DROPPED]; s.n_whole = (uint32_t)h_cnt[CC_WHOLE]; s.n_cut = (uint32_t)h_cnt[CC_CUT];
    s.n_multi_run = (uint32_t)h_cnt[CC_MULTI]; s.n_unseen = (uint32_t)h_cnt[CC_UNSEEN];
    s.n_bases_out = clip->h_toff[n];
    if (stats) *stats = s;
    *out = clip.release();
    return PBA_OK;
}

int pba_clip_rows(pba_ctx *ctx, const pba_clip *clip, pba_clip_row *out, uint32_t cap) {
    if (!ctx || !clip) return PBA_E_INVALID;
    if (cap < clip->n || (!out && clip->n)) PBA_FAIL(PBA_E_INVALID, "pba_clip_rows: room for fewer rows than the set has reads");
    if (clip->n) memcpy(out, clip->h_table.data(), sizeof(pba_clip_row) * (size_t)clip->n);
    return PBA_OK;
}

int pba_clip_coverage(pba_ctx *ctx, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows, int margin, uint32_t flags,
                      uint32_t read, int32_t *cov, uint32_t cap, uint32_t *n_out) {
    if (!ctx || !reads || !n_out || (!rows && n_rows) || (!cov && cap)) return PBA_E_INVALID;
    *n_out = 0;
    PBA_TRY(clip_check(ctx, "pba_clip_coverage", reads, rows, n_rows, margin, flags));
    if (read >= reads->n) PBA_FAIL(PBA_E_INVALID, "pba_clip_coverage: no such read");
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = reads->n, L = reads->h_len[read];
    const uint64_t ent = clip_entries(L);
    if (ent > kClipMaxEntries) PBA_FAIL(PBA_E_TOOLONG, "pba_clip_coverage: a read of 0x7FFFFFF0 bases or more");
    // the arena offsets of the whole set, as pba_clip_create uploads them: the kernels are the same, the range is one read
    std::vector<unsigned long long> h_cum((size_t)n + 1, 0ull);
    for (uint32_t r = 0; r < n; ++r) h_cum[r + 1] = h_cum[r] + clip_entries(reads->h_len[r]);
    size_t carve = 0;
    auto take = [&carve](size_t bytes) { const size_t at = carve; carve += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_cum = take(8 * ((size_t)n + 1)), o_niv = take(4 * (size_t)n), o_cnt = take(8 * CC_COUNT), o_cov = take(4 * std::max<size_t>(L, 1));
    uint8_t *work = nullptr, *d_rows = nullptr;
    int *arena = nullptr;
    POOL(POOL_CLIP_WORK, carve, work);
    POOL(POOL_CLIP_ARENA, 4 * (size_t)ent, arena);
    POOL(POOL_LAY_ROWS, std::max<size_t>(1, sizeof(pba_strand_overlap) * n_rows), d_rows);
    unsigned long long *cum = (unsigned long long *)(work + o_cum), *cnt = (unsigned long long *)(work + o_cnt);
    int *niv = (int *)(work + o_niv), *d_cov = (int *)(work + o_cov);
    hipStream_t st = ctx->stream;
    if (n_rows) HIPCHK(hipMemcpyAsync(d_rows, rows, sizeof(pba_strand_overlap) * n_rows, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(cum, h_cum.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(niv, 0, 4 * (size_t)n, st));
    HIPCHK(hipMemsetAsync(cnt, 0, 8 * CC_COUNT, st));
    HIPCHK(memset_big(arena, 0, 4 * (size_t)ent, st));
    if (n_rows) hipLaunchKernelGGL(k_clip_events, dim3(elem_grid(n_rows, 256)), dim3(256), 0, st, (const pba_strand_overlap *)d_rows, n_rows, cum,
                                   read, read + 1, margin, flags, arena, niv, cnt);
    clip_launch_sweep(st, arena, cum, read, read + 1, reads->d_len, niv, margin, 1, 0, flags, nullptr, nullptr, d_cov);
    HIPCHK(hipGetLastError());
    const uint32_t k = std::min(cap, L);
    if (k) HIPCHK(hipMemcpyAsync(cov, d_cov, 4 * (size_t)k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                         // (h_cum must outlive its copy)
    *n_out = L;
    return PBA_OK;
}

int pba_clip_apply(pba_ctx *ctx, const pba_clip *clip, const pba_seqs *reads, pba_seqs **clipped) {
    if (!ctx || !clip || !reads || !clipped) return PBA_E_INVALID;
    *clipped = nullptr;
    if (reads->n != clip->n || !std::equal(clip->h_len.begin(), clip->h_len.end(), reads->h_len.begin()))
        PBA_FAIL(PBA_E_INVALID, "pba_clip_apply: the set differs from the clipped one in count or lengths");
    if (reads->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_clip_apply: the read set holds bytes outside ACGT (code 3 would come back as T)");
    HIPCHK(hipSetDevice(ctx->device));
    StageClock clk;
    if (!clk.init()) PBA_FAIL(PBA_E_HIP, "pba_clip_apply: hipEventCreate");
    const uint32_t n = clip->n;
    const uint64_t total = clip->h_toff[n];
    size_t carve = 0;
    auto take = [&carve](size_t bytes) { const size_t at = carve; carve += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_off = take(8 * ((size_t)n + 1)), o_text = take((size_t)total + kSlack);
    uint8_t *buf = nullptr;
    POOL(POOL_CLIP_TEXT, carve, buf);
    unsigned long long *d_off = (unsigned long long *)(buf + o_off);
    char *text = (char *)(buf + o_text);
    clip->stats.gather_ms = 0.f;
    {
        const auto timed = clk.time(ctx->stream, &clip->stats.gather_ms);
        HIPCHK(hipMemcpyAsync(d_off, clip->h_toff.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
        if (total) {
            hipLaunchKernelGGL(k_clip_gather, dim3(elem_grid((total + 15) / 16, 256)), dim3(256), 0, ctx->stream, reads->dev(),
                               clip->table.as<pba_clip_row>(), d_off, n, (unsigned long long)total, text);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return pba_seqs_from_device_text(ctx, text, d_off, n, total, 0, clipped);
}

int pba_clip_last_stats(const pba_clip *clip, pba_clip_stats *out) {
    if (!clip || !out) return PBA_E_INVALID;
    *out = clip->stats;
    return PBA_OK;
}

void pba_clip_destroy(pba_clip *clip) {
    if (!clip) return;
    (void)hipSetDevice(clip->device);
    delete clip;
}

}  // extern "C"
