// pba_census.hip -- the seed-key census (pba_census_*): how often every masked seed key occurs among the
// positions the seed index visits, the histogram and the cutoff read off it, the probe entries of over-frequent keys masked
// out, a per-sequence repeat profile, and the both-strand overlap call composed on top (pba_overlap_strands_masked).  Host
// side; the kernels are in census.h.  One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here
// fails loudly (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
//
// The census owns its counters (one u32 per value of the mask's care bits, the probe table's direct addressing) and two u64
// totals behind them.  Everything else a call needs -- the tile offsets, keys and counts of a look-up, the histogram, the
// per-sequence profile -- is carved out of the ctx's pooled work buffer (POOL_LAY_WORK, as the layout and the placement carve
// theirs) and written before it is read: a repeated call allocates nothing.
#include "pba_host.h"

#include "census.h"

extern "C" {

struct pba_census {
    int device;
    uint32_t mask;
    int mode;
    uint32_t bits;
    uint32_t mv[5];
    DevBuf counters;                             // 2^bits u32, then tot[2] (u64: counted, zero keys)
    pba_census_stats stats;
    uint64_t buckets() const { return 1ull << bits; }
    CensusDev dev() const {
        CensusDev C;
        C.count = counters.as<uint32_t>(); C.mask = mask;
        memcpy(C.mv, mv, sizeof mv);
        return C;
    }
    unsigned long long *d_tot() const { return (unsigned long long *)(counters.as<uint8_t>() + 4 * buckets()); }
};

// the tile offsets of sequences [lo, hi) of s under `mode` (hi - lo + 1 of them) and the positions they visit; PBA_E_TOOLONG
// if the tiles outgrow a launch
static int census_tiles(pba_ctx *ctx, const char *who, const pba_seqs *s, uint32_t lo, uint32_t hi, int mode, std::vector<uint32_t> &tile_at,
                        uint64_t *visited) {
    tile_at.assign((size_t)(hi - lo) + 1, 0);
    uint64_t tiles = 0, v = 0;
    for (uint32_t r = lo; r < hi; ++r) {
        tile_at[r - lo] = (uint32_t)tiles;
        const VisitRule w = visit_rule(s->h_len[r], mode);                  // the index's own rule, as the kernels read it
        tiles += census_tiles_of(w);
        v += w.visited;
        if (tiles >= (1ull << 31)) return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "2^31 tiles or more in one call");
    }
    tile_at[hi - lo] = (uint32_t)tiles;
    *visited = v;
    return PBA_OK;
}

static bool census_mode_ok(int mode) { return mode == PBA_INDEX_ALL || mode == PBA_INDEX_HEAD_TAIL; }

int pba_census_add(pba_ctx *ctx, pba_census *c, const pba_seqs *s, uint32_t lo, uint32_t hi) {
    if (!ctx || !c || !s || lo > hi || hi > s->n) return PBA_E_INVALID;
    std::vector<uint32_t> tile_at;
    uint64_t visited = 0;
    PBA_TRY(census_tiles(ctx, "pba_census_add", s, lo, hi, c->mode, tile_at, &visited));
    if (c->stats.n_visited + visited >= (1ull << 32)) PBA_FAIL(PBA_E_TOOLONG, "pba_census: 2^32 visited positions or more (a counter is 32 bits)");
    HIPCHK(hipSetDevice(ctx->device));
    StageClock clk;
    if (!clk.init()) PBA_FAIL(PBA_E_HIP, "pba_census_add: hipEventCreate");
    const uint32_t n = hi - lo, tiles = tile_at[n];
    hipStream_t st = ctx->stream;
    unsigned long long h_tot[2] = {0, 0};
    if (tiles) {
        uint32_t *d_tile_at = nullptr;
        POOL(POOL_LAY_WORK, 4 * ((size_t)n + 1), d_tile_at);
        HIPCHK(hipMemcpyAsync(d_tile_at, tile_at.data(), 4 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
        {
            const auto timed = clk.time(st, &c->stats.count_ms);
            if (c->mode == PBA_INDEX_ALL)
                hipLaunchKernelGGL(k_census_count<PBA_INDEX_ALL>, dim3(tiles), dim3(CENSUS_THREADS), 0, st, s->dev(), lo, n, d_tile_at, c->dev(), c->d_tot());
            else
                hipLaunchKernelGGL(k_census_count<PBA_INDEX_HEAD_TAIL>, dim3(tiles), dim3(CENSUS_THREADS), 0, st, s->dev(), lo, n, d_tile_at, c->dev(), c->d_tot());
            HIPCHK(hipGetLastError());
        }
    }
    HIPCHK(hipMemcpyAsync(h_tot, c->d_tot(), sizeof h_tot, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                         // (the tile offsets must outlive their copy)
    c->stats.n_seqs += n;
    c->stats.n_visited += visited;
    c->stats.n_counted = h_tot[0];
    c->stats.n_zero_keys = h_tot[1];
    if (c->stats.n_counted + c->stats.n_zero_keys != c->stats.n_visited)
        PBA_FAIL(PBA_E_HIP, "pba_census_add: the kernel counted other positions than the lengths give (an inconsistency inside the engine)");
    return PBA_OK;
}

int pba_census_create(pba_ctx *ctx, const pba_seqs *s, uint32_t lo, uint32_t hi, uint32_t mask, int mode, pba_census **out) {
    if (!ctx || !s || !out || lo > hi || hi > s->n) return PBA_E_INVALID;
    *out = nullptr;
    if (!mask) PBA_FAIL(PBA_E_INVALID, "pba_census_create: mask 0");
    if (!census_mode_ok(mode)) PBA_FAIL(PBA_E_INVALID, "pba_census_create: mode is neither PBA_INDEX_ALL nor PBA_INDEX_HEAD_TAIL");
    const int care = __builtin_popcount(mask);
    if (care > 26) PBA_FAIL(PBA_E_TOOLONG, "pba_census_create: a mask with more than 26 care bits (the counters are direct-address)");
    HIPCHK(hipSetDevice(ctx->device));
    std::unique_ptr<pba_census, void (*)(pba_census *)> c(new (std::nothrow) pba_census(), pba_census_destroy);
    if (!c) PBA_FAIL(PBA_E_NOMEM, "pba_census");
    c->device = ctx->device; c->mask = mask; c->mode = mode; c->bits = (uint32_t)care;
    compress_masks(mask, c->mv);
    memset(&c->stats, 0, sizeof c->stats);
    c->stats.bits = c->bits;
    const size_t bytes = 4 * (size_t)c->buckets() + 16;
    if (hipMalloc(&c->counters.p, bytes) != hipSuccess) { (void)hipGetLastError(); c->counters.p = nullptr; PBA_FAIL(PBA_E_NOMEM, "pba_census_create: the counters"); }
    HIPCHK(memset_big(c->counters.p, 0, bytes, ctx->stream));
    PBA_TRY(pba_census_add(ctx, c.get(), s, lo, hi));
    *out = c.release();
    return PBA_OK;
}

int pba_census_lookup(pba_ctx *ctx, const pba_census *c, const uint32_t *keys, uint32_t n, uint32_t *counts) {
    if (!ctx || !c || ((!keys || !counts) && n)) return PBA_E_INVALID;
    if (!n) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t at = (4 * (size_t)n + 255) & ~(size_t)255;
    uint8_t *work = nullptr;
    POOL(POOL_LAY_WORK, at + 4 * (size_t)n, work);
    uint32_t *d_keys = (uint32_t *)work, *d_counts = (uint32_t *)(work + at);
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(d_keys, keys, 4 * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_census_lookup, dim3((n + 255) / 256), dim3(256), 0, st, c->dev(), d_keys, n, d_counts);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(counts, d_counts, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return PBA_OK;
}

int pba_census_histogram(pba_ctx *ctx, const pba_census *c, uint64_t *hist, uint32_t cap, uint64_t *n_distinct, uint32_t *max_count) {
    if (!ctx || !c || !hist) return PBA_E_INVALID;
    if (cap < 2) PBA_FAIL(PBA_E_INVALID, "pba_census_histogram: cap below 2");
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long *d = nullptr;                         // res[2], then the slots
    POOL(POOL_LAY_WORK, 8 * ((size_t)cap + 2), d);
    hipStream_t st = ctx->stream;
    HIPCHK(memset_big(d, 0, 8 * ((size_t)cap + 2), st));
    const uint64_t B = c->buckets();
    const uint32_t grid = (uint32_t)std::min<uint64_t>((B + 255) / 256, 8ull * (uint32_t)ctx->prop.multiProcessorCount);
    hipLaunchKernelGGL(k_census_hist, dim3(grid), dim3(256), 0, st, (const uint32_t *)c->counters.as<uint32_t>(), B, cap, d + 2, d);
    HIPCHK(hipGetLastError());
    unsigned long long res[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(res, d, sizeof res, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hist, d + 2, 8 * (size_t)cap, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    hist[0] = B - res[0];
    if (n_distinct) *n_distinct = res[0];
    if (max_count) *max_count = (uint32_t)res[1];
    return PBA_OK;
}

int pba_census_cutoff(const uint64_t *hist, uint32_t cap, double fraction, uint32_t floor, uint32_t *max_occ) {
    if (!hist || !max_occ || cap < 2 || !(fraction >= 0.0) || !(fraction <= 1.0)) return PBA_E_INVALID;
    uint64_t n_distinct = 0;
    for (uint32_t v = 1; v < cap; ++v) n_distinct += hist[v];
    const uint64_t budget = (uint64_t)(fraction * n_distinct);
    uint64_t above = n_distinct;                             // distinct keys with count > c, c = 0
    for (uint32_t c = 1; c + 2 <= cap; ++c) {                // c in [1, cap - 2]
        above -= hist[c];
        if (c >= floor && above <= budget) { *max_occ = c; return PBA_OK; }
    }
    return PBA_E_TOOLONG;
}

int pba_census_read_repeats(pba_ctx *ctx, const pba_census *c, const pba_seqs *s, uint32_t max_occ, uint32_t *n_over,
                            uint32_t *n_visited, uint32_t cap) {
    if (!ctx || !c || !s || ((!n_over || !n_visited) && s->n)) return PBA_E_INVALID;
    if (cap < s->n) PBA_FAIL(PBA_E_INVALID, "pba_census_read_repeats: cap below the number of sequences");
    const uint32_t n = s->n;
    if (!n) return PBA_OK;
    std::vector<uint32_t> tile_at;
    uint64_t visited = 0;
    PBA_TRY(census_tiles(ctx, "pba_census_read_repeats", s, 0, n, c->mode, tile_at, &visited));
    HIPCHK(hipSetDevice(ctx->device));
    const size_t at = (4 * ((size_t)n + 1) + 255) & ~(size_t)255;
    uint8_t *work = nullptr;
    POOL(POOL_LAY_WORK, at + 8 * (size_t)n, work);
    uint32_t *d_tile_at = (uint32_t *)work;
    unsigned long long *d_out = (unsigned long long *)(work + at);
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemcpyAsync(d_tile_at, tile_at.data(), 4 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    HIPCHK(memset_big(d_out, 0, 8 * (size_t)n, st));
    const uint32_t tiles = tile_at[n];
    if (tiles) {
        if (c->mode == PBA_INDEX_ALL)
            hipLaunchKernelGGL(k_census_repeats<PBA_INDEX_ALL>, dim3(tiles), dim3(CENSUS_THREADS), 0, st, s->dev(), n, d_tile_at, c->dev(), max_occ, d_out);
        else
            hipLaunchKernelGGL(k_census_repeats<PBA_INDEX_HEAD_TAIL>, dim3(tiles), dim3(CENSUS_THREADS), 0, st, s->dev(), n, d_tile_at, c->dev(), max_occ, d_out);
        HIPCHK(hipGetLastError());
    }
    std::vector<unsigned long long> h_out(n);
    HIPCHK(hipMemcpyAsync(h_out.data(), d_out, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t r = 0; r < n; ++r) { n_over[r] = (uint32_t)h_out[r]; n_visited[r] = (uint32_t)(h_out[r] >> 32); }
    return PBA_OK;
}

int pba_census_mask_probes(pba_ctx *ctx, const pba_census *c, void *d_entries, uint64_t n_slots, uint32_t mask, uint32_t max_occ,
                           uint64_t *n_masked) {
    if (!ctx || !c || !n_masked || (!d_entries && n_slots)) return PBA_E_INVALID;
    *n_masked = 0;
    if (mask != c->mask) PBA_FAIL(PBA_E_INVALID, "pba_census_mask_probes: the census was counted under another mask");
    if (!n_slots) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    unsigned long long *d_n = nullptr;
    POOL(POOL_LAY_WORK, 8, d_n);
    hipStream_t st = ctx->stream;
    HIPCHK(hipMemsetAsync(d_n, 0, 8, st));
    hipLaunchKernelGGL(k_census_mask, dim3(elem_grid(n_slots, 256)), dim3(256), 0, st, c->dev(), (uint64_t *)d_entries, n_slots, max_occ, d_n);
    HIPCHK(hipGetLastError());
    unsigned long long h_n = 0;
    HIPCHK(hipMemcpyAsync(&h_n, d_n, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *n_masked = h_n;
    return PBA_OK;
}

int pba_overlap_strands_masked(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi, uint32_t mask,
                               double R, int max_trial, int overlap_min, int kernel, int strands, const pba_census *c, uint32_t max_occ,
                               pba_strand_overlap *out, uint64_t cap, uint64_t *n_out, pba_overlap_stats stats[2], uint64_t n_masked[2]) {
    if (!ctx || !reads || !c || !n_out || (!out && cap)) return PBA_E_INVALID;
    if (strands < 1 || strands > 3) PBA_FAIL(PBA_E_INVALID, "pba_overlap_strands_masked: strands must be 1 (+1), 2 (-1) or 3 (both)");
    if (c->mode != PBA_INDEX_HEAD_TAIL) PBA_FAIL(PBA_E_INVALID, "pba_overlap_strands_masked: the census must be a PBA_INDEX_HEAD_TAIL one (what a target's index visits)");
    if (c->mask != mask) PBA_FAIL(PBA_E_INVALID, "pba_overlap_strands_masked: the census was counted under another mask");
    if (max_trial < 1 || max_trial > 63) PBA_FAIL(PBA_E_INVALID, "max_trial must be in [1, 63]");
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        PBA_FAIL(PBA_E_INVALID, "pba_overlap_strands_masked: reads_rc differs from reads in count or lengths");
    if (reads->non_acgt || (reads_rc && reads_rc->non_acgt)) PBA_FAIL(PBA_E_ALPHABET, "pba_overlap_strands_masked: the read set holds bytes outside ACGT");
    HIPCHK(hipSetDevice(ctx->device));
    *n_out = 0;
    if (n_masked) n_masked[0] = n_masked[1] = 0;
    struct Own {
        pba_seqs *rc = nullptr;
        pba_probe_table *tab[2] = {nullptr, nullptr};
        ~Own() { pba_probe_table_destroy(tab[0]); pba_probe_table_destroy(tab[1]); if (rc) pba_seqs_destroy(rc); }
    } own;
    if ((strands & 2) && !reads_rc) {
        PBA_TRY(pba_seqs_revcomp(ctx, reads, nullptr, &own.rc));
        reads_rc = own.rc;
    }
    const pba_seqs *sets[2] = {reads, reads_rc};
    const uint64_t pcap = (uint64_t)reads->n * 2u * (uint32_t)max_trial;
    DevBuf d_pent;                                           // the entries of one strand at a time: a table keeps none of them
    for (int k = 0; k < 2; ++k) {
        if (!(strands & (1 << k))) continue;
        if (!d_pent.p) HIPCHK(hipMalloc(&d_pent.p, sizeof(uint64_t) * (pcap + 1)));
        uint64_t n_pent = 0, masked = 0;
        PBA_TRY(pba_overlap_probes(ctx, sets[k], 0, reads->n, mask, max_trial, d_pent.p, pcap, &n_pent));
        PBA_TRY(pba_census_mask_probes(ctx, c, d_pent.p, n_pent, mask, max_occ, &masked));
        if (n_masked) n_masked[k] = masked;
        PBA_TRY(pba_probe_table_create(ctx, d_pent.p, n_pent, mask, max_trial, &own.tab[k]));
    }
    return pba_overlap_strands_table(ctx, reads, (strands & 2) ? reads_rc : nullptr, t_lo, t_hi, own.tab[0], own.tab[1], R, overlap_min,
                                     kernel, out, cap, n_out, stats);
}

int pba_census_last_stats(const pba_census *c, pba_census_stats *out) {
    if (!c || !out) return PBA_E_INVALID;
    *out = c->stats;
    return PBA_OK;
}

void pba_census_destroy(pba_census *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

}  // extern "C"
