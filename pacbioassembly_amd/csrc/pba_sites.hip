// pba_sites.hip -- variant sites from pile-ups and every row's allele at each site (include/pba.h): the scan of a
// live pile-up's arena under the rule of sites.h (flag pass, rank, compaction), the object the sites live in, its maker from
// a caller's list, and the host side of the alleles outlet of the traced bit-vector pass (align_alleles.h: AlleleJob, run by
// k_allele_pairs in pba_align.hip; TraceInto::alleles through trace_batch) with its row-level entry points.  The slot runner,
// the chunk loop and the row layout are shared with pba_cigar.hip and pba_windows.hip (pba_rows.h, aln_rows.h).
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything that needs the device fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind those entry points.
//
// The arena is flat, so the scan knows no targets: one lane per box, one bitmap word per wavefront.  The arena offset of a
// target is no multiple of 64, so words straddle targets; a record's target comes from box_off by binary search in the
// compaction pass, which only the flagged lanes run.  Records come out sorted by (target, pos, kind) by construction: their
// rank is the scanned per-word count plus the popcount of the word's lower bits.
#include "pba_rows.h"
#include "sites.h"

// (struct pba_sites, sites_same_set and pair_alleles_bound: pba_rows.h, shared with pba_phase.hip)

// ---- the scan ------------------------------------------------------------------------------------------------------------
// Flag pass: one lane per box (8 + 8 + 4 bytes, coalesced), one wavefront per bitmap word; lane 0 stores the two words and
// their counts with plain vector stores.
static __global__ void __launch_bounds__(256)
k_sites_flag(ConsDev C, unsigned long long n_boxes, unsigned long long words, SiteRule rule, unsigned long long *bm_sel,
             unsigned long long *bm_sup, uint32_t *cnt_sel, uint32_t *cnt_all) {
    const int lane = threadIdx.x & (PBA_WAVE - 1);
    const unsigned long long stride = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long w = (unsigned long long)blockIdx.x * 4ull + threadIdx.x / PBA_WAVE; w < words; w += stride) {
        const unsigned long long box = w * 64ull + (unsigned long long)lane;
        uint32_t kinds = 0u;
        if (box < n_boxes) kinds = site_rule(C.sel[box], C.sup[box], C.tot[box], rule).kinds;
        const uint64_t s = __builtin_amdgcn_ballot_w64((kinds & (uint32_t)PBA_SITE_SEL) != 0u);
        const uint64_t u = __builtin_amdgcn_ballot_w64((kinds & (uint32_t)PBA_SITE_SUP) != 0u);
        if (lane == 0) {
            bm_sel[w] = s; bm_sup[w] = u;
            cnt_sel[w] = (uint32_t)__builtin_popcountll(s);
            cnt_all[w] = (uint32_t)(__builtin_popcountll(s) + __builtin_popcountll(u));
        }
    }
}

// Compaction pass: the flagged lanes of every word with a site write their records, and the packed word of a SEL site, at
// their ranks.  rank_*: the inclusive scans of the flag pass's counts.
static __global__ void __launch_bounds__(256)
k_sites_write(ConsDev C, unsigned long long words, SiteRule rule, const unsigned long long *bm_sel, const unsigned long long *bm_sup,
              const uint32_t *rank_sel, const uint32_t *rank_all, const unsigned long long *box_off, uint32_t nt, uint32_t t_lo,
              SeqSetDev S, pba_site *recs, uint2 *sel) {
    const int lane = threadIdx.x & (PBA_WAVE - 1);
    const unsigned long long stride = (unsigned long long)gridDim.x * 4ull;
    for (unsigned long long w = (unsigned long long)blockIdx.x * 4ull + threadIdx.x / PBA_WAVE; w < words; w += stride) {
        const unsigned long long s = bm_sel[w], u = bm_sup[w];
        if (!(((s | u) >> lane) & 1ull)) continue;
        const unsigned long long box = w * 64ull + (unsigned long long)lane, below = (1ull << lane) - 1ull;
        uint32_t lo = 0, hi = nt;                              // the last k with box_off[k] <= box: an empty target owns no box
        while (hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if (box_off[mid] <= box) lo = mid; else hi = mid; }
        const uint32_t t = t_lo + lo, pos = (uint32_t)(box - box_off[lo]);
        const int own = (S.packed[S.off[t] + (pos >> 2)] >> (6 - 2 * (pos & 3u))) & 3;         // 2-bit code == C2I of the base
        const SiteCall c = site_rule(C.sel[box], C.sup[box], C.tot[box], rule);
        uint32_t at = (w ? rank_all[w - 1] : 0u) + (uint32_t)__builtin_popcountll(s & below) + (uint32_t)__builtin_popcountll(u & below);
        if ((s >> lane) & 1ull) {
            const pba_site r = site_record(c, PBA_SITE_SEL, (int32_t)t, (int32_t)pos, own);
            recs[at] = r;
            sel[(w ? rank_sel[w - 1] : 0u) + (uint32_t)__builtin_popcountll(s & below)] = make_uint2(at, site_pack(r));
            ++at;
        }
        if ((u >> lane) & 1ull) recs[at] = site_record(c, PBA_SITE_SUP, (int32_t)t, (int32_t)pos, own);
    }
}

// ---- the object ------------------------------------------------------------------------------------------------------------
static void sites_free(pba_sites *s) {
    for (void *q : {(void *)s->d_recs, (void *)s->d_bm, (void *)s->d_rank, (void *)s->d_sel, (void *)s->d_box_off})
        if (q) (void)hipFree(q);
    delete s;
}
struct SitesGuard { pba_sites *s; ~SitesGuard() { if (s) sites_free(s); } pba_sites *release() { pba_sites *r = s; s = nullptr; return r; } };

// an empty object over the sequences [t_lo, t_hi) of `seqs` with the arrays that depend on the arena alone
static int sites_new(pba_ctx *ctx, const pba_seqs *seqs, uint32_t t_lo, uint32_t t_hi, SitesGuard &g) {
    pba_sites *s = new (std::nothrow) pba_sites();
    if (!s) PBA_FAIL(PBA_E_NOMEM, "pba_sites");
    g.s = s;
    const uint32_t nt = t_hi - t_lo;
    s->device = ctx->device; s->t_lo = t_lo; s->t_hi = t_hi; s->n_seqs = seqs->n;
    s->box_off.assign((size_t)nt + 1, 0);
    for (uint32_t k = 0; k < nt; ++k) s->box_off[k + 1] = s->box_off[k] + seqs->h_len[t_lo + k];
    s->n_boxes = s->box_off[nt];
    if (s->n_boxes >= (1ull << 31)) PBA_FAIL(PBA_E_TOOLONG, "pba_sites: 2^31 boxes or more in one range");
    s->words = (s->n_boxes + 63) / 64;
    HIPCHK(hipMalloc((void **)&s->d_bm, sizeof(uint64_t) * (s->words + 1)));
    HIPCHK(hipMalloc((void **)&s->d_rank, sizeof(uint32_t) * (s->words + 1)));
    HIPCHK(hipMalloc((void **)&s->d_box_off, sizeof(uint64_t) * ((size_t)nt + 1)));
    HIPCHK(hipMemcpyAsync(s->d_box_off, s->box_off.data(), sizeof(uint64_t) * ((size_t)nt + 1), hipMemcpyHostToDevice, ctx->stream));
    return PBA_OK;
}

// what the host keeps of the records: every target's record range, its SEL positions
static void sites_index(pba_sites *s, const pba_site *recs) {
    const uint32_t nt = s->t_hi - s->t_lo;
    s->rec_off.assign((size_t)nt + 1, 0); s->sel_off.assign((size_t)nt + 1, 0);
    s->sel_pos.clear(); s->sel_rec.clear();
    for (uint64_t x = 0; x < s->n; ++x) {
        const size_t k = (size_t)((uint32_t)recs[x].target - s->t_lo);
        ++s->rec_off[k + 1];
        if (recs[x].kind == PBA_SITE_SEL) { ++s->sel_off[k + 1]; s->sel_pos.push_back(recs[x].pos); s->sel_rec.push_back((uint32_t)x); }
    }
    for (uint32_t k = 0; k < nt; ++k) { s->rec_off[k + 1] += s->rec_off[k]; s->sel_off[k + 1] += s->sel_off[k]; }
}

int pba_pileup_sites(pba_ctx *ctx, const pba_pileup *p, const pba_seqs *target, int min_depth, int min_alt, int min_permille,
                     pba_sites **out) {
    static const char who[] = "pba_pileup_sites";
    if (!ctx || !p || !target || !out) return PBA_E_INVALID;
    *out = nullptr;
    PileView v;
    PBA_TRY(pile_view(ctx, who, p, &v));
    if (min_depth < 1 || min_alt < 1 || min_permille < 0 || min_permille > 1000)
        return ctx_fail_as(ctx, PBA_E_INVALID, who, "min_depth and min_alt must be at least 1, min_permille in [0, 1000]");
    bool same = target->n == v.n_reads;
    for (uint32_t k = 0; same && k < v.t_hi - v.t_lo; ++k) same = v.box_off[k + 1] - v.box_off[k] == target->h_len[v.t_lo + k];
    if (!same) return ctx_fail_as(ctx, PBA_E_INVALID, who, "the target set is not the set of this pile-up");
    HIPCHK(hipSetDevice(ctx->device));
    SitesGuard g{nullptr};
    PBA_TRY(sites_new(ctx, target, v.t_lo, v.t_hi, g));
    pba_sites *s = g.s;
    const uint32_t nt = v.t_hi - v.t_lo;
    const SiteRule rule{min_depth, min_alt, min_permille, v.weight};
    DevBuf bm_sup, rank_all, scratch;
    HIPCHK(hipMalloc(&bm_sup.p, sizeof(uint64_t) * (s->words + 1)));
    HIPCHK(hipMalloc(&rank_all.p, sizeof(uint32_t) * (s->words + 1)));
    HIPCHK(hipMalloc(&scratch.p, sizeof(uint32_t) * scan_scratch_words(s->words)));
    HIPCHK(hipMemsetAsync(s->d_bm + s->words, 0, sizeof(uint64_t), ctx->stream));
    uint32_t totals[2] = {0u, 0u};
    const uint32_t grid = elem_grid(s->words * 64, 256);
    if (s->words) {
        hipLaunchKernelGGL(k_sites_flag, dim3(grid), dim3(256), 0, ctx->stream, v.C, (unsigned long long)s->n_boxes, (unsigned long long)s->words,
                           rule, s->d_bm, bm_sup.as<unsigned long long>(), s->d_rank, rank_all.as<uint32_t>());
        HIPCHK(hipGetLastError());
        (void)scan_inclusive(ctx, s->d_rank, s->words, scratch.as<uint32_t>());
        (void)scan_inclusive(ctx, rank_all.as<uint32_t>(), s->words, scratch.as<uint32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&totals[0], s->d_rank + (s->words - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(&totals[1], rank_all.as<uint32_t>() + (s->words - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    s->n_sel = totals[0]; s->n = totals[1];           // (fewer than 2^31 boxes, two records each at most: below 2^32)
    HIPCHK(hipMalloc((void **)&s->d_recs, sizeof(pba_site) * (s->n + 1)));
    HIPCHK(hipMalloc((void **)&s->d_sel, sizeof(uint2) * (s->n_sel + 1)));
    std::vector<pba_site> recs(s->n);
    if (s->n) {
        hipLaunchKernelGGL(k_sites_write, dim3(grid), dim3(256), 0, ctx->stream, v.C, (unsigned long long)s->words, rule, s->d_bm,
                           bm_sup.as<unsigned long long>(), s->d_rank, rank_all.as<uint32_t>(), s->d_box_off, nt, v.t_lo, target->dev(),
                           s->d_recs, s->d_sel);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(recs.data(), s->d_recs, sizeof(pba_site) * s->n, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (uint64_t x = 0; x < s->n; ++x)
        if (recs[x].target < (int32_t)v.t_lo || (uint32_t)recs[x].target >= v.t_hi) PBA_FAIL(PBA_E_HIP, "pba_pileup_sites: a record names a target outside the range");
    sites_index(s, recs.data());
    *out = g.release();
    return PBA_OK;
}

int pba_sites_create(pba_ctx *ctx, const pba_seqs *seqs, uint32_t t_lo, uint32_t t_hi, const pba_site *recs, uint64_t n, pba_sites **out) {
    static const char who[] = "pba_sites_create";
    if (!ctx || !seqs || !out || (n && !recs) || t_lo > t_hi || t_hi > seqs->n) return PBA_E_INVALID;
    *out = nullptr;
    if (n >= (1ull << 32)) return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "2^32 sites or more");
    for (uint64_t x = 0; x < n; ++x) {
        const pba_site &r = recs[x];
        if (r.target < 0 || (uint32_t)r.target < t_lo || (uint32_t)r.target >= t_hi) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a site's target is outside the range");
        if (r.pos < 0 || (uint32_t)r.pos >= seqs->h_len[r.target]) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a site's position is outside its sequence");
        if (r.kind != PBA_SITE_SEL && r.kind != PBA_SITE_SUP) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a site's kind is neither SEL nor SUP");
        if (r.own > 3 || r.major > 4 || r.minor > (r.kind == PBA_SITE_SEL ? 4 : 3)) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a site's allele code is out of range");
        if (x) {
            const pba_site &b = recs[x - 1];
            const bool after = r.target != b.target ? r.target > b.target : (r.pos != b.pos ? r.pos > b.pos : r.kind > b.kind);
            if (!after) return ctx_fail_as(ctx, PBA_E_INVALID, who, "the sites are not sorted strictly by (target, pos, kind)");
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    SitesGuard g{nullptr};
    PBA_TRY(sites_new(ctx, seqs, t_lo, t_hi, g));
    pba_sites *s = g.s;
    s->n = n;
    std::vector<uint64_t> bm(s->words + 1, 0);
    std::vector<uint32_t> rank(s->words + 1, 0);
    std::vector<uint2> sel;
    for (uint64_t x = 0; x < n; ++x) {
        if (recs[x].kind != PBA_SITE_SEL) continue;
        const uint64_t box = s->box_off[(uint32_t)recs[x].target - t_lo] + (uint64_t)recs[x].pos;
        bm[box >> 6] |= 1ull << (box & 63);
        ++rank[box >> 6];
        sel.push_back(make_uint2((uint32_t)x, site_pack(recs[x])));
    }
    for (uint64_t w = 1; w < s->words; ++w) rank[w] += rank[w - 1];
    s->n_sel = sel.size();
    sel.push_back(make_uint2(0u, 0u));
    HIPCHK(hipMalloc((void **)&s->d_recs, sizeof(pba_site) * (n + 1)));
    HIPCHK(hipMalloc((void **)&s->d_sel, sizeof(uint2) * sel.size()));
    if (n) HIPCHK(hipMemcpyAsync(s->d_recs, recs, sizeof(pba_site) * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(s->d_sel, sel.data(), sizeof(uint2) * sel.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(s->d_bm, bm.data(), sizeof(uint64_t) * bm.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(s->d_rank, rank.data(), sizeof(uint32_t) * rank.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));            // (the sources are locals)
    sites_index(s, recs);
    *out = g.release();
    return PBA_OK;
}

uint64_t pba_sites_count(const pba_sites *s) { return s ? s->n : 0; }
uint64_t pba_sites_count_sel(const pba_sites *s) { return s ? s->n_sel : 0; }

int pba_sites_target_range(const pba_sites *s, uint32_t target, uint64_t *lo, uint64_t *hi) {
    if (!s || !lo || !hi || target < s->t_lo || target >= s->t_hi) return PBA_E_INVALID;
    *lo = s->rec_off[target - s->t_lo]; *hi = s->rec_off[target - s->t_lo + 1];
    return PBA_OK;
}

int pba_sites_get(pba_ctx *ctx, const pba_sites *s, uint64_t lo, uint64_t hi, pba_site *out) {
    if (!ctx || !s || lo > hi || hi > s->n || (hi > lo && !out)) return PBA_E_INVALID;
    if (hi == lo) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out, s->d_recs + lo, sizeof(pba_site) * (hi - lo), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

void pba_sites_destroy(pba_sites *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    sites_free(s);                        // hipFree waits for the work that uses the buffers
}

// ---- alleles of rows ---------------------------------------------------------------------------------------------------------
// the alleles of the jobs dense and in row order on the host, the totals row by row
static int rows_alleles_out(pba_ctx *ctx, const char *who, const pba_seqs *const A[2], const pba_seqs *const B[2], const std::vector<RowJob> &jobs,
                            uint64_t n_rows, double R, int gate, const pba_sites *sites, pba_allele *out, uint64_t cap, uint64_t *off,
                            uint64_t *n_total, pba_allele_counts *sum, pba_result *res, uint64_t max_slots) {
    if (!sites_same_set(sites, A[0])) return ctx_fail_as(ctx, PBA_E_INVALID, who, "the sites were not made from this target set");
    for (const RowJob &jb : jobs)
        if (jb.pr.a_seq < sites->t_lo || jb.pr.a_seq >= sites->t_hi) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's target is outside the range of the sites");
    std::vector<std::vector<pba_allele>> of(jobs.size());
    std::vector<pba_allele> h;
    std::vector<pba_aln_counts> cnt(n_rows, pba_aln_counts{0, 0, 0, 0});
    const auto sink = [&](const SlotBatch &b) -> int {
        h.resize(b.rel[b.nb] + 1);
        HIPCHK(hipMemcpyAsync(h.data(), b.d->slot.p, sizeof(pba_allele) * b.rel[b.nb], hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (size_t q = 0; q < b.nb; ++q) of[b.at[q]].assign(h.begin() + (ptrdiff_t)b.rel[q], h.begin() + (ptrdiff_t)(b.rel[q] + (uint64_t)b.have[q]));
        return PBA_OK;
    };
    const auto bound = [sites, R](const pba_pair &p) -> uint64_t { return pair_alleles_bound(sites, p, R); };
    const AllelesInto view = sites->view();
    PBA_TRY(rows_chunks<pba_allele>(ctx, who, A, B, jobs, R, bound, SlotsInto{}, ~0u, cnt.data(), res, max_slots ? max_slots : kAlleleChunkSlots,
                                    nullptr, sink, &view, gate));
    rows_layout(of, job_rows(jobs), n_rows, out, cap, off, n_total);
    for (uint64_t k = 0; sum && k < n_rows; ++k)
        sum[k] = pba_allele_counts{(int32_t)(off[k + 1] - off[k]), cnt[k].n_eq, cnt[k].n_x, cnt[k].n_ins, cnt[k].n_del};
    return PBA_OK;
}

int pba_overlap_rows_alleles_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                    uint64_t n, double R, const pba_sites *sites, pba_allele *out, uint64_t cap, uint64_t *off,
                                    uint64_t *n_total, pba_allele_counts *sum, pba_result *res, uint64_t max_slots) {
    static const char who[] = "pba_overlap_rows_alleles";
    if (!ctx || !reads || !sites || (!rows && n) || !off || !n_total || (cap && !out)) return PBA_E_INVALID;
    std::vector<RowJob> jobs;
    PBA_TRY(overlap_rows_jobs(ctx, who, reads, reads_rc, rows, n, R, nullptr, res, &jobs));
    const pba_seqs *const A[2] = {reads, reads}, *const B[2] = {reads, reads_rc};
    return rows_alleles_out(ctx, who, A, B, jobs, n, R, 0, sites, out, cap, off, n_total, sum, res, max_slots);
}

int pba_overlap_rows_alleles(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                             double R, const pba_sites *sites, pba_allele *out, uint64_t cap, uint64_t *off, uint64_t *n_total,
                             pba_allele_counts *sum, pba_result *res) {
    return pba_overlap_rows_alleles_budget(ctx, reads, reads_rc, rows, n, R, sites, out, cap, off, n_total, sum, res, 0);
}

int pba_map_rows_alleles_budget(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                                const pba_map_row *rows, uint64_t n, double R, int overlap_min, const pba_sites *sites, pba_allele *out,
                                uint64_t cap, uint64_t *off, uint64_t *n_total, pba_allele_counts *sum, pba_result *res,
                                uint64_t max_slots) {
    static const char who[] = "pba_map_rows_alleles";
    if (!ctx || !target || !reads || !sites || (!rows && n) || !off || !n_total || (cap && !out)) return PBA_E_INVALID;
    std::vector<RowJob> jobs;
    PBA_TRY(map_rows_vote_jobs(ctx, who, target, reads, reads_rc, rows, n, R, nullptr, res, &jobs));
    const pba_seqs *const A[2] = {target, target}, *const B[2] = {reads, reads_rc};
    return rows_alleles_out(ctx, who, A, B, jobs, n, R, overlap_min, sites, out, cap, off, n_total, sum, res, max_slots);
}

int pba_map_rows_alleles(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_map_row *rows,
                         uint64_t n, double R, int overlap_min, const pba_sites *sites, pba_allele *out, uint64_t cap, uint64_t *off,
                         uint64_t *n_total, pba_allele_counts *sum, pba_result *res) {
    return pba_map_rows_alleles_budget(ctx, target, reads, reads_rc, rows, n, R, overlap_min, sites, out, cap, off, n_total, sum, res, 0);
}
