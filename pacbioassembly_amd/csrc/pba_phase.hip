// pba_phase.hip -- overlap rows phased by their alleles (include/pba.h: pba_phase_*, pba_alleles_phase, pba_overlap_rows_phase;
// DESIGN 5.14): the kernels of the phase rule (phase.h) over classified allele records, the driver both entry points share,
// the gather that puts a chunk's allele slots (pba_rows.h, the alleles outlet of the traced pass) side by side in one device
// buffer, and the host-only pba_phase_rows_apply.  One process per GPU, one pba_ctx per process, one HIP stream per ctx.
// Everything that needs the device fails loudly (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind those entry points.
//
// Every term of the rule is in {-1, 0, +1}: a row's sum over 64 records is popcount(ballot(term > 0)) - popcount(ballot(term <
// 0)), one wavefront per row, no shuffle, no LDS.  What a row adds to its sites goes out as 32-bit vector atomics in global
// memory.  All targets go in one launch: a row's records are of one target, a site is of one target, and nothing else ties
// rows together.
#include "pba_rows.h"
#include "phase.h"

// ---- classify --------------------------------------------------------------------------------------------------------------
// inv[record index] = SEL rank, for the SEL records (the others keep the 0xFFFFFFFF the host put there)
static __global__ void __launch_bounds__(256)
k_phase_inverse(const uint2 *sel, uint32_t n_sel, uint32_t *inv) {
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n_sel; s += gridDim.x * 256u) inv[sel[s].x] = s;
}

// One lane per SEL site: the seed orientation, and everything the later passes add to or read, written here.
static __global__ void __launch_bounds__(256)
k_phase_seed(const uint2 *sel, uint32_t n_sel, int self_weight, int32_t *o0, int32_t *o, int32_t *f, int32_t *score, int32_t *agree,
             int32_t *dis) {
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n_sel; s += gridDim.x * 256u) {
        const int v = phase_seed(sel[s].y);
        o0[s] = v; o[s] = v; f[s] = 0; score[s] = self_weight * v; agree[s] = 0; dis[s] = 0;
    }
}

// One lane per record: { SEL rank, v } in one word.  A record whose site is no SEL record of the object cannot come from the
// host checks or from the sink; it is counted in *bad and classified as nothing.
static __global__ void __launch_bounds__(256)
k_phase_classify(const pba_allele *rec, unsigned long long n_rec, const uint32_t *inv, unsigned long long n_sites, const uint2 *sel,
                 uint32_t *pk, uint32_t *bad) {
    const unsigned long long stride = (unsigned long long)gridDim.x * 256ull;
    for (unsigned long long x = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; x < n_rec; x += stride) {
        const pba_allele r = rec[x];
        const uint32_t s = r.site < n_sites ? inv[r.site] : 0xFFFFFFFFu;
        if (s == 0xFFFFFFFFu) { pk[x] = 0u; atomicAdd(bad, 1u); continue; }
        pk[x] = phase_rec(s, phase_value(sel[s].y, r.allele));
    }
}

// ---- the half-iteration over rows ---------------------------------------------------------------------------------------------
// One wavefront per row: g = sum of o[site] * v over its records, h = lab(g).  !FINAL: h * v is added to f[site].  FINAL: the
// row's pba_phase_row, and its records counted at their sites as agreeing or disagreeing with the label.
template <bool FINAL>
static __global__ void __launch_bounds__(256)
k_phase_rows(const uint32_t *pk, const unsigned long long *beg, const uint32_t *len, uint32_t n, const int32_t *o, int32_t *f,
             int min_margin, pba_phase_row *rows, int32_t *agree, int32_t *dis) {
    const int lane = threadIdx.x & (PBA_WAVE - 1);
    const uint32_t stride = gridDim.x * 4u;
    for (uint32_t r = blockIdx.x * 4u + threadIdx.x / PBA_WAVE; r < n; r += stride) {
        const unsigned long long b = beg[r];
        const uint32_t m = __builtin_amdgcn_readfirstlane(len[r]);
        int pos = 0, neg = 0;
        for (uint32_t base = 0; base < m; base += PBA_WAVE) {
            int t = 0;
            if (base + lane < m) {
                const uint32_t w = pk[b + base + lane];
                t = o[phase_rec_rank(w)] * phase_rec_value(w);
            }
            pos += __builtin_popcountll(__builtin_amdgcn_ballot_w64(t > 0));
            neg += __builtin_popcountll(__builtin_amdgcn_ballot_w64(t < 0));
        }
        const int g = pos - neg, h = phase_lab(g, min_margin);
        if (FINAL && lane == 0) rows[r] = pba_phase_row{h, g, pos + neg, (int32_t)m};
        if (h == 0) continue;
        for (uint32_t base = 0; base < m; base += PBA_WAVE) {
            if (base + lane >= m) continue;
            const uint32_t w = pk[b + base + lane], s = phase_rec_rank(w);
            const int v = phase_rec_value(w);
            if (!FINAL) {
                if (v != 0) atomicAdd(&f[s], h * v);
            } else {
                const int t = h * v * o[s];
                if (t != 0) atomicAdd(t > 0 ? &agree[s] : &dis[s], 1);
            }
        }
    }
}

// ---- orient ----------------------------------------------------------------------------------------------------------------
// One lane per SEL site: o = sign(self_weight * o0 + f), the f kept as the site's score, f zeroed for the next half-iteration;
// the wavefront's flips counted by ballot, one atomic a wavefront.
static __global__ void __launch_bounds__(256)
k_phase_orient(uint32_t n_sel, int self_weight, const int32_t *o0, int32_t *f, int32_t *o, int32_t *score, uint32_t *flips) {
    const uint32_t words = (n_sel + PBA_WAVE - 1) / PBA_WAVE, stride = gridDim.x * 4u;
    const int lane = threadIdx.x & (PBA_WAVE - 1);
    for (uint32_t w = blockIdx.x * 4u + threadIdx.x / PBA_WAVE; w < words; w += stride) {
        const uint32_t s = w * PBA_WAVE + (uint32_t)lane;
        bool flipped = false;
        if (s < n_sel) {
            const int fv = self_weight * o0[s] + f[s], now = phase_sign(fv);
            flipped = now != o[s];
            o[s] = now; score[s] = fv; f[s] = 0;
        }
        const int nf = __builtin_popcountll(__builtin_amdgcn_ballot_w64(flipped));
        if (lane == 0 && nf) atomicAdd(flips, (uint32_t)nf);
    }
}

static __global__ void __launch_bounds__(256)
k_phase_sites_out(const uint2 *sel, uint32_t n_sel, const int32_t *o, const int32_t *score, const int32_t *agree, const int32_t *dis,
                  pba_phase_site *out) {
    for (uint32_t s = blockIdx.x * 256u + threadIdx.x; s < n_sel; s += gridDim.x * 256u)
        out[s] = pba_phase_site{sel[s].x, o[s], score[s], agree[s], dis[s]};
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
// One wavefront per slot of a finished batch: its n[q] records from slot[off[q] ..) to dst[dst_beg[q] ..).
static __global__ void __launch_bounds__(256)
k_phase_gather(const pba_allele *slot, const uint64_t *off, const int32_t *n, const unsigned long long *dst_beg, uint32_t nb, pba_allele *dst) {
    const int lane = threadIdx.x & (PBA_WAVE - 1);
    const uint32_t stride = gridDim.x * 4u;
    for (uint32_t q = blockIdx.x * 4u + threadIdx.x / PBA_WAVE; q < nb; q += stride) {
        const uint64_t room = off[q + 1] - off[q];
        int32_t m = n[q];
        if (m < 0) m = 0;
        if ((uint64_t)m > room) m = (int32_t)room;                         // never beyond the slot
        for (int32_t x = lane; x < m; x += PBA_WAVE) dst[dst_beg[q] + (unsigned long long)x] = slot[off[q] + (uint64_t)x];
    }
}

// ---- the driver ----------------------------------------------------------------------------------------------------------------
struct EventPair {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~EventPair() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

// The rule over n rows whose records lie on the device: row r owns rec[beg[r] .. beg[r] + len[r]) (beg, len on the host), n_rec
// records in all.  rows_out: n; sites_out (nullable): n_sel; st: counts and phase_ms filled in.
static int phase_run(pba_ctx *ctx, const char *who, const pba_sites *sites, const pba_allele *d_rec, uint64_t n_rec,
                     const std::vector<unsigned long long> &beg, const std::vector<uint32_t> &len, uint64_t n,
                     const pba_phase_params &P, pba_phase_row *rows_out, pba_phase_site *sites_out, pba_phase_stats *st) {
    if (n > 0x7FFFFFFFull) return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "2^31 rows or more in one call");
    if (sites->n_sel >= kPhaseMaxSel) return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "2^30 SEL sites or more");
    const uint32_t n_sel = (uint32_t)sites->n_sel;
    const size_t ns = (size_t)n_sel + 1;
    DevBuf inv, pk, d_beg, d_len, arr, cnt, d_rows, d_sites;
    EventPair ev;
    HIPCHK(hipEventCreate(&ev.e[0])); HIPCHK(hipEventCreate(&ev.e[1]));
    HIPCHK(hipMalloc(&inv.p, sizeof(uint32_t) * (sites->n + 1)));
    HIPCHK(hipMalloc(&pk.p, sizeof(uint32_t) * (n_rec + 1)));
    HIPCHK(hipMalloc(&d_beg.p, sizeof(unsigned long long) * (n + 1)));
    HIPCHK(hipMalloc(&d_len.p, sizeof(uint32_t) * (n + 1)));
    HIPCHK(hipMalloc(&arr.p, sizeof(int32_t) * 6 * ns));                   // o0, o, f, score, agree, dis
    HIPCHK(hipMalloc(&cnt.p, sizeof(uint32_t) * ((size_t)P.n_iter + 2)));  // flips of every iteration, then the bad records
    HIPCHK(hipMalloc(&d_rows.p, sizeof(pba_phase_row) * (n + 1)));
    HIPCHK(hipMalloc(&d_sites.p, sizeof(pba_phase_site) * ns));
    int32_t *o0 = arr.as<int32_t>(), *o = o0 + ns, *f = o + ns, *score = f + ns, *agree = score + ns, *dis = agree + ns;
    uint32_t *flips = cnt.as<uint32_t>(), *bad = flips + P.n_iter;
    if (n) {
        HIPCHK(hipMemcpyAsync(d_beg.p, beg.data(), sizeof(unsigned long long) * n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(d_len.p, len.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(hipMemsetAsync(inv.p, 0xFF, sizeof(uint32_t) * (sites->n + 1), ctx->stream));
    HIPCHK(hipMemsetAsync(cnt.p, 0, sizeof(uint32_t) * ((size_t)P.n_iter + 2), ctx->stream));
    HIPCHK(hipEventRecord(ev.e[0], ctx->stream));
    const dim3 tb(256);
    const dim3 g_sel(elem_grid(n_sel, 256)), g_rec(elem_grid(n_rec, 256)), g_rows(elem_grid(n * PBA_WAVE, 256));
    if (n_sel) {
        hipLaunchKernelGGL(k_phase_inverse, g_sel, tb, 0, ctx->stream, sites->d_sel, n_sel, inv.as<uint32_t>());
        hipLaunchKernelGGL(k_phase_seed, g_sel, tb, 0, ctx->stream, sites->d_sel, n_sel, P.self_weight, o0, o, f, score, agree, dis);
    }
    if (n_rec)
        hipLaunchKernelGGL(k_phase_classify, g_rec, tb, 0, ctx->stream, d_rec, (unsigned long long)n_rec, inv.as<uint32_t>(),
                           (unsigned long long)sites->n, sites->d_sel, pk.as<uint32_t>(), bad);
    HIPCHK(hipGetLastError());
    for (int k = 0; k < P.n_iter && n_sel; ++k) {
        if (n)
            hipLaunchKernelGGL(k_phase_rows<false>, g_rows, tb, 0, ctx->stream, pk.as<uint32_t>(), d_beg.as<unsigned long long>(),
                               d_len.as<uint32_t>(), (uint32_t)n, o, f, P.min_margin, (pba_phase_row *)nullptr, (int32_t *)nullptr,
                               (int32_t *)nullptr);
        hipLaunchKernelGGL(k_phase_orient, g_sel, tb, 0, ctx->stream, n_sel, P.self_weight, o0, f, o, score, flips + k);
    }
    if (n)
        hipLaunchKernelGGL(k_phase_rows<true>, g_rows, tb, 0, ctx->stream, pk.as<uint32_t>(), d_beg.as<unsigned long long>(),
                           d_len.as<uint32_t>(), (uint32_t)n, o, f, P.min_margin, d_rows.as<pba_phase_row>(), agree, dis);
    if (n_sel && sites_out)
        hipLaunchKernelGGL(k_phase_sites_out, g_sel, tb, 0, ctx->stream, sites->d_sel, n_sel, o, score, agree, dis, d_sites.as<pba_phase_site>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ev.e[1], ctx->stream));
    std::vector<uint32_t> h_cnt((size_t)P.n_iter + 2, 0u);
    HIPCHK(hipMemcpyAsync(h_cnt.data(), cnt.p, sizeof(uint32_t) * h_cnt.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (n) HIPCHK(hipMemcpyAsync(rows_out, d_rows.p, sizeof(pba_phase_row) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (n_sel && sites_out) HIPCHK(hipMemcpyAsync(sites_out, d_sites.p, sizeof(pba_phase_site) * n_sel, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (h_cnt[(size_t)P.n_iter]) {
        snprintf(ctx->err, sizeof ctx->err, "%s: %u allele records name no SEL site of the object", who, h_cnt[(size_t)P.n_iter]);
        return PBA_E_HIP;
    }
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) st->phase_ms += ms;
    st->n_rows = n; st->n_sites = n_sel; st->n_records = n_rec;
    st->n_flipped_last = P.n_iter > 0 ? h_cnt[(size_t)P.n_iter - 1] : 0u;
    for (uint64_t r = 0; r < n; ++r) {
        if (rows_out[r].label > 0) ++st->n_same; else if (rows_out[r].label < 0) ++st->n_other; else ++st->n_unphased;
    }
    return PBA_OK;
}

static int phase_args_ok(pba_ctx *ctx, const char *who, const pba_phase_params *params) {
    if (!phase_params_ok(*params))
        return ctx_fail_as(ctx, PBA_E_INVALID, who, "n_iter must be in [0, 64], min_margin at least 1, self_weight in [0, 65535]");
    return PBA_OK;
}

int pba_alleles_phase(pba_ctx *ctx, const pba_sites *sites, const pba_allele *rec, const uint64_t *off, uint64_t n,
                      const pba_phase_params *params, pba_phase_row *rows_out, pba_phase_site *sites_out, pba_phase_stats *stats) {
    static const char who[] = "pba_alleles_phase";
    if (!ctx || !sites || !params || (n && (!off || !rows_out))) return PBA_E_INVALID;
    PBA_TRY(phase_args_ok(ctx, who, params));
    pba_phase_stats st;
    memset(&st, 0, sizeof st);
    std::vector<unsigned long long> beg(n);
    std::vector<uint32_t> len(n);
    uint64_t total = 0;
    for (uint64_t r = 0; r < n; ++r) {
        if (off[r + 1] < off[r] || off[r + 1] - off[r] > 0x7FFFFFFFull) return ctx_fail_as(ctx, PBA_E_INVALID, who, "off decreases (or a row has 2^31 records or more)");
        beg[r] = off[r] - off[0]; len[r] = (uint32_t)(off[r + 1] - off[r]);
        total += len[r];
    }
    if (total && !rec) return PBA_E_INVALID;
    const pba_allele *src = n ? rec + off[0] : rec;
    for (uint64_t r = 0; r < n; ++r) {
        size_t target = 0;
        for (uint32_t x = 0; x < len[r]; ++x) {
            const pba_allele &a = src[beg[r] + x];
            if (a.site >= sites->n) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a record's site is beyond the sites of the object");
            const auto it = std::lower_bound(sites->sel_rec.begin(), sites->sel_rec.end(), a.site);
            if (it == sites->sel_rec.end() || *it != a.site) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a record's site is not a SEL record");
            if (a.allele > (uint32_t)PBA_ALLELE_DEL) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a record's allele is out of range");
            const uint64_t rank = (uint64_t)(it - sites->sel_rec.begin());
            const size_t t = (size_t)(std::upper_bound(sites->sel_off.begin(), sites->sel_off.end(), rank) - sites->sel_off.begin());
            if (x) {
                if (a.site <= src[beg[r] + x - 1].site) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's sites are not strictly ascending");
                if (t != target) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's sites are of more than one target");
            }
            target = t;
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_rec;
    HIPCHK(hipMalloc(&d_rec.p, sizeof(pba_allele) * (total + 1)));
    if (total) HIPCHK(hipMemcpyAsync(d_rec.p, src, sizeof(pba_allele) * total, hipMemcpyHostToDevice, ctx->stream));
    PBA_TRY(phase_run(ctx, who, sites, d_rec.as<pba_allele>(), total, beg, len, n, *params, rows_out, sites_out, &st));
    if (stats) *stats = st;
    return PBA_OK;
}

int pba_overlap_rows_phase_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                  uint64_t n, double R, const pba_sites *sites, const pba_phase_params *params, pba_phase_row *rows_out,
                                  pba_phase_site *sites_out, pba_phase_stats *stats, pba_result *res, uint64_t max_slots) {
    static const char who[] = "pba_overlap_rows_phase";
    if (!ctx || !reads || !sites || !params || (n && (!rows || !rows_out))) return PBA_E_INVALID;
    PBA_TRY(phase_args_ok(ctx, who, params));
    pba_phase_stats st;
    memset(&st, 0, sizeof st);
    std::vector<RowJob> jobs;
    PBA_TRY(overlap_rows_jobs(ctx, who, reads, reads_rc, rows, n, R, nullptr, res, &jobs));
    if (!sites_same_set(sites, reads)) return ctx_fail_as(ctx, PBA_E_INVALID, who, "the sites were not made from this target set");
    uint64_t room = 0;                                     // every row's bound: what the gathered records can come to at most
    for (const RowJob &jb : jobs) {
        if (jb.pr.a_seq < sites->t_lo || jb.pr.a_seq >= sites->t_hi) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's target is outside the range of the sites");
        room += pair_alleles_bound(sites, jb.pr, R);
    }
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_rec;
    HIPCHK(hipMalloc(&d_rec.p, sizeof(pba_allele) * (room + 1)));
    EventPair ev;
    HIPCHK(hipEventCreate(&ev.e[0])); HIPCHK(hipEventCreate(&ev.e[1]));
    HIPCHK(hipEventRecord(ev.e[0], ctx->stream));
    std::vector<unsigned long long> beg(n, 0ull), dst;
    std::vector<uint32_t> len(n, 0u);
    uint64_t total = 0;
    const auto sink = [&](const SlotBatch &b) -> int {
        dst.resize(b.nb);
        for (size_t q = 0; q < b.nb; ++q) {
            const uint64_t row = jobs[b.at[q]].row;
            dst[q] = beg[row] = total; len[row] = (uint32_t)b.have[q];
            total += (uint64_t)b.have[q];
        }
        if (total > room) return ctx_fail_as(ctx, PBA_E_HIP, who, "the rows hold more records than their bounds");
        DevBuf d_dst;
        HIPCHK(hipMalloc(&d_dst.p, sizeof(unsigned long long) * b.nb));
        HIPCHK(hipMemcpyAsync(d_dst.p, dst.data(), sizeof(unsigned long long) * b.nb, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_phase_gather, dim3(elem_grid((uint64_t)b.nb * PBA_WAVE, 256)), dim3(256), 0, ctx->stream, b.d->slot.as<pba_allele>(),
                           b.d->off.as<uint64_t>(), b.d->n.as<int32_t>(), d_dst.as<unsigned long long>(), (uint32_t)b.nb,
                           d_rec.as<pba_allele>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));         // (dst is reused, the batch's slots go with the batch)
        return PBA_OK;
    };
    const auto bound = [sites, R](const pba_pair &p) -> uint64_t { return pair_alleles_bound(sites, p, R); };
    const AllelesInto view = sites->view();
    const pba_seqs *const A[2] = {reads, reads}, *const B[2] = {reads, reads_rc};
    PBA_TRY(rows_chunks<pba_allele>(ctx, who, A, B, jobs, R, bound, SlotsInto{}, ~0u, nullptr, res, max_slots ? max_slots : kAlleleChunkSlots,
                                    nullptr, sink, &view, 0));
    HIPCHK(hipEventRecord(ev.e[1], ctx->stream));
    HIPCHK(hipEventSynchronize(ev.e[1]));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) st.alleles_ms = ms;
    PBA_TRY(phase_run(ctx, who, sites, d_rec.as<pba_allele>(), total, beg, len, n, *params, rows_out, sites_out, &st));
    if (stats) *stats = st;
    return PBA_OK;
}

int pba_overlap_rows_phase(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                           double R, const pba_sites *sites, const pba_phase_params *params, pba_phase_row *rows_out,
                           pba_phase_site *sites_out, pba_phase_stats *stats, pba_result *res) {
    return pba_overlap_rows_phase_budget(ctx, reads, reads_rc, rows, n, R, sites, params, rows_out, sites_out, stats, res, 0);
}

int64_t pba_phase_rows_apply(const pba_strand_overlap *rows, const pba_phase_row *phase, uint64_t n, int keep_unphased,
                             pba_strand_overlap *out_rows) {
    if (n && (!rows || !phase || !out_rows)) return -1;
    int64_t kept = 0;
    for (uint64_t k = 0; k < n; ++k)
        if (phase[k].label > 0 || (phase[k].label == 0 && keep_unphased)) out_rows[kept++] = rows[k];
    return kept;
}
