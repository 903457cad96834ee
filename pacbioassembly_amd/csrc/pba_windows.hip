// pba_windows.hip -- per-window alignment counts and rows trimmed where they break (include/pba.h): the host side
// of the windows outlet of the traced bit-vector pass (align_windows.h: WindowJob, run by k_window_pairs in pba_align.hip;
// TraceInto::windows through trace_batch), the trim kernel over windows, the host twins of both, and the row-level entry
// points.  The slot runner, the chunk loop and the row layout are shared with pba_cigar.hip (pba_rows.h, aln_rows.h).
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything that needs the device fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind those entry points.
//
// A window is one pba_aln_counts.  A pair's slot is sized by pba_windows_bound, the windows its clipped len_a touches; the
// sink knows n_win from the goal cell, never writes beyond a slot and reports the count, so a wrong bound would surface as
// PBA_E_HIP here.
#include "pba_rows.h"

static const uint32_t kWinFlags = PBA_CIG_REVERSED | PBA_CIG_B_IS_QUERY;

// ---- the host twins of the sink ----------------------------------------------------------------------------------------
// the local window index of a-element e (e >= 0; x(e) >= 0 is the caller's)
static inline int window_of(int a_pos, int a_backward, int W, int e) {
    const int g = (a_backward ? a_pos - e : a_pos + e) / W - a_pos / W;
    return g < 0 ? -g : g;
}

uint32_t pba_windows_bound(int a_pos, int a_len, int b_len, double R, int W, int a_backward) {
    if (W < 1 || a_pos < 0 || a_len < 0 || b_len < 0 || !(R > 0.0) || !(R < 1.0)) return 0;
    const int la = text_clip(a_len, b_len, R).len_a, last = std::max(la - 1, 0);
    if (a_backward ? a_pos - last < 0 : (long long)a_pos + last > 0x7FFFFFFFll) return 0;
    return (uint32_t)window_of(a_pos, a_backward, W, last) + 1u;
}

int pba_windows_from_script(const uint8_t *ops, int32_t nedit, const char *a_elems, const char *b_elems, int a_pos, int a_backward,
                            int W, uint32_t flags, pba_aln_counts *win, int32_t cap) {
    if (nedit < 0 || cap < 0 || W < 1 || a_pos < 0 || (flags & ~kWinFlags) || (nedit && (!ops || !a_elems || !b_elems)) || (cap && !win)) return -1;
    const bool swap = (flags & PBA_CIG_B_IS_QUERY) != 0, rev = (flags & PBA_CIG_REVERSED) != 0;
    std::vector<pba_aln_counts> w(1, pba_aln_counts{0, 0, 0, 0});       // origin-first
    const bool ok = script_walk(ops, nedit, a_elems, b_elems, swap, [&](uint32_t code, int op, int i, int) {
        const int e = op == 2 ? std::max(i - 1, 0) : i;                 // INSERT: the a-element before it
        if (a_backward && a_pos - e < 0) return false;
        const size_t at = (size_t)window_of(a_pos, a_backward, W, e);
        if (at >= w.size()) w.resize(at + 1, pba_aln_counts{0, 0, 0, 0});
        aln_count(w[at], code);
        return true;
    });
    if (!ok) return -1;
    const size_t nw = w.size();
    for (size_t x = 0; x < nw && x < (size_t)cap; ++x) win[x] = rev ? w[nw - 1 - x] : w[x];
    return (int)nw;
}

// ---- one batch -----------------------------------------------------------------------------------------------------------
static inline uint64_t pair_windows_bound(const pba_pair &p, double R, int W) {
    return pba_windows_bound(p.a_pos, p.a_len, p.b_len, R, W, (p.flags & PBA_A_BACKWARD) != 0);
}

int pba_align_batch_windows(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R, int maxn,
                            int maxm, int W, uint32_t flags, pba_result *out, pba_aln_counts *win, const uint64_t *win_off,
                            int32_t *nwin, pba_aln_counts *counts) {
    if (!ctx || !A || !B || (n && (!pairs || !out || !win_off || !nwin || !counts))) return PBA_E_INVALID;
    if (W < 1) PBA_FAIL(PBA_E_INVALID, "pba_align_batch_windows: W must be at least 1");
    if (flags & ~kWinFlags) PBA_FAIL(PBA_E_INVALID, "pba_align_batch_windows: unknown flag");
    if (n == 0) return PBA_OK;
    if (!(R > 0.0) || !(R < 1.0)) PBA_FAIL(PBA_E_INVALID, "R must be in (0,1)");
    if (n > 0x7FFFFFFFull) PBA_FAIL(PBA_E_INVALID, "too many pairs in one batch");
    if (A->non_acgt || B->non_acgt)
        PBA_FAIL(PBA_E_ALPHABET, "a sequence set holds bytes outside ACGT: use pba_align_text_trace and pba_windows_from_script");
    std::vector<uint64_t> rel(n + 1, 0);
    for (size_t q = 0; q < n; ++q) {
        if (pairs[q].a_len < 0 || pairs[q].b_len < 0 || pairs[q].a_pos < 0) PBA_FAIL(PBA_E_INVALID, "pair outside its sequence (or longer than the engine limit)");
        const uint64_t bound = pair_windows_bound(pairs[q], R, W);
        if (bound == 0) PBA_FAIL(PBA_E_INVALID, "pair outside its sequence (or longer than the engine limit)");
        if (win_off[q + 1] < win_off[q] || win_off[q + 1] - win_off[q] < bound)
            PBA_FAIL(PBA_E_INVALID, "win_off must leave pba_windows_bound(a_pos, a_len, b_len, R, W, a_backward) slots per pair");
        rel[q + 1] = win_off[q + 1] - win_off[0];
    }
    if (rel[n] && !win) return PBA_E_INVALID;
    SlotBufs d;
    SlotsInto extra{};
    extra.flags = flags; extra.W = W;
    PBA_TRY(slots_run<pba_aln_counts>(ctx, A, B, pairs, n, R, maxn, maxm, extra, nullptr, rel.data(), out, nwin, counts, d));
    // only what a pair has goes to the caller's array: the rest of a slot, and the slot of a failing pair, stay untouched
    std::vector<pba_aln_counts> h(rel[n] + 1);
    HIPCHK(hipMemcpyAsync(h.data(), d.slot.p, sizeof(pba_aln_counts) * rel[n], hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; q < n; ++q)
        if (nwin[q]) memcpy(win + win_off[q], h.data() + rel[q], sizeof(pba_aln_counts) * (size_t)nwin[q]);
    return PBA_OK;
}

// ---- the trim kernel -------------------------------------------------------------------------------------------------------
// One wavefront per item, 64 windows to a step: the good mask is a ballot, the runs come from it by ctz, the sums of
// a-elements, b-elements and errors before every window from a wave scan; the open run and the best run so far are carried
// wave-uniform across steps.  Item q: win[off[q] ..), nwin[q] windows (nwin nullable: all of [off[q], off[q + 1])).  No
// floating point: thr[m] for m = 0 .. thr_max is the host's.
struct TrimRun { int beg, a0, b0, e0; };
static __global__ void __launch_bounds__(PBA_WAVE)
k_trim_rows(const pba_aln_counts *win, const uint64_t *off, const int32_t *nwin, uint32_t n, const int32_t *thr, int thr_max,
            int min_span, pba_trim_span *spans) {
    const uint32_t q = blockIdx.x;
    if (q >= n) return;
    const int lane = threadIdx.x & (PBA_WAVE - 1);
    const uint64_t o0 = off[q], room = off[q + 1] - o0;
    int nw = nwin ? nwin[q] : (int)(room < 0x7FFFFFFFull ? room : 0x7FFFFFFFull);
    if (nw < 0) nw = 0;
    if ((uint64_t)nw > room) nw = (int)room;                               // never beyond the item's own windows
    nw = __builtin_amdgcn_readfirstlane(nw);
    int pre_a = 0, pre_b = 0, pre_e = 0, n_good = 0, n_runs = 0;
    bool open = false;
    TrimRun run{0, 0, 0, 0};
    int best_na = -1, best_beg = 0, best_end = 0, best_a0 = 0, best_b0 = 0, best_nb = 0, best_cost = 0;
    auto close = [&](int end, int a1, int b1, int e1) {                    // the open run ends before window `end`
        ++n_runs;
        const int na = a1 - run.a0;
        if (na > best_na) {                                                // strictly: a tie stays with the first
            best_na = na; best_beg = run.beg; best_end = end; best_a0 = run.a0; best_b0 = run.b0; best_nb = b1 - run.b0; best_cost = e1 - run.e0;
        }
        open = false;
    };
    for (int base = 0; base < nw; base += PBA_WAVE) {
        const int cnt = min(PBA_WAVE, nw - base);
        int a = 0, b = 0, e = 0;
        bool good = false;
        if (lane < cnt) {
            const int4 v = *(const int4 *)(win + o0 + (uint64_t)(base + lane));
            a = v.x + v.y + v.z; b = v.x + v.y + v.w; e = v.y + v.z + v.w;
            good = e <= thr[min(max(a, 0), thr_max)];
        }
        uint64_t m = __builtin_amdgcn_ballot_w64(good);
        n_good += __builtin_popcountll(m);
        int sa = a, sb = b, se = e;                                        // inclusive scans (lanes beyond cnt add nothing)
#pragma unroll
        for (int d = 1; d < PBA_WAVE; d <<= 1) {
            const int ta = __shfl_up(sa, d, PBA_WAVE), tb = __shfl_up(sb, d, PBA_WAVE), te = __shfl_up(se, d, PBA_WAVE);
            if (lane >= d) { sa += ta; sb += tb; se += te; }
        }
        const int xa = pre_a + sa - a, xb = pre_b + sb - b, xe = pre_e + se - e;   // the sums before this lane's window
        for (;;) {
            int s = 0;                                                     // a carried run goes on from lane 0, if that is good
            if (!open) {
                if (m == 0ull) break;
                s = (int)__builtin_ctzll(m);
                open = true;
                run.beg = base + s;
                run.a0 = __builtin_amdgcn_readlane(xa, s); run.b0 = __builtin_amdgcn_readlane(xb, s); run.e0 = __builtin_amdgcn_readlane(xe, s);
            }
            const uint64_t z = ~(m >> s);                                  // the first window at or after s that is not good
            const int end = s + (z ? (int)__builtin_ctzll(z) : PBA_WAVE);
            if (end >= PBA_WAVE) break;                                    // still open at the step's edge (a lane beyond cnt is not good)
            close(base + end, __builtin_amdgcn_readlane(xa, end), __builtin_amdgcn_readlane(xb, end), __builtin_amdgcn_readlane(xe, end));
            m = (m >> end) << end;
        }
        pre_a += __builtin_amdgcn_readlane(sa, PBA_WAVE - 1); pre_b += __builtin_amdgcn_readlane(sb, PBA_WAVE - 1);
        pre_e += __builtin_amdgcn_readlane(se, PBA_WAVE - 1);
    }
    if (open) close(nw, pre_a, pre_b, pre_e);
    if (lane == 0) {
        pba_trim_span o{PBA_TRIM_DROPPED, nw, n_good, n_runs, 0, 0, 0, 0, 0, 0, 0};
        if (n_runs > 0 && best_na >= min_span && best_nb != 0) {
            o.state = best_beg == 0 && best_end == nw ? PBA_TRIM_WHOLE : PBA_TRIM_CUT;
            o.w_beg = best_beg; o.w_end = best_end; o.a0 = best_a0; o.b0 = best_b0; o.na = best_na; o.nb = best_nb; o.cost = best_cost;
        }
        spans[q] = o;
    }
}

// thr[m] = (int32_t)(max_err * (double)m) for m = 0 .. thr_max, on the device (the caller owns d_thr)
static int trim_table(pba_ctx *ctx, double max_err, int thr_max, DevBuf &d_thr) {
    std::vector<int32_t> thr((size_t)thr_max + 1);
    for (int m = 0; m <= thr_max; ++m) thr[(size_t)m] = (int32_t)(max_err * (double)m);
    HIPCHK(hipMalloc(&d_thr.p, sizeof(int32_t) * thr.size()));
    HIPCHK(hipMemcpyAsync(d_thr.p, thr.data(), sizeof(int32_t) * thr.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));                             // (thr is a local)
    return PBA_OK;
}
static int trim_args_ok(pba_ctx *ctx, const char *who, int W, double max_err, int min_span) {
    if (W < 1) return ctx_fail_as(ctx, PBA_E_INVALID, who, "W must be at least 1");
    if (!(max_err >= 0.0) || !(max_err <= 1.0)) return ctx_fail_as(ctx, PBA_E_INVALID, who, "max_err must be in [0, 1]");
    if (min_span < 0) return ctx_fail_as(ctx, PBA_E_INVALID, who, "min_span must not be negative");
    return PBA_OK;
}

int pba_windows_trim(pba_ctx *ctx, const pba_aln_counts *win, const uint64_t *win_off, uint64_t n, int W, double max_err, int min_span,
                     pba_trim_span *spans) {
    static const char who[] = "pba_windows_trim";
    if (!ctx || (n && (!win_off || !spans))) return PBA_E_INVALID;
    PBA_TRY(trim_args_ok(ctx, who, W, max_err, min_span));
    if (n == 0) return PBA_OK;
    if (n > 0x7FFFFFFFull) return ctx_fail_as(ctx, PBA_E_INVALID, who, "too many items in one call");
    std::vector<uint64_t> rel(n + 1, 0);
    for (uint64_t q = 0; q < n; ++q) {
        if (win_off[q + 1] < win_off[q] || win_off[q + 1] - win_off[q] > 0x7FFFFFFFull) return ctx_fail_as(ctx, PBA_E_INVALID, who, "win_off decreases (or an item has 2^31 windows or more)");
        rel[q + 1] = win_off[q + 1] - win_off[0];
    }
    if (rel[n] && !win) return PBA_E_INVALID;
    const pba_aln_counts *src = win + win_off[0];
    int na_max = 0;
    for (uint64_t x = 0; x < rel[n]; ++x) {
        const pba_aln_counts &c = src[x];
        if (c.n_eq < 0 || c.n_x < 0 || c.n_ins < 0 || c.n_del < 0) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a window holds a negative count");
        const int64_t na = (int64_t)c.n_eq + c.n_x + c.n_ins;
        if (na > W) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a window consumes more than W a-elements");
        na_max = std::max(na_max, (int)na);
    }
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_win, d_off, d_thr, d_spans;
    HIPCHK(hipMalloc(&d_win.p, sizeof(pba_aln_counts) * (rel[n] + 1)));
    HIPCHK(hipMalloc(&d_off.p, sizeof(uint64_t) * (n + 1)));
    HIPCHK(hipMalloc(&d_spans.p, sizeof(pba_trim_span) * n));
    if (rel[n]) HIPCHK(hipMemcpyAsync(d_win.p, src, sizeof(pba_aln_counts) * rel[n], hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_off.p, rel.data(), sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    PBA_TRY(trim_table(ctx, max_err, na_max, d_thr));
    hipLaunchKernelGGL(k_trim_rows, dim3((uint32_t)n), dim3(PBA_WAVE), 0, ctx->stream, d_win.as<pba_aln_counts>(), d_off.as<uint64_t>(),
                       (const int32_t *)nullptr, (uint32_t)n, d_thr.as<int32_t>(), na_max, min_span, d_spans.as<pba_trim_span>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(spans, d_spans.p, sizeof(pba_trim_span) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

// ---- rows ----------------------------------------------------------------------------------------------------------------
static const uint64_t kWinChunkSlots = 1ull << 26;      // bounded window slots of one chunk of rows on the device (1 GiB)

// the windows of a chunk loop (pba_rows.h) over the jobs' pairs under W
static int rows_windows(pba_ctx *ctx, const char *who, const pba_seqs *const A[2], const pba_seqs *const B[2], const std::vector<RowJob> &jobs,
                        double R, int W, uint32_t drop_flags, pba_aln_counts *counts, pba_result *res, uint64_t max_slots, uint32_t *n_chunks,
                        const std::function<int(const SlotBatch &)> &sink) {
    SlotsInto extra{};
    extra.W = W;
    const auto bound = [R, W](const pba_pair &p) -> uint64_t { return pair_windows_bound(p, R, W); };
    return rows_chunks<pba_aln_counts>(ctx, who, A, B, jobs, R, bound, extra, drop_flags, counts, res, max_slots ? max_slots : kWinChunkSlots,
                                       n_chunks, sink);
}

// the windows of the jobs dense and in row order on the host: every job's windows kept until the rows are laid out
static int rows_windows_out(pba_ctx *ctx, const char *who, const pba_seqs *const A[2], const pba_seqs *const B[2],
                            const std::vector<RowJob> &jobs, uint64_t n_rows, double R, int W, pba_aln_counts *win, uint64_t cap,
                            uint64_t *win_off, uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots) {
    std::vector<std::vector<pba_aln_counts>> of(jobs.size());
    std::vector<pba_aln_counts> h;
    const auto sink = [&](const SlotBatch &b) -> int {
        h.resize(b.rel[b.nb] + 1);
        HIPCHK(hipMemcpyAsync(h.data(), b.d->slot.p, sizeof(pba_aln_counts) * b.rel[b.nb], hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (size_t q = 0; q < b.nb; ++q) of[b.at[q]].assign(h.begin() + (ptrdiff_t)b.rel[q], h.begin() + (ptrdiff_t)(b.rel[q] + (uint64_t)b.have[q]));
        return PBA_OK;
    };
    PBA_TRY(rows_windows(ctx, who, A, B, jobs, R, W, 0u, counts, res, max_slots, nullptr, sink));
    rows_layout(of, job_rows(jobs), n_rows, win, cap, win_off, n_slots);
    return PBA_OK;
}

int pba_map_rows_windows_budget(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                                const pba_map_row *rows, uint64_t n, double R, int W, pba_aln_counts *win, uint64_t cap,
                                uint64_t *win_off, uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots) {
    static const char who[] = "pba_map_rows_windows";
    if (!ctx || !target || !reads || (!rows && n) || !win_off || !n_slots || (cap && !win)) return PBA_E_INVALID;
    if (W < 1) return ctx_fail_as(ctx, PBA_E_INVALID, who, "W must be at least 1");
    std::vector<RowJob> jobs;
    PBA_TRY(map_rows_jobs(ctx, who, target, reads, reads_rc, rows, n, R, counts, res, &jobs));
    const pba_seqs *const A[2] = {reads, reads_rc}, *const B[2] = {target, target};
    return rows_windows_out(ctx, who, A, B, jobs, n, R, W, win, cap, win_off, n_slots, counts, res, max_slots);
}

int pba_map_rows_windows(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_map_row *rows,
                         uint64_t n, double R, int W, pba_aln_counts *win, uint64_t cap, uint64_t *win_off, uint64_t *n_slots,
                         pba_aln_counts *counts, pba_result *res) {
    return pba_map_rows_windows_budget(ctx, target, reads, reads_rc, rows, n, R, W, win, cap, win_off, n_slots, counts, res, 0);
}

int pba_overlap_rows_windows_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                    uint64_t n, double R, int W, pba_aln_counts *win, uint64_t cap, uint64_t *win_off,
                                    uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots) {
    static const char who[] = "pba_overlap_rows_windows";
    if (!ctx || !reads || (!rows && n) || !win_off || !n_slots || (cap && !win)) return PBA_E_INVALID;
    if (W < 1) return ctx_fail_as(ctx, PBA_E_INVALID, who, "W must be at least 1");
    std::vector<RowJob> jobs;
    PBA_TRY(overlap_rows_jobs(ctx, who, reads, reads_rc, rows, n, R, counts, res, &jobs));
    const pba_seqs *const A[2] = {reads, reads}, *const B[2] = {reads, reads_rc};
    return rows_windows_out(ctx, who, A, B, jobs, n, R, W, win, cap, win_off, n_slots, counts, res, max_slots);
}

int pba_overlap_rows_windows(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                             double R, int W, pba_aln_counts *win, uint64_t cap, uint64_t *win_off, uint64_t *n_slots,
                             pba_aln_counts *counts, pba_result *res) {
    return pba_overlap_rows_windows_budget(ctx, reads, reads_rc, rows, n, R, W, win, cap, win_off, n_slots, counts, res, 0);
}

// ---- rows trimmed ----------------------------------------------------------------------------------------------------------
// a span over a row's windows (target forward, I / D under the default flags: a = the target) as the row's trimmed intervals
static pba_trim_row trim_row_of(const pba_strand_overlap &r, int32_t slen, const pba_trim_span &s) {
    pba_trim_row o{s.state, s.n_win, s.n_good, s.n_runs, s.w_beg, s.w_end, 0, 0, 0, 0, s.cost};
    if (s.state == PBA_TRIM_DROPPED) return o;
    // element order is the reverse of the target's order for dir -1: what lies before the run there lies behind it here
    const int32_t a0 = r.dir == 1 ? s.a0 : r.matlen_a - s.a0 - s.na, b0 = r.dir == 1 ? s.b0 : r.matlen_b - s.b0 - s.nb;
    int32_t w0, w1;                                    // on the query text that was walked
    if (r.dir == 1) { o.t_beg = r.t_beg + a0; o.t_end = o.t_beg + s.na; w0 = r.j + b0; w1 = w0 + s.nb; }
    else { o.t_end = r.t_end - a0; o.t_beg = o.t_end - s.na; w1 = slen - r.j - b0; w0 = w1 - s.nb; }
    if (r.strand == 1) { o.q_beg = w0; o.q_end = w1; } else { o.q_beg = slen - w1; o.q_end = slen - w0; }
    return o;
}

int pba_overlap_rows_trim_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                 uint64_t n, double R, int W, double max_err, int min_span, pba_trim_row *out, pba_trim_stats *stats,
                                 uint64_t max_slots) {
    static const char who[] = "pba_overlap_rows_trim";
    if (!ctx || !reads || (n && (!rows || !out))) return PBA_E_INVALID;
    PBA_TRY(trim_args_ok(ctx, who, W, max_err, min_span));
    pba_trim_stats st;
    memset(&st, 0, sizeof st);
    st.n_rows = n;
    if (stats) *stats = st;
    std::vector<RowJob> jobs;
    PBA_TRY(overlap_rows_jobs(ctx, who, reads, reads_rc, rows, n, R, nullptr, nullptr, &jobs));
    if (n == 0) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    DevBuf d_thr;
    const int thr_max = std::min(W, kMaxSeqLen);        // (a window consumes at most W a-elements, an accessor holds kMaxSeqLen)
    PBA_TRY(trim_table(ctx, max_err, thr_max, d_thr));
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 3; ++k) if (e[k]) (void)hipEventDestroy(e[k]); } } guard{ev};
    for (int k = 0; k < 3; ++k) HIPCHK(hipEventCreate(&ev[k]));
    HIPCHK(hipEventRecord(ev[0], ctx->stream));         // (a chunk's traced pass runs from the end of the trim before it)
    std::vector<pba_trim_span> spans;
    const auto sink = [&](const SlotBatch &b) -> int {
        DevBuf d_spans;
        HIPCHK(hipMalloc(&d_spans.p, sizeof(pba_trim_span) * b.nb));
        HIPCHK(hipEventRecord(ev[1], ctx->stream));
        hipLaunchKernelGGL(k_trim_rows, dim3((uint32_t)b.nb), dim3(PBA_WAVE), 0, ctx->stream, b.d->slot.as<pba_aln_counts>(),
                           b.d->off.as<uint64_t>(), b.d->n.as<int32_t>(), (uint32_t)b.nb, d_thr.as<int32_t>(), thr_max, min_span,
                           d_spans.as<pba_trim_span>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[2], ctx->stream));
        spans.resize(b.nb);
        HIPCHK(hipMemcpyAsync(spans.data(), d_spans.p, sizeof(pba_trim_span) * b.nb, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) st.windows_ms += ms;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) st.trim_ms += ms;
        HIPCHK(hipEventRecord(ev[0], ctx->stream));
        for (size_t q = 0; q < b.nb; ++q) {
            const RowJob &jb = jobs[b.at[q]];
            const pba_strand_overlap &r = rows[jb.row];
            out[jb.row] = trim_row_of(r, (int32_t)reads->h_len[r.query], spans[q]);
            st.n_windows += (uint64_t)spans[q].n_win;
            if (spans[q].state == PBA_TRIM_WHOLE) ++st.n_whole; else if (spans[q].state == PBA_TRIM_CUT) ++st.n_cut; else ++st.n_dropped;
        }
        return PBA_OK;
    };
    const pba_seqs *const A[2] = {reads, reads}, *const B[2] = {reads, reads_rc};
    // (default naming for the rule: I consumes a, the target; the order stays the target's)
    PBA_TRY(rows_windows(ctx, who, A, B, jobs, R, W, PBA_CIG_B_IS_QUERY, nullptr, nullptr, max_slots, &st.n_chunks, sink));
    if (stats) *stats = st;
    return PBA_OK;
}

int pba_overlap_rows_trim(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                          double R, int W, double max_err, int min_span, pba_trim_row *out, pba_trim_stats *stats) {
    return pba_overlap_rows_trim_budget(ctx, reads, reads_rc, rows, n, R, W, max_err, min_span, out, stats, 0);
}

int64_t pba_trim_rows_apply(const pba_strand_overlap *rows, const pba_trim_row *trims, uint64_t n, pba_strand_overlap *out_rows) {
    if (n && (!rows || !trims || !out_rows)) return -1;
    int64_t kept = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (trims[k].state == PBA_TRIM_DROPPED) continue;
        pba_strand_overlap r = rows[k];
        r.t_beg = trims[k].t_beg; r.t_end = trims[k].t_end; r.q_beg = trims[k].q_beg; r.q_end = trims[k].q_end;
        out_rows[kept++] = r;
    }
    return kept;
}
