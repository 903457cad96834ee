// pba_cigar.hip -- run-length alignments (CIGAR over = X I D) for explicit pairs, mapped reads and overlap rows: the host
// side of the runs outlet of the traced bit-vector pass (align_cigar.h: CigarJob, run by k_cigar_pairs in pba_align.hip;
// TraceInto::runs through trace_batch), the compaction of a chunk's bounded slots into one dense array, and the host twins
// of the sink.  The slot runner, the chunk loop and the row layout are shared with pba_windows.hip (pba_rows.h, aln_rows.h).
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything that needs the device fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind those entry points.
//
// A run is len << 4 | op (include/pba.h).  A pair's slot is sized by pba_cigar_bound, a proven bound on the runs of a
// success; the sink never writes beyond a slot and reports the count, so a wrong bound would surface as PBA_E_HIP here.
#include "pba_rows.h"

#include <string>

// ---- the host twins of the sink ----------------------------------------------------------------------------------------
uint32_t pba_cigar_bound(int a_len, int b_len, double R) {
    if (a_len < 0 || b_len < 0 || !(R > 0.0) || !(R < 1.0)) return 0;
    const TextClip c = text_clip(a_len, b_len, R);
    const int m = std::min(c.len_a, c.len_b);
    return m > 10 ? (uint32_t)(2 * c.md - 1) : (uint32_t)c.len_a + (uint32_t)c.len_b;
}

int pba_cigar_from_script(const uint8_t *ops, int32_t nedit, const char *a_elems, const char *b_elems, uint32_t flags,
                          uint32_t *cigar, int32_t cap, pba_aln_counts *counts) {
    if (nedit < 0 || cap < 0 || (nedit && (!ops || !a_elems || !b_elems)) || (cap && !cigar)) return -1;
    const bool swap = (flags & PBA_CIG_B_IS_QUERY) != 0, rev = (flags & PBA_CIG_REVERSED) != 0;
    std::vector<uint32_t> runs;                 // origin-first
    pba_aln_counts c{0, 0, 0, 0};
    const bool ok = script_walk(ops, nedit, a_elems, b_elems, swap, [&](uint32_t code, int, int, int) {
        aln_count(c, code);
        if (!runs.empty() && (runs.back() & 15u) == code) runs.back() += 16u;
        else runs.push_back(16u | code);
        return true;
    });
    if (!ok) return -1;
    const size_t nr = runs.size();
    for (size_t x = 0; x < nr && x < (size_t)cap; ++x) cigar[x] = rev ? runs[nr - 1 - x] : runs[x];
    if (counts) *counts = c;
    return (int)nr;
}

int pba_cigar_string(const uint32_t *cigar, int32_t n, char *out, int32_t cap) {
    if (!out || cap <= 0 || n < 0 || (n && !cigar)) return 0;
    static const char kOp[16] = {'?', 'I', 'D', '?', '?', '?', '?', '=', 'X', '?', '?', '?', '?', '?', '?', '?'};
    std::string s;
    for (int32_t x = 0; x < n; ++x) { s += std::to_string(cigar[x] >> 4); s += kOp[cigar[x] & 15u]; }
    out[0] = 0;
    if (s.size() + 1 > (size_t)cap) return 0;
    memcpy(out, s.c_str(), s.size() + 1);
    return (int)s.size();
}

int pba_map_row_aln_pair(const pba_map_row *row, uint32_t contig_len, uint32_t read_len, double R, pba_pair *out) {
    if (!row || !out || !row->found || (row->strand != 1 && row->strand != -1)) return PBA_E_INVALID;
    if (!(R > 0.0) || !(R < 1.0) || row->contig < 0 || row->read < 0 || row->j < 0 || row->pos < 0) return PBA_E_INVALID;
    if (contig_len > 0x7FFFFFFFu || read_len > 0x7FFFFFFFu) return PBA_E_INVALID;
    if ((uint32_t)row->j >= read_len || (uint32_t)row->pos >= contig_len) return PBA_E_INVALID;
    // align cuts the longer side to the shorter + max_dst itself (seq_aligner.h:94-102): the same cut, made here
    const TextClip c = text_clip((int)(read_len - (uint32_t)row->j), (int)(contig_len - (uint32_t)row->pos), R);
    if (c.len_a > kMaxSeqLen || c.len_b > kMaxSeqLen) return PBA_E_TOOLONG;
    memset(out, 0, sizeof *out);
    out->a_seq = (uint32_t)row->read; out->a_pos = row->j; out->a_len = c.len_a;
    out->b_seq = (uint32_t)row->contig; out->b_pos = row->pos; out->b_len = c.len_b;
    return PBA_OK;
}

// ---- compaction: the bounded slots of a batch to one dense array -------------------------------------------------------
// exclusive scan of the run counts (a count above its slot counts as the slot: nothing was written beyond it): dense_off[0 .. n]
static __global__ void __launch_bounds__(1024)
k_cig_scan(const int32_t *ncig, const uint64_t *slot_off, uint32_t n, uint64_t *dense_off) {
    __shared__ uint32_t scan[1024];
    __shared__ uint64_t carry;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n; base += 1024) {
        const uint32_t q = base + tid;
        uint32_t cnt = 0;
        if (q < n) {
            const uint64_t have = ncig[q] > 0 ? (uint64_t)ncig[q] : 0ull, room = slot_off[q + 1] - slot_off[q];
            cnt = (uint32_t)(have < room ? have : room);
        }
        scan[tid] = cnt;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {              // inclusive scan (Hillis-Steele; once per chunk of rows, not hot)
            const uint32_t t = tid >= d ? scan[tid - d] : 0u;
            __syncthreads();
            scan[tid] += t;
            __syncthreads();
        }
        if (q < n) dense_off[q] = carry + scan[tid] - cnt;
        __syncthreads();
        if (tid == 1023) carry += scan[1023];
        __syncthreads();
    }
    if (tid == 0) dense_off[n] = carry;
}
// the gather: one wavefront per pair copies its real runs to their dense place
static __global__ void __launch_bounds__(PBA_WAVE)
k_cig_compact(const uint32_t *cig, const uint64_t *slot_off, const uint64_t *dense_off, uint32_t n, uint32_t *dense) {
    const uint32_t q = blockIdx.x;
    if (q >= n) return;
    const uint64_t from = slot_off[q], to = dense_off[q], cnt = dense_off[q + 1] - to;    // (cnt <= the slot, by the scan)
    for (uint64_t x = threadIdx.x; x < cnt; x += PBA_WAVE) dense[to + x] = cig[from + x];
}

// ---- one batch -----------------------------------------------------------------------------------------------------------
// The real runs of a finished batch, dense and in pair order, on the host (synchronised): doff[0 .. n] their offsets.  Only
// they cross to the host, not the bounded slots.  They land in *dense or, where the caller has room of its own, at `into`.
static int cigar_compact(pba_ctx *ctx, const SlotBufs &d, size_t n, std::vector<uint64_t> &doff, std::vector<uint32_t> *dense, uint32_t *into) {
    DevBuf d_doff, d_dense;
    doff.resize(n + 1);
    HIPCHK(hipMalloc(&d_doff.p, sizeof(uint64_t) * (n + 1)));
    hipLaunchKernelGGL(k_cig_scan, dim3(1), dim3(1024), 0, ctx->stream, d.n.as<int32_t>(), d.off.as<uint64_t>(), (uint32_t)n,
                       d_doff.as<uint64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(doff.data(), d_doff.p, sizeof(uint64_t) * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (dense) { dense->resize(doff[n]); into = dense->data(); }
    if (!doff[n]) return PBA_OK;
    HIPCHK(hipMalloc(&d_dense.p, sizeof(uint32_t) * doff[n]));            // (the scan's total: every gathered run lands inside)
    hipLaunchKernelGGL(k_cig_compact, dim3((uint32_t)n), dim3(PBA_WAVE), 0, ctx->stream, d.slot.as<uint32_t>(), d.off.as<uint64_t>(),
                       d_doff.as<uint64_t>(), (uint32_t)n, d_dense.as<uint32_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(into, d_dense.p, sizeof(uint32_t) * doff[n], hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

int pba_align_batch_cigar(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R,
                          int maxn, int maxm, uint32_t flags, pba_result *out, uint32_t *cigar, const uint64_t *cig_off,
                          int32_t *ncig, pba_aln_counts *counts) {
    if (!ctx || !A || !B || (n && (!pairs || !out || !cig_off || !ncig || !counts))) return PBA_E_INVALID;
    if (n == 0) return PBA_OK;
    if (flags & ~(PBA_CIG_REVERSED | PBA_CIG_B_IS_QUERY)) PBA_FAIL(PBA_E_INVALID, "pba_align_batch_cigar: unknown flag");
    if (!(R > 0.0) || !(R < 1.0)) PBA_FAIL(PBA_E_INVALID, "R must be in (0,1)");
    if (n > 0x7FFFFFFFull) PBA_FAIL(PBA_E_INVALID, "too many pairs in one batch");
    if (A->non_acgt || B->non_acgt)
        PBA_FAIL(PBA_E_ALPHABET, "a sequence set holds bytes outside ACGT: use pba_align_text_trace and pba_cigar_from_script");
    std::vector<uint64_t> rel(n + 1, 0);
    uint64_t run_max = 0;
    for (size_t q = 0; q < n; ++q) {
        if (pairs[q].a_len < 0 || pairs[q].b_len < 0) PBA_FAIL(PBA_E_INVALID, "pair outside its sequence (or longer than the engine limit)");
        const uint64_t bound = pba_cigar_bound(pairs[q].a_len, pairs[q].b_len, R);
        if (cig_off[q + 1] < cig_off[q] || cig_off[q + 1] - cig_off[q] < bound)
            PBA_FAIL(PBA_E_INVALID, "cig_off must leave pba_cigar_bound(a_len, b_len, R) slots per pair");
        rel[q + 1] = cig_off[q + 1] - cig_off[0];
        run_max = std::max(run_max, bound);
    }
    if (rel[n] && !cigar) return PBA_E_INVALID;
    SlotBufs d;
    SlotsInto extra{};
    extra.flags = flags; extra.run_max = run_max;
    PBA_TRY(slots_run<uint32_t>(ctx, A, B, pairs, n, R, maxn, maxm, extra, nullptr, rel.data(), out, ncig, counts, d));
    // The dense runs land at the head of the caller's own array and move out to their slots from the last pair down: a
    // pair's slot never starts before its dense place (every slot holds its pair's runs, so the offsets dominate), and what
    // lies behind it has moved already.  No second array on the host.
    std::vector<uint64_t> doff;
    uint32_t *const head = cigar + cig_off[0];
    PBA_TRY(cigar_compact(ctx, d, n, doff, nullptr, head));
    for (size_t q = 0; q < n; ++q)
        if (doff[q + 1] - doff[q] != (uint64_t)ncig[q] || doff[q] > rel[q]) PBA_FAIL(PBA_E_HIP, "the compaction's offsets disagree with the run counts");
    for (size_t q = n; q-- > 0;)
        if (ncig[q] && rel[q] != doff[q]) memmove(head + rel[q], head + doff[q], sizeof(uint32_t) * (size_t)ncig[q]);
    return PBA_OK;
}

// ---- rows ----------------------------------------------------------------------------------------------------------------
static const uint64_t kCigChunkSlots = 1ull << 28;      // bounded slots of one chunk of rows on the device (1 GiB)

// The jobs through the chunk loop (pba_rows.h); every batch compacted on the device, only its real runs copied to the host and
// kept per job, then laid out in row order.
static int rows_cigar(pba_ctx *ctx, const char *who, const pba_seqs *const A[2], const pba_seqs *const B[2],
                      const std::vector<RowJob> &jobs, uint64_t n_rows, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off,
                      uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots) {
    std::vector<std::vector<uint32_t>> of(jobs.size());
    std::vector<uint32_t> dense;
    std::vector<uint64_t> doff;
    const auto sink = [&](const SlotBatch &b) -> int {
        PBA_TRY(cigar_compact(ctx, *b.d, b.nb, doff, &dense, nullptr));
        for (size_t q = 0; q < b.nb; ++q) {
            if (doff[q + 1] - doff[q] != (uint64_t)b.have[q]) PBA_FAIL(PBA_E_HIP, "the compaction's offsets disagree with the run counts");
            of[b.at[q]].assign(dense.begin() + (ptrdiff_t)doff[q], dense.begin() + (ptrdiff_t)doff[q + 1]);
        }
        return PBA_OK;
    };
    const auto bound = [R](const pba_pair &p) -> uint64_t { return pba_cigar_bound(p.a_len, p.b_len, R); };
    PBA_TRY(rows_chunks<uint32_t>(ctx, who, A, B, jobs, R, bound, SlotsInto{}, 0u, counts, res, max_slots ? max_slots : kCigChunkSlots,
                                  nullptr, sink));
    rows_layout(of, job_rows(jobs), n_rows, cigar, cap, cig_off, n_slots);
    return PBA_OK;
}

// what every row-level entry point, here and in pba_windows.hip, checks before it looks at a row
static int rows_cigar_check(pba_ctx *ctx, const char *who, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_seqs *target,
                            uint64_t n, double R) {
    if (!(R > 0.0) || !(R < 1.0)) PBA_FAIL(PBA_E_INVALID, "R must be in (0,1)");
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        return ctx_fail_as(ctx, PBA_E_INVALID, who, "reads_rc differs from reads in count or lengths");
    if (reads->non_acgt || (reads_rc && reads_rc->non_acgt) || (target && target->non_acgt))
        return ctx_fail_as(ctx, PBA_E_ALPHABET, who, "a set holds bytes outside ACGT");
    if (n > 0x7FFFFFFFull) return ctx_fail_as(ctx, PBA_E_INVALID, who, "too many rows in one call");
    return PBA_OK;
}

// voting: the roles of pba_map_row_pair (a = contig), not held to the row; else pba_map_row_aln_pair's, the walk that found it
static int map_jobs(pba_ctx *ctx, const char *who, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                    const pba_map_row *rows, uint64_t n, double R, pba_aln_counts *counts, pba_result *res, std::vector<RowJob> *jobs,
                    bool voting) {
    PBA_TRY(rows_cigar_check(ctx, who, reads, reads_rc, target, n, R));
    for (uint64_t k = 0; k < n; ++k) {
        const pba_map_row &r = rows[k];
        if (counts) counts[k] = pba_aln_counts{0, 0, 0, 0};
        if (res) { memset(&res[k], 0, sizeof res[k]); res[k].rc = -1; }
        if (!r.found) continue;
        if (r.contig < 0 || (uint32_t)r.contig >= target->n) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's contig is not a contig of the set");
        if (r.read < 0 || (uint32_t)r.read >= reads->n) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's read is not a read of the set");
        if (r.strand == -1 && !reads_rc) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a strand -1 row needs reads_rc");
        RowJob jb{};
        const int st = (voting ? pba_map_row_pair : pba_map_row_aln_pair)(&r, target->h_len[r.contig], reads->h_len[r.read], R, &jb.pr);
        if (st == PBA_E_TOOLONG) return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "a row's accessor is longer than the engine limit");
        if (st != PBA_OK) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's strand or anchor is not valid for its sequences");
        jb.row = k; jb.flags = 0u; jb.batch = r.strand == 1 ? 0 : 1;
        jb.cost = r.cost; jb.matlen_a = r.matlen_a; jb.matlen_b = r.matlen_b; jb.not_held = voting ? 1 : 0;
        jobs->push_back(jb);
    }
    return PBA_OK;
}
int map_rows_jobs(pba_ctx *ctx, const char *who, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                  const pba_map_row *rows, uint64_t n, double R, pba_aln_counts *counts, pba_result *res, std::vector<RowJob> *jobs) {
    return map_jobs(ctx, who, target, reads, reads_rc, rows, n, R, counts, res, jobs, false);
}
int map_rows_vote_jobs(pba_ctx *ctx, const char *who, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                       const pba_map_row *rows, uint64_t n, double R, pba_aln_counts *counts, pba_result *res, std::vector<RowJob> *jobs) {
    return map_jobs(ctx, who, target, reads, reads_rc, rows, n, R, counts, res, jobs, true);
}

int pba_map_rows_cigar_budget(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                              const pba_map_row *rows, uint64_t n, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off,
                              uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots) {
    static const char who[] = "pba_map_rows_cigar";
    if (!ctx || !target || !reads || (!rows && n) || !cig_off || !n_slots || (cap && !cigar)) return PBA_E_INVALID;
    std::vector<RowJob> jobs;
    PBA_TRY(map_rows_jobs(ctx, who, target, reads, reads_rc, rows, n, R, counts, res, &jobs));
    const pba_seqs *const A[2] = {reads, reads_rc}, *const B[2] = {target, target};
    return rows_cigar(ctx, who, A, B, jobs, n, R, cigar, cap, cig_off, n_slots, counts, res, max_slots);
}

int pba_map_rows_cigar(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                       const pba_map_row *rows, uint64_t n, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off,
                       uint64_t *n_slots, pba_aln_counts *counts, pba_result *res) {
    return pba_map_rows_cigar_budget(ctx, target, reads, reads_rc, rows, n, R, cigar, cap, cig_off, n_slots, counts, res, 0);
}

int overlap_rows_jobs(pba_ctx *ctx, const char *who, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                      uint64_t n, double R, pba_aln_counts *counts, pba_result *res, std::vector<RowJob> *jobs) {
    PBA_TRY(rows_cigar_check(ctx, who, reads, reads_rc, nullptr, n, R));
    for (uint64_t k = 0; k < n; ++k) {
        const pba_strand_overlap &r = rows[k];
        if (counts) counts[k] = pba_aln_counts{0, 0, 0, 0};
        if (res) { memset(&res[k], 0, sizeof res[k]); res[k].rc = -1; }
        if (r.target < 0 || (uint32_t)r.target >= reads->n || r.query < 0 || (uint32_t)r.query >= reads->n)
            return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's target or query is not a read of the set");
        if (r.strand == -1 && !reads_rc) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a strand -1 row needs reads_rc");
        RowJob jb{};
        if (pba_overlap_row_pair(&r, reads->h_len[r.target], reads->h_len[r.query], &jb.pr) != PBA_OK)
            return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's accessors lie outside its reads");
        if (jb.pr.a_len > kMaxSeqLen || jb.pr.b_len > kMaxSeqLen)
            return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "a row's accessor is longer than the engine limit");
        // the target's forward order: a backward pair's goal lies at the low end of the target
        jb.row = k; jb.flags = PBA_CIG_B_IS_QUERY | (r.dir == -1 ? PBA_CIG_REVERSED : 0u); jb.batch = r.strand == 1 ? 0 : 1;
        jb.cost = r.cost; jb.matlen_a = r.matlen_a; jb.matlen_b = r.matlen_b;
        jobs->push_back(jb);
    }
    return PBA_OK;
}

int pba_overlap_rows_cigar_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                  uint64_t n, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off, uint64_t *n_slots,
                                  pba_aln_counts *counts, pba_result *res, uint64_t max_slots) {
    static const char who[] = "pba_overlap_rows_cigar";
    if (!ctx || !reads || (!rows && n) || !cig_off || !n_slots || (cap && !cigar)) return PBA_E_INVALID;
    std::vector<RowJob> jobs;
    PBA_TRY(overlap_rows_jobs(ctx, who, reads, reads_rc, rows, n, R, counts, res, &jobs));
    const pba_seqs *const A[2] = {reads, reads}, *const B[2] = {reads, reads_rc};
    return rows_cigar(ctx, who, A, B, jobs, n, R, cigar, cap, cig_off, n_slots, counts, res, max_slots);
}

int pba_overlap_rows_cigar(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                           double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off, uint64_t *n_slots, pba_aln_counts *counts,
                           pba_result *res) {
    return pba_overlap_rows_cigar_budget(ctx, reads, reads_rc, rows, n, R, cigar, cap, cig_off, n_slots, counts, res, 0);
}
