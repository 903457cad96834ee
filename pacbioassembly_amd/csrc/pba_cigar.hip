// pba_cigar.hip -- run-length alignments (CIGAR over = X I D) for explicit pairs, mapped reads and overlap rows: the host
// side of the third sink of the traced bit-vector pass (align_cigar.h: CigarSink, run by k_cigar_pairs in pba_align.hip
// through trace_batch), the compaction of a chunk's bounded slots into one dense array, and the host twins of the sink.
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything that needs the device fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind those entry points.
//
// A run is len << 4 | op (include/pba.h).  A pair's slot is sized by pba_cigar_bound, a proven bound on the runs of a
// success; the sink never writes beyond a slot and reports the count, so a wrong bound would surface as PBA_E_HIP here.
#include "pba_host.h"

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
    int i = 0, j = 0;
    for (int32_t k = 0; k < nedit; ++k) {
        uint32_t code;
        if (ops[k] == 1) { code = a_elems[i] == b_elems[j] ? PBA_CIG_EQ : PBA_CIG_X; ++i; ++j; }
        else if (ops[k] == 2) { code = swap ? PBA_CIG_INS : PBA_CIG_DEL; ++j; }       // INSERT consumes b only
        else if (ops[k] == 3) { code = swap ? PBA_CIG_DEL : PBA_CIG_INS; ++i; }       // DELETE consumes a only
        else return -1;
        if (code == PBA_CIG_EQ) ++c.n_eq; else if (code == PBA_CIG_X) ++c.n_x; else if (code == PBA_CIG_INS) ++c.n_ins; else ++c.n_del;
        if (!runs.empty() && (runs.back() & 15u) == code) runs.back() += 16u;
        else runs.push_back(16u | code);
    }
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
// The device side of a batch of runs: slot q = [off[q], off[q + 1]) of d_cig.
struct CigBufs { DevBuf cig, off, ncig, counts, pflags; };

// slots on the device, the batch through trace_batch, counts and results back on the host (synchronised)
static int cigar_run(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R, int maxn,
                     int maxm, uint32_t flags, const uint32_t *pair_flags, const uint64_t *rel_off /* n + 1, from 0 */,
                     uint64_t run_max, pba_result *out, int32_t *ncig, pba_aln_counts *counts, CigBufs &d) {
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMalloc(&d.cig.p, sizeof(uint32_t) * (rel_off[n] + 16)));
    HIPCHK(hipMalloc(&d.off.p, sizeof(uint64_t) * (n + 1)));
    HIPCHK(hipMalloc(&d.ncig.p, sizeof(int32_t) * n));
    HIPCHK(hipMalloc(&d.counts.p, sizeof(pba_aln_counts) * n));
    HIPCHK(hipMemcpyAsync(d.off.p, rel_off, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(d.ncig.p, 0, sizeof(int32_t) * n, ctx->stream));
    HIPCHK(hipMemsetAsync(d.counts.p, 0, sizeof(pba_aln_counts) * n, ctx->stream));
    if (pair_flags) {
        HIPCHK(hipMalloc(&d.pflags.p, sizeof(uint32_t) * n));
        HIPCHK(hipMemcpyAsync(d.pflags.p, pair_flags, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    }
    const CigarInto into{d.cig.as<uint32_t>(), d.off.as<uint64_t>(), d.ncig.as<int32_t>(), d.counts.as<pba_aln_counts>(),
                         d.pflags.as<uint32_t>(), flags, run_max};
    PBA_TRY(trace_batch(ctx, A, B, pairs, n, R, maxn, maxm, PBA_KERNEL_BITVEC, out, nullptr, nullptr, nullptr, nullptr, 0, &into));
    HIPCHK(hipMemcpyAsync(ncig, d.ncig.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(counts, d.counts.p, sizeof(pba_aln_counts) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; q < n; ++q)
        if (ncig[q] < 0 || (uint64_t)ncig[q] > rel_off[q + 1] - rel_off[q]) {
            snprintf(ctx->err, sizeof ctx->err, "pair %llu (a_len %d, b_len %d) has %d runs, its slot holds %llu: the run bound does not hold",
                     (unsigned long long)q, pairs[q].a_len, pairs[q].b_len, ncig[q], (unsigned long long)(rel_off[q + 1] - rel_off[q]));
            return PBA_E_HIP;
        }
    return PBA_OK;
}

// The real runs of a finished batch, dense and in pair order, on the host (synchronised): doff[0 .. n] their offsets.  Only
// they cross to the host, not the bounded slots.  They land in *dense or, where the caller has room of its own, at `into`.
static int cigar_compact(pba_ctx *ctx, const CigBufs &d, size_t n, std::vector<uint64_t> &doff, std::vector<uint32_t> *dense, uint32_t *into) {
    DevBuf d_doff, d_dense;
    doff.resize(n + 1);
    HIPCHK(hipMalloc(&d_doff.p, sizeof(uint64_t) * (n + 1)));
    hipLaunchKernelGGL(k_cig_scan, dim3(1), dim3(1024), 0, ctx->stream, d.ncig.as<int32_t>(), d.off.as<uint64_t>(), (uint32_t)n,
                       d_doff.as<uint64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(doff.data(), d_doff.p, sizeof(uint64_t) * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (dense) { dense->resize(doff[n]); into = dense->data(); }
    if (!doff[n]) return PBA_OK;
    HIPCHK(hipMalloc(&d_dense.p, sizeof(uint32_t) * doff[n]));            // (the scan's total: every gathered run lands inside)
    hipLaunchKernelGGL(k_cig_compact, dim3((uint32_t)n), dim3(PBA_WAVE), 0, ctx->stream, d.cig.as<uint32_t>(), d.off.as<uint64_t>(),
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
    CigBufs d;
    PBA_TRY(cigar_run(ctx, A, B, pairs, n, R, maxn, maxm, flags, nullptr, rel.data(), run_max, out, ncig, counts, d));
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

// The jobs (in row order) in chunks whose bounded slots stay under max_slots, each chunk as up to two batches (A[s] against
// B[s]); every batch compacted on the device, its real runs copied to the host and laid out in row order.  row_n[k]: runs
// of row k (0 for a row without a job).
static int rows_cigar(pba_ctx *ctx, const char *who, const pba_seqs *const A[2], const pba_seqs *const B[2],
                      const std::vector<RowJob> &jobs, uint64_t n_rows, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off,
                      uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots) {
    if (max_slots == 0) max_slots = kCigChunkSlots;
    std::vector<uint32_t> row_n(n_rows, 0);
    uint64_t pos = 0;                                   // dense position of the next job's runs
    bool fits = true;
    std::vector<pba_pair> pairs;
    std::vector<uint32_t> pflags, which, dense;
    std::vector<uint64_t> rel, doff;
    std::vector<pba_result> out;
    std::vector<int32_t> ncig;
    std::vector<pba_aln_counts> cnt;
    for (size_t j0 = 0; j0 < jobs.size();) {
        size_t j1 = j0;
        uint64_t slots = 0;
        while (j1 < jobs.size()) {                      // greedy take: at least one row
            const uint64_t b = pba_cigar_bound(jobs[j1].pr.a_len, jobs[j1].pr.b_len, R);
            if (j1 > j0 && slots + b > max_slots) break;
            slots += b; ++j1;
        }
        std::vector<std::vector<uint32_t>> runs_of(j1 - j0);
        for (int s = 0; s < 2; ++s) {
            pairs.clear(); pflags.clear(); which.clear(); rel.assign(1, 0);
            uint64_t run_max = 0;
            for (size_t j = j0; j < j1; ++j) {
                if (jobs[j].batch != s) continue;
                const uint64_t b = pba_cigar_bound(jobs[j].pr.a_len, jobs[j].pr.b_len, R);
                pairs.push_back(jobs[j].pr); pflags.push_back(jobs[j].flags); which.push_back((uint32_t)(j - j0));
                rel.push_back(rel.back() + b);
                run_max = std::max(run_max, b);
            }
            const size_t nb = pairs.size();
            if (!nb) continue;
            out.resize(nb); ncig.resize(nb); cnt.resize(nb);
            CigBufs d;
            PBA_TRY(cigar_run(ctx, A[s], B[s], pairs.data(), nb, R, 0, 0, 0u, pflags.data(), rel.data(), run_max, out.data(),
                              ncig.data(), cnt.data(), d));
            for (size_t q = 0; q < nb; ++q) {           // held to the row: the same roles, the same lengths, the same R
                const RowJob &jb = jobs[j0 + which[q]];
                if (res) res[jb.row] = out[q];
                if (counts) counts[jb.row] = cnt[q];
                if (!walk_agrees(out[q], jb.cost, jb.matlen_a, jb.matlen_b)) {
                    snprintf(ctx->err, sizeof ctx->err,
                             "%s: row %llu re-runs to rc %d cost %d matlen %d/%d, the row says cost %d matlen %d/%d: not a row of these "
                             "sets under this R", who, (unsigned long long)jb.row, out[q].rc, out[q].cost, out[q].matlen_a,
                             out[q].matlen_b, jb.cost, jb.matlen_a, jb.matlen_b);
                    return PBA_E_INVALID;
                }
            }
            PBA_TRY(cigar_compact(ctx, d, nb, doff, &dense, nullptr));
            for (size_t q = 0; q < nb; ++q) {
                if (doff[q + 1] - doff[q] != (uint64_t)ncig[q]) PBA_FAIL(PBA_E_HIP, "the compaction's offsets disagree with the run counts");
                runs_of[which[q]].assign(dense.begin() + (ptrdiff_t)doff[q], dense.begin() + (ptrdiff_t)doff[q + 1]);
            }
        }
        for (size_t j = j0; j < j1; ++j) {              // row order; whole rows only, up to the first that does not fit
            const std::vector<uint32_t> &r = runs_of[j - j0];
            row_n[jobs[j].row] = (uint32_t)r.size();
            if (fits && pos + r.size() <= cap) { if (!r.empty()) memcpy(cigar + pos, r.data(), sizeof(uint32_t) * r.size()); }
            else fits = false;
            pos += r.size();
        }
        j0 = j1;
    }
    cig_off[0] = 0;
    for (uint64_t k = 0; k < n_rows; ++k) cig_off[k + 1] = cig_off[k] + row_n[k];
    *n_slots = cig_off[n_rows];
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

int map_rows_jobs(pba_ctx *ctx, const char *who, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                  const pba_map_row *rows, uint64_t n, double R, pba_aln_counts *counts, pba_result *res, std::vector<RowJob> *jobs) {
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
        const int st = pba_map_row_aln_pair(&r, target->h_len[r.contig], reads->h_len[r.read], R, &jb.pr);
        if (st == PBA_E_TOOLONG) return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "a row's accessor is longer than the engine limit");
        if (st != PBA_OK) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's strand or anchor is not valid for its sequences");
        jb.row = k; jb.flags = 0u; jb.batch = r.strand == 1 ? 0 : 1;
        jb.cost = r.cost; jb.matlen_a = r.matlen_a; jb.matlen_b = r.matlen_b;
        jobs->push_back(jb);
    }
    return PBA_OK;
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
