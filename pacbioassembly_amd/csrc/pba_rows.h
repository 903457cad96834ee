// pba_rows.h -- the host side the bounded-slot outlets of the traced pass share (pba_cigar.hip: runs, T = uint32_t;
// pba_windows.hip: per-window counts, T = pba_aln_counts; pba_sites.hip: alleles at selection sites, T = pba_allele): one batch
// of slots through trace_batch, and the chunk loop of the row-level entry points (a job marked not_held is not held to its row).
// (The script walker and the row layout need no device: aln_rows.h.)  Behind them the sites object and the slot bound of the
// alleles outlet, which pba_sites.hip and pba_phase.hip share.  Host code only.
#ifndef PBA_ROWS_H
#define PBA_ROWS_H

#include "aln_rows.h"
#include "pba_host.h"

// The device side of a batch of slots: slot q = [off[q], off[q + 1]) of `slot`, n[q] elements in it.
struct SlotBufs { DevBuf slot, off, n, counts, pflags; };

// Slots on the device, the batch through trace_batch, counts and results back on the host (synchronised); the elements stay
// on the device.  extra: run_max (runs) or W (windows), and the flags of every pair where pair_flags is null; sites and gate:
// alleles only (counts then carry n_own, n_major, n_minor, n_other in their four ints).  Every count is held to its slot: the
// sinks never write beyond one, so a bound that does not hold surfaces here as PBA_E_HIP.
template <class T> struct SlotKind;      // what the slots of T hold: the outlet, its words for the message, the slack behind the slots
template <> struct SlotKind<uint32_t> { static constexpr TraceInto::Kind kind = TraceInto::RUNS; static constexpr int pad = 16; static constexpr const char *many = "runs", *one = "run"; };
template <> struct SlotKind<pba_aln_counts> { static constexpr TraceInto::Kind kind = TraceInto::WINDOWS; static constexpr int pad = 1; static constexpr const char *many = "windows", *one = "window"; };
template <> struct SlotKind<pba_allele> { static constexpr TraceInto::Kind kind = TraceInto::ALLELES; static constexpr int pad = 1; static constexpr const char *many = "alleles", *one = "site"; };
template <class T>
static int slots_run(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R, int maxn, int maxm,
                     SlotsInto extra, const uint32_t *pair_flags, const uint64_t *rel_off /* n + 1, from 0 */, pba_result *out,
                     int32_t *have, pba_aln_counts *counts, SlotBufs &d, const AllelesInto *sites = nullptr, int gate = 0) {
    using K = SlotKind<T>;
    constexpr bool windows = K::kind != TraceInto::RUNS;      // the pair's a_pos matters to the bound
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMalloc(&d.slot.p, sizeof(T) * (rel_off[n] + K::pad)));
    HIPCHK(hipMalloc(&d.off.p, sizeof(uint64_t) * (n + 1)));
    HIPCHK(hipMalloc(&d.n.p, sizeof(int32_t) * n));
    HIPCHK(hipMalloc(&d.counts.p, sizeof(pba_aln_counts) * n));
    HIPCHK(hipMemcpyAsync(d.off.p, rel_off, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemsetAsync(d.n.p, 0, sizeof(int32_t) * n, ctx->stream));
    HIPCHK(hipMemsetAsync(d.counts.p, 0, sizeof(pba_aln_counts) * n, ctx->stream));
    if (pair_flags) {
        HIPCHK(hipMalloc(&d.pflags.p, sizeof(uint32_t) * n));
        HIPCHK(hipMemcpyAsync(d.pflags.p, pair_flags, sizeof(uint32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    }
    extra.slot = d.slot.p; extra.off = d.off.as<uint64_t>(); extra.n = d.n.as<int32_t>(); extra.counts = d.counts.as<pba_aln_counts>();
    extra.pair_flags = d.pflags.as<uint32_t>();
    PBA_TRY(trace_batch(ctx, A, B, pairs, n, R, maxn, maxm, PBA_KERNEL_BITVEC, out,
                        K::kind == TraceInto::ALLELES ? TraceInto::alleles(extra, *sites, gate)
                                                      : (K::kind == TraceInto::WINDOWS ? TraceInto::windows(extra) : TraceInto::runs(extra))));
    HIPCHK(hipMemcpyAsync(have, d.n.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(counts, d.counts.p, sizeof(pba_aln_counts) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; q < n; ++q)
        if (have[q] < 0 || (uint64_t)have[q] > rel_off[q + 1] - rel_off[q]) {
            char pair[96];
            if (windows) snprintf(pair, sizeof pair, "a_pos %d, a_len %d, b_len %d", pairs[q].a_pos, pairs[q].a_len, pairs[q].b_len);
            else snprintf(pair, sizeof pair, "a_len %d, b_len %d", pairs[q].a_len, pairs[q].b_len);
            snprintf(ctx->err, sizeof ctx->err, "pair %llu (%s) has %d %s, its slot holds %llu: the %s bound does not hold", (unsigned long long)q,
                     pair, have[q], K::many, (unsigned long long)(rel_off[q + 1] - rel_off[q]), K::one);
            return PBA_E_HIP;
        }
    return PBA_OK;
}

// What a finished batch of a chunk hands on: its device arrays, its pairs' slots (rel, from 0) and counts, and which job of
// `jobs` pair q is (jobs[at[q]]).
struct SlotBatch { const SlotBufs *d; size_t nb; const uint64_t *rel; const int32_t *have; const size_t *at; };

// The rows driver: the jobs (in row order) in chunks whose bounded slots (bound(pair) each) stay under max_slots, each chunk as
// up to two batches (A[s] against B[s]), every pair held to its row; `sink` takes each finished batch while its elements are on
// the device.  extra: W for windows.  drop_flags: PBA_CIG_* taken out of every job's flags.  (bound is called twice a row, a
// million times for a set of 100 k reads: a template parameter, so that it inlines.)
template <class T, class Bound>
static int rows_chunks(pba_ctx *ctx, const char *who, const pba_seqs *const A[2], const pba_seqs *const B[2], const std::vector<RowJob> &jobs,
                       double R, Bound bound, SlotsInto extra, uint32_t drop_flags,
                       pba_aln_counts *counts, pba_result *res, uint64_t max_slots, uint32_t *n_chunks,
                       const std::function<int(const SlotBatch &)> &sink, const AllelesInto *sites = nullptr, int gate = 0) {
    std::vector<pba_pair> pairs;
    std::vector<uint32_t> pflags;
    std::vector<size_t> at;
    std::vector<uint64_t> rel;
    std::vector<pba_result> out;
    std::vector<int32_t> have;
    std::vector<pba_aln_counts> cnt;
    for (size_t j0 = 0; j0 < jobs.size();) {
        size_t j1 = j0;
        uint64_t slots = 0;
        while (j1 < jobs.size()) {                      // greedy take: at least one row
            const uint64_t b = bound(jobs[j1].pr);
            if (j1 > j0 && slots + b > max_slots) break;
            slots += b; ++j1;
        }
        if (n_chunks) ++*n_chunks;
        for (int s = 0; s < 2; ++s) {
            pairs.clear(); pflags.clear(); at.clear(); rel.assign(1, 0);
            extra.run_max = 0;
            for (size_t j = j0; j < j1; ++j) {
                if (jobs[j].batch != s) continue;
                const uint64_t b = bound(jobs[j].pr);
                pairs.push_back(jobs[j].pr); pflags.push_back(jobs[j].flags & ~drop_flags); at.push_back(j);
                rel.push_back(rel.back() + b);
                extra.run_max = std::max(extra.run_max, b);
            }
            const size_t nb = pairs.size();
            if (!nb) continue;
            out.resize(nb); have.resize(nb); cnt.resize(nb);
            SlotBufs d;
            PBA_TRY(slots_run<T>(ctx, A[s], B[s], pairs.data(), nb, R, 0, 0, extra, pflags.data(), rel.data(), out.data(), have.data(),
                                 cnt.data(), d, sites, gate));
            for (size_t q = 0; q < nb; ++q) {           // held to the row: the same roles, the same lengths, the same R
                const RowJob &jb = jobs[at[q]];
                if (res) res[jb.row] = out[q];
                if (counts) counts[jb.row] = cnt[q];
                if (!jb.not_held && !walk_agrees(out[q], jb.cost, jb.matlen_a, jb.matlen_b)) {
                    snprintf(ctx->err, sizeof ctx->err,
                             "%s: row %llu re-runs to rc %d cost %d matlen %d/%d, the row says cost %d matlen %d/%d: not a row of these "
                             "sets under this R", who, (unsigned long long)jb.row, out[q].rc, out[q].cost, out[q].matlen_a,
                             out[q].matlen_b, jb.cost, jb.matlen_a, jb.matlen_b);
                    return PBA_E_INVALID;
                }
            }
            const SlotBatch sb{&d, nb, rel.data(), have.data(), at.data()};
            PBA_TRY(sink(sb));
        }
        j0 = j1;
    }
    return PBA_OK;
}

// the rows of the jobs, for rows_layout
static inline std::vector<uint64_t> job_rows(const std::vector<RowJob> &jobs) {
    std::vector<uint64_t> r(jobs.size());
    for (size_t j = 0; j < jobs.size(); ++j) r[j] = jobs[j].row;
    return r;
}

// ---- the sites object (made in pba_sites.hip; its alleles outlet is also driven from pba_phase.hip) ----------------------------
struct pba_sites {
    int device;
    uint32_t t_lo, t_hi, n_seqs;
    uint64_t n, n_sel, n_boxes, words;
    pba_site *d_recs;                   // n records, sorted by (target, pos, kind)
    unsigned long long *d_bm;           // SEL bitmap of the arena, words + 1 (the last: zero)
    uint32_t *d_rank;                   // inclusive scan of the words' SEL counts
    uint2 *d_sel;                       // per SEL site, in rank order: { record index, own | major << 4 | minor << 8 }
    unsigned long long *d_box_off;      // nt + 1
    // on the host, for the per-row slot bounds, the target ranges and the checks of caller-supplied allele records
    std::vector<uint64_t> box_off, rec_off, sel_off;    // nt + 1 each
    std::vector<int32_t> sel_pos;                       // the SEL positions, target by target
    std::vector<uint32_t> sel_rec;                      // the record index of every SEL site, in rank order
    AllelesInto view() const { return AllelesInto{d_bm, d_rank, d_sel, d_box_off, t_lo, n_boxes}; }
};

static const uint64_t kAlleleChunkSlots = 1ull << 27;   // bounded allele slots of one chunk of rows on the device (1 GiB)

// `set` is the set these sites were made from, as far as lengths can tell
static inline bool sites_same_set(const pba_sites *s, const pba_seqs *set) {
    if (set->n != s->n_seqs) return false;
    for (uint32_t k = 0; k < s->t_hi - s->t_lo; ++k)
        if (s->box_off[k + 1] - s->box_off[k] != set->h_len[s->t_lo + k]) return false;
    return true;
}

// The SEL sites in the a-span the accessor could cover at most: the clipped len_a elements from a_pos, by binary search in
// the host's positions.  0 is a legal bound: the row is still walked and held.
static inline uint64_t pair_alleles_bound(const pba_sites *s, const pba_pair &p, double R) {
    const int la = text_clip(p.a_len, p.b_len, R).len_a;
    if (la < 1) return 0;
    const int64_t last = (p.flags & PBA_A_BACKWARD) ? (int64_t)p.a_pos - (la - 1) : (int64_t)p.a_pos + (la - 1);
    const int64_t lo = std::min<int64_t>(p.a_pos, last), hi = std::max<int64_t>(p.a_pos, last);
    const size_t k = p.a_seq - s->t_lo;
    const int32_t *b = s->sel_pos.data() + s->sel_off[k], *e = s->sel_pos.data() + s->sel_off[k + 1];
    return (uint64_t)(std::upper_bound(b, e, (int32_t)std::min<int64_t>(hi, 0x7FFFFFFF)) - std::lower_bound(b, e, (int32_t)std::max<int64_t>(lo, 0)));
}

#endif
