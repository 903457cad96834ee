// pba_pileup.hip -- read correction from overlap pile-ups: the vote boxes of MANY references at once (every read of a
// target range is one, csrc/consensus.h has the single-reference form), the segmented vote and evolve, and the driver
// that chains overlap -> vote -> evolve over a read set.  Host side and kernels.
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
//
// Box arena: sel[], sup[] (4 x u16 in a u64 each, A in bits 15:0, as ConsDev) and tot[] over all bases of the range, the
// segment of target t at box_off[t - t_lo] (u64 on the device; the host keeps the arena below 2^31 boxes so that the vote
// kernel's box indices stay ints).  20 bytes per base.  No 3*max_len margins and no second ping-pong set: nothing grows,
// and evolve writes only text.  No text byte per box either: the box of base i is filled straight from the packed read,
// the votes never read the text, and the winner of an evolved box comes from its counters.
// Votes: k_vote_pairs<NB, true, SEG = true> (pba_align.hip) through trace_batch, strand +1 rows against `reads`, strand -1
// rows against `reads_rc`, both into the same arena.  Counters are u16 bumped with 32-bit atomics on their dword: a
// selection counter holds weight + votes <= 65 535 (beyond that it would carry into its neighbour, not wrap).
// Evolve: every box yields 0..2 characters -- winner(sel) if its selection holds a majority of tot, then winner(sup) if
// its suppliment does (ref_seq.h:327-336, the FP64 test of k_cons_evolve).  The reference also folds a deleted box's
// selection into the suppliment of the last box kept before it, which changes only the NEXT round's sup counters; only the
// text leaves a pile-up, so those counts are not materialised.  A count pass (one workgroup per target) gives the new
// lengths, the host scans them, and a write pass puts every target's text at its final offset of one contiguous text,
// which pba_seqs_from_device_text packs.
#include "pba_host.h"

#include <deque>
#include <memory>

// boxes of target t0 + blockIdx.x <- vote_box(base, weight) (ref_seq.h:118: selection(c, n), total(1)), from the packed read
static __global__ void __launch_bounds__(256)
k_pile_fill(SeqSetDev S, uint32_t k0, PileView P, int weight) {
    const uint32_t k = k0 + blockIdx.x, t = P.t_lo + k;
    const uint8_t *seq = S.packed + S.off[t];
    const uint32_t len = S.len[t];
    const unsigned long long first = P.box_off[k];
    for (uint32_t i = threadIdx.x; i < len; i += 256) {
        const int code = (seq[i >> 2] >> (6 - 2 * (i & 3))) & 3;            // 2-bit code == C2I of the base
        P.dev.sel[first + i] = (unsigned long long)(unsigned)(weight & 0xFFFF) << (16 * code);
        P.dev.sup[first + i] = 0ull;
        P.dev.tot[first + i] = 1;
    }
}

// what box i yields: bit 0 = its selection is kept (is_valid(0.5), ref_seq.h:336), bit 1 = its suppliment splits off
// (has_supply(0.5), ref_seq.h:327)
__device__ __forceinline__ int pile_yield(const PileView &P, unsigned long long i, unsigned long long &sel, unsigned long long &sup) {
    sel = P.dev.sel[i]; sup = P.dev.sup[i];
    const int tot = P.dev.tot[i];
    const bool S = (double)cons_max4(sup) > 0.5 * (double)tot;
    const bool V = (double)cons_max4(sel) > 0.5 * (double)tot;
    return (V ? 1 : 0) | (S ? 2 : 0);
}

// count pass: len_out[k] = characters target k evolves to
static __global__ void __launch_bounds__(256)
k_pile_count(PileView P, uint32_t k0, int *len_out) {
    __shared__ int part[4];
    const uint32_t k = k0 + blockIdx.x;
    const unsigned long long first = P.box_off[k], len = P.box_off[k + 1] - first;
    int mine = 0;
    for (unsigned long long i = threadIdx.x; i < len; i += 256) {
        unsigned long long sel, sup;
        const int y = pile_yield(P, first + i, sel, sup);
        mine += (y & 1) + (y >> 1);
    }
    const int w = wave_sum_i32(mine);                          // every lane is here: the loop has ended for all of them
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0) part[threadIdx.x / PBA_WAVE] = w;
    __syncthreads();
    if (threadIdx.x == 0) len_out[k] = part[0] + part[1] + part[2] + part[3];
}

// write pass: the text of target k at text[text_off[k] ..), 256 boxes per step.  A box yields at most two characters, so the
// offsets inside a step are two ballots and two popcounts per lane plus the totals of the wavefronts before it in LDS.
static __global__ void __launch_bounds__(256)
k_pile_write(PileView P, uint32_t k0, const unsigned long long *text_off, char *text) {
    __shared__ int part[4];
    const uint32_t k = k0 + blockIdx.x;
    const unsigned long long first = P.box_off[k], len = P.box_off[k + 1] - first;
    char *out = text + text_off[k];
    const int lane = threadIdx.x & (PBA_WAVE - 1), wave = threadIdx.x / PBA_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long done = 0;                               // characters written by the steps before this one
    for (unsigned long long base = 0; base < len; base += 256) {
        const unsigned long long i = base + threadIdx.x;
        unsigned long long sel = 0, sup = 0;
        const int y = i < len ? pile_yield(P, first + i, sel, sup) : 0;
        const unsigned long long mv = __builtin_amdgcn_ballot_w64((y & 1) != 0), ms = __builtin_amdgcn_ballot_w64((y & 2) != 0);
        if (lane == 0) part[wave] = __builtin_popcountll(mv) + __builtin_popcountll(ms);
        __syncthreads();
        int before = __builtin_popcountll(mv & below) + __builtin_popcountll(ms & below);
        for (int w = 0; w < wave; ++w) before += part[w];
        const int step = part[0] + part[1] + part[2] + part[3];
        unsigned long long at = done + (unsigned long long)before;
        if (y & 1) out[at++] = cons_winner(sel);
        if (y & 2) out[at] = cons_winner(sup);                 // the split box sits right behind (ref_seq.h:328-334)
        done += (unsigned long long)step;
        __syncthreads();                                       // part[] is rewritten by the next step
    }
}

extern "C" {

struct pba_pileup {
    int device;
    uint32_t t_lo, t_hi, n_reads;
    int weight;
    bool spent;
    uint64_t n_boxes;
    unsigned long long *d_sel, *d_sup, *d_box_off;
    int *d_tot;
    std::vector<uint64_t> box_off;      // nt + 1
    std::vector<int32_t> n_rows;        // rows voted per target
};

static PileView pile_view(const pba_pileup *p) {
    PileView v;
    v.dev = ConsDev{p->d_sel, p->d_sup, p->d_tot, nullptr};
    v.box_off = p->d_box_off; v.t_lo = p->t_lo;
    return v;
}

static void pile_free_boxes(pba_pileup *p) {
    if (p->d_sel) (void)hipFree(p->d_sel);
    if (p->d_sup) (void)hipFree(p->d_sup);
    if (p->d_tot) (void)hipFree(p->d_tot);
    if (p->d_box_off) (void)hipFree(p->d_box_off);
    p->d_sel = p->d_sup = p->d_box_off = nullptr; p->d_tot = nullptr;
}

// a launch's global size is a 32-bit number: one workgroup of 256 threads per target, at most 2^22 targets per launch
static const uint32_t kPileSlice = 1u << 22;
static const uint64_t kPileMaxBoxes = (1ull << 31) - 65536;

int pba_overlap_row_pair(const pba_strand_overlap *row, uint32_t target_len, uint32_t query_len, pba_pair *out) {
    if (!row || !out) return PBA_E_INVALID;
    if ((row->dir != 1 && row->dir != -1) || (row->strand != 1 && row->strand != -1)) return PBA_E_INVALID;
    if (row->target < 0 || row->query < 0 || row->j < 0 || row->ref_pos < 0) return PBA_E_INVALID;
    if (target_len > 0x7FFFFFFFu || query_len > 0x7FFFFFFFu) return PBA_E_INVALID;
    const int64_t tl = target_len, slen = query_len;
    if (row->j >= slen) return PBA_E_INVALID;                                  // b_len = slen - j >= 1
    const bool fwd = row->dir == 1;
    if (fwd ? row->ref_pos >= tl : (int64_t)row->ref_pos + 16 > tl) return PBA_E_INVALID;
    memset(out, 0, sizeof *out);
    out->a_seq = (uint32_t)row->target; out->b_seq = (uint32_t)row->query;
    out->a_pos = fwd ? row->ref_pos : row->ref_pos + 15;                       // spaced_seed.cpp:285
    out->a_len = fwd ? (int32_t)(tl - row->ref_pos) : row->ref_pos + 16;       // get_accessor, ref_seq.h:284-285
    out->b_pos = fwd ? row->j : (int32_t)(slen - row->j - 1);                  // spaced_seed.cpp:274-276
    out->b_len = (int32_t)(slen - row->j);
    out->flags = fwd ? 0u : (PBA_A_BACKWARD | PBA_B_BACKWARD);
    return PBA_OK;
}

int pba_pileup_create(pba_ctx *ctx, const pba_seqs *reads, uint32_t t_lo, uint32_t t_hi, int weight, pba_pileup **out) {
    if (!ctx || !reads || !out || t_lo > t_hi || t_hi > reads->n) return PBA_E_INVALID;
    *out = nullptr;
    if (weight < 1 || weight > 0xFFFF) PBA_FAIL(PBA_E_INVALID, "pba_pileup_create: weight must be in [1, 65535]");
    if (reads->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_pileup_create: the read set holds bytes outside ACGT");
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t nt = t_hi - t_lo;
    std::unique_ptr<pba_pileup> p(new (std::nothrow) pba_pileup());
    if (!p) PBA_FAIL(PBA_E_NOMEM, "pba_pileup");
    p->device = ctx->device; p->t_lo = t_lo; p->t_hi = t_hi; p->n_reads = reads->n; p->weight = weight; p->spent = false;
    p->d_sel = p->d_sup = p->d_box_off = nullptr; p->d_tot = nullptr;
    p->box_off.assign((size_t)nt + 1, 0);
    p->n_rows.assign(nt, 0);
    for (uint32_t k = 0; k < nt; ++k) p->box_off[k + 1] = p->box_off[k] + reads->h_len[t_lo + k];
    p->n_boxes = p->box_off[nt];
    if (p->n_boxes >= kPileMaxBoxes) PBA_FAIL(PBA_E_TOOLONG, "pba_pileup_create: 2^31 boxes or more in one pile-up: use a smaller target range");
    const size_t cap = (size_t)p->n_boxes + 64;
    const bool ok = hipMalloc((void **)&p->d_sel, cap * 8) == hipSuccess && hipMalloc((void **)&p->d_sup, cap * 8) == hipSuccess &&
                    hipMalloc((void **)&p->d_tot, cap * 4) == hipSuccess &&
                    hipMalloc((void **)&p->d_box_off, sizeof(uint64_t) * ((size_t)nt + 1)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); pile_free_boxes(p.get()); PBA_FAIL(PBA_E_NOMEM, "pba_pileup_create: vote boxes"); }
    hipError_t e = hipMemcpyAsync(p->d_box_off, p->box_off.data(), sizeof(uint64_t) * ((size_t)nt + 1), hipMemcpyHostToDevice, ctx->stream);
    const PileView P = pile_view(p.get());
    for (uint32_t k0 = 0; k0 < nt && e == hipSuccess; k0 += kPileSlice) {
        hipLaunchKernelGGL(k_pile_fill, dim3(std::min(kPileSlice, nt - k0)), dim3(256), 0, ctx->stream, reads->dev(), k0, P, weight);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { pile_free_boxes(p.get()); return ctx_fail(ctx, PBA_E_HIP, "pba_pileup_create", e); }
    *out = p.release();
    return PBA_OK;
}

void pba_pileup_destroy(pba_pileup *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    pile_free_boxes(p);                   // hipFree waits for the work that uses the buffers
    delete p;
}

// `reads` is the set these boxes were filled from, as far as lengths can tell
static bool pile_same_reads(const pba_pileup *p, const pba_seqs *reads) {
    if (reads->n != p->n_reads) return false;
    for (uint32_t k = 0; k < p->t_hi - p->t_lo; ++k)
        if (p->box_off[k + 1] - p->box_off[k] != reads->h_len[p->t_lo + k]) return false;
    return true;
}

int pba_pileup_vote(pba_ctx *ctx, pba_pileup *p, const pba_seqs *reads, const pba_seqs *reads_rc,
                    const pba_strand_overlap *rows, uint64_t n, double R, pba_result *res) {
    if (!ctx || !p || !reads || (!rows && n)) return PBA_E_INVALID;
    if (p->spent) PBA_FAIL(PBA_E_INVALID, "pba_pileup_vote: the pile-up is spent");
    if (!(R > 0.0) || !(R < 1.0)) PBA_FAIL(PBA_E_INVALID, "R must be in (0,1)");
    if (!pile_same_reads(p, reads)) PBA_FAIL(PBA_E_INVALID, "pba_pileup_vote: reads is not the set of this pile-up");
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        PBA_FAIL(PBA_E_INVALID, "pba_pileup_vote: reads_rc differs from reads in count or lengths");
    if (reads->non_acgt || (reads_rc && reads_rc->non_acgt)) PBA_FAIL(PBA_E_ALPHABET, "pba_pileup_vote: the read set holds bytes outside ACGT");
    if (n == 0) return PBA_OK;
    if (n > 0x7FFFFFFFull) PBA_FAIL(PBA_E_INVALID, "pba_pileup_vote: too many rows in one call");
    std::vector<pba_pair> pairs[2];       // strand +1 (B = reads), strand -1 (B = reads_rc)
    std::vector<uint32_t> which[2];
    for (uint64_t k = 0; k < n; ++k) {
        const pba_strand_overlap &r = rows[k];
        if (r.target < 0 || (uint32_t)r.target < p->t_lo || (uint32_t)r.target >= p->t_hi)
            PBA_FAIL(PBA_E_INVALID, "pba_pileup_vote: a row's target is outside the pile-up's range");
        if (r.query < 0 || (uint32_t)r.query >= reads->n) PBA_FAIL(PBA_E_INVALID, "pba_pileup_vote: a row's query is not a read of the set");
        if (r.strand == -1 && !reads_rc) PBA_FAIL(PBA_E_INVALID, "pba_pileup_vote: a strand -1 row needs reads_rc");
        pba_pair pr;
        if (pba_overlap_row_pair(&r, reads->h_len[r.target], reads->h_len[r.query], &pr) != PBA_OK)
            PBA_FAIL(PBA_E_INVALID, "pba_pileup_vote: a row's accessors lie outside its reads");
        const int s = r.strand == 1 ? 0 : 1;
        pairs[s].push_back(pr); which[s].push_back((uint32_t)k);
    }
    HIPCHK(hipSetDevice(ctx->device));
    const PileView view = pile_view(p);
    std::vector<pba_result> out;
    bool voted = false;                   // a batch of this call has gone through
    for (int s = 0; s < 2; ++s) {
        if (pairs[s].empty()) continue;
        out.resize(pairs[s].size());
        // (the rows passed their OVERLAP_MIN gate when they were found: the walk votes whatever re-runs to success)
        const int st = trace_batch(ctx, reads, s ? reads_rc : reads, pairs[s].data(), pairs[s].size(), R, 0, 0, PBA_KERNEL_BITVEC,
                                   out.data(), nullptr, nullptr, nullptr, nullptr, 0, &view);
        if (st != PBA_OK) {
            // PBA_E_TOOLONG / PBA_E_INVALID come from the plan and the pair checks, before any launch.  Anything else may have
            // left votes behind, and so has an earlier batch of this call: the boxes no longer say which rows they hold.
            if (voted || (st != PBA_E_TOOLONG && st != PBA_E_INVALID)) p->spent = true;
            return st;
        }
        voted = true;
        for (size_t q = 0; q < out.size(); ++q) {
            const pba_strand_overlap &r = rows[which[s][q]];
            if (res) res[which[s][q]] = out[q];
            if (out[q].rc < 0 || out[q].cost != r.cost || out[q].matlen_a != r.matlen_a || out[q].matlen_b != r.matlen_b) {
                p->spent = true;
                snprintf(ctx->err, sizeof ctx->err,
                         "pba_pileup_vote: row %llu (target %d, query %d, strand %d) re-runs to rc %d cost %d matlen %d/%d, the row says cost %d "
                         "matlen %d/%d: not an overlap of these sets under this R (the pile-up is spent)",
                         (unsigned long long)which[s][q], r.target, r.query, r.strand, out[q].rc, out[q].cost, out[q].matlen_a, out[q].matlen_b,
                         r.cost, r.matlen_a, r.matlen_b);
                return PBA_E_INVALID;
            }
        }
        for (size_t q = 0; q < out.size(); ++q) ++p->n_rows[(uint32_t)rows[which[s][q]].target - p->t_lo];
    }
    return PBA_OK;
}

int pba_pileup_dump(pba_ctx *ctx, const pba_pileup *p, uint32_t target, uint16_t *sel, uint16_t *sup, int32_t *tot, int cap,
                    int32_t *n) {
    if (!ctx || !p || !n || cap < 0 || (cap && (!sel || !sup || !tot)) || target < p->t_lo || target >= p->t_hi) return PBA_E_INVALID;
    if (p->spent) PBA_FAIL(PBA_E_INVALID, "pba_pileup_dump: the pile-up is spent");
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t first = p->box_off[target - p->t_lo];
    *n = (int32_t)(p->box_off[target - p->t_lo + 1] - first);
    const int k = std::min(*n, cap);
    if (k > 0) {
        HIPCHK(hipMemcpyAsync(sel, p->d_sel + first, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(sup, p->d_sup + first, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(tot, p->d_tot + first, (size_t)k * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return PBA_OK;
}

// evolve to one contiguous device text: target k at text[text_off[k] .. text_off[k+1]); the boxes are released
// (d_toff: text_off on the device, nt + 1 u64)
static int pile_evolve_text(pba_ctx *ctx, pba_pileup *p, DevBuf *text, DevBuf *d_toff, std::vector<uint64_t> *text_off,
                            pba_correct_row *rows_out) {
    if (p->spent) PBA_FAIL(PBA_E_INVALID, "pba_pileup_evolve: the pile-up is spent");
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t nt = p->t_hi - p->t_lo;
    const PileView P = pile_view(p);
    DevBuf d_len;
    std::vector<int32_t> len_out(nt, 0);
    HIPCHK(hipMalloc(&d_len.p, sizeof(int32_t) * ((size_t)nt + 1)));
    for (uint32_t k0 = 0; k0 < nt; k0 += kPileSlice)
        hipLaunchKernelGGL(k_pile_count, dim3(std::min(kPileSlice, nt - k0)), dim3(256), 0, ctx->stream, P, k0, d_len.as<int>());
    HIPCHK(hipGetLastError());
    if (nt) HIPCHK(hipMemcpyAsync(len_out.data(), d_len.p, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    text_off->assign((size_t)nt + 1, 0);
    for (uint32_t k = 0; k < nt; ++k) (*text_off)[k + 1] = (*text_off)[k] + (uint64_t)len_out[k];
    const uint64_t total = (*text_off)[nt];
    HIPCHK(hipMalloc(&text->p, total + kSlack));
    d_toff->reset();
    HIPCHK(hipMalloc(&d_toff->p, sizeof(uint64_t) * ((size_t)nt + 1)));
    HIPCHK(hipMemcpyAsync(d_toff->p, text_off->data(), sizeof(uint64_t) * ((size_t)nt + 1), hipMemcpyHostToDevice, ctx->stream));
    for (uint32_t k0 = 0; k0 < nt; k0 += kPileSlice)
        hipLaunchKernelGGL(k_pile_write, dim3(std::min(kPileSlice, nt - k0)), dim3(256), 0, ctx->stream, P, k0,
                           d_toff->as<unsigned long long>(), text->as<char>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (uint32_t k = 0; rows_out && k < nt; ++k) {
        rows_out[k].target = (int32_t)(p->t_lo + k); rows_out[k].n_rows = p->n_rows[k];
        rows_out[k].len_in = (int32_t)(p->box_off[k + 1] - p->box_off[k]); rows_out[k].len_out = len_out[k];
    }
    p->spent = true;
    pile_free_boxes(p);
    return PBA_OK;
}

int pba_pileup_evolve(pba_ctx *ctx, pba_pileup *p, pba_seqs **corrected, pba_correct_row *rows_out) {
    if (!ctx || !p || !corrected) return PBA_E_INVALID;
    *corrected = nullptr;
    DevBuf text, d_toff;
    std::vector<uint64_t> text_off;
    const int st = pile_evolve_text(ctx, p, &text, &d_toff, &text_off, rows_out);
    if (st != PBA_OK) return st;
    return pba_seqs_from_device_text(ctx, text.p, d_toff.p, p->t_hi - p->t_lo, text_off.back(), 0, corrected);
}

int pba_ctx_last_correct_profile(const pba_ctx *ctx, pba_correct_profile *out) {
    if (!ctx || !out) return PBA_E_INVALID;
    *out = ctx->cprof;
    return PBA_OK;
}

// a stage of pba_correct_reads between two events on the ctx's stream (every stage ends synchronised)
struct StageClock {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~StageClock() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    bool init() { return hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess; }
    void begin(hipStream_t s) { (void)hipEventRecord(e0, s); }
    void end(hipStream_t s, float *acc) {
        float ms = 0.f;
        (void)hipEventRecord(e1, s);
        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *acc += ms;
    }
};

static void stats_add(pba_overlap_stats &a, const pba_overlap_stats &b, bool first) {
    if (first) { a = b; return; }
    a.n_candidates += b.n_candidates; a.n_pairs += b.n_pairs; a.n_overlaps += b.n_overlaps; a.n_redo += b.n_redo;
    a.scan_ms += b.scan_ms; a.sort_ms += b.sort_ms; a.walk_ms += b.walk_ms; a.n_big_targets += b.n_big_targets;
    a.n_prefiltered += b.n_prefiltered; a.cap_fill += b.cap_fill; a.cap_overflow += b.cap_overflow; a.n_listed += b.n_listed;
    a.wide_first = std::max(a.wide_first, b.wide_first);
}

int pba_correct_reads(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                      uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                      pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2]) {
    return pba_correct_reads_budget(ctx, reads, reads_rc, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, strands, weight, 0,
                                    corrected, rows_out, stats);
}

int pba_correct_reads_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                             uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                             uint64_t max_boxes, pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2]) {
    if (!ctx || !reads || !corrected || t_lo > t_hi || t_hi > reads->n) return PBA_E_INVALID;
    *corrected = nullptr;
    if (weight < 1 || weight > 0xFFFF) PBA_FAIL(PBA_E_INVALID, "pba_correct_reads: weight must be in [1, 65535]");
    if (strands < 1 || strands > 3) PBA_FAIL(PBA_E_INVALID, "pba_correct_reads: strands must be 1 (+1), 2 (-1) or 3 (both)");
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        PBA_FAIL(PBA_E_INVALID, "pba_correct_reads: reads_rc differs from reads in count or lengths");
    if (reads->non_acgt || (reads_rc && reads_rc->non_acgt)) PBA_FAIL(PBA_E_ALPHABET, "pba_correct_reads: the read set holds bytes outside ACGT");
    if (max_trial < 1 || max_trial > 63) PBA_FAIL(PBA_E_INVALID, "max_trial must be in [1, 63]");
    HIPCHK(hipSetDevice(ctx->device));
    struct Own {
        pba_seqs *rc = nullptr;
        pba_probe_table *tab[2] = {nullptr, nullptr};
        pba_pileup *pile = nullptr;
        ~Own() { pba_pileup_destroy(pile); pba_probe_table_destroy(tab[0]); pba_probe_table_destroy(tab[1]); if (rc) pba_seqs_destroy(rc); }
    } own;
    StageClock clk;
    if (!clk.init()) PBA_FAIL(PBA_E_HIP, "pba_correct_reads: events");
    pba_correct_profile prof;
    memset(&prof, 0, sizeof prof);
    pba_overlap_stats tot[2];
    memset(tot, 0, sizeof tot);
    int st = PBA_OK;
    // the reverse complement and the probe tables once, every chunk of targets against them
    clk.begin(ctx->stream);
    if ((strands & 2) && !reads_rc) {
        st = pba_seqs_revcomp(ctx, reads, nullptr, &own.rc);
        if (st != PBA_OK) return st;
        reads_rc = own.rc;
    }
    const pba_seqs *sets[2] = {reads, reads_rc};
    for (int s = 0; s < 2; ++s) {
        if (!(strands & (1 << s))) continue;
        const uint64_t pcap = (uint64_t)reads->n * 2u * (uint32_t)max_trial;
        DevBuf d_pent;
        HIPCHK(hipMalloc(&d_pent.p, sizeof(uint64_t) * (pcap + 1)));
        uint64_t n_pent = 0;
        st = pba_overlap_probes(ctx, sets[s], 0, reads->n, mask, max_trial, d_pent.p, pcap, &n_pent);
        if (st == PBA_OK) st = pba_probe_table_create(ctx, d_pent.p, n_pent, mask, max_trial, &own.tab[s]);
        if (st != PBA_OK) return st;
    }
    clk.end(ctx->stream, &prof.overlap_ms);
    std::deque<DevBuf> texts;                        // one per chunk
    DevBuf d_toff;                                   // the offsets of the last chunk's text, on the device
    std::vector<uint64_t> all_off(1, 0), chunk_bytes;
    std::vector<pba_strand_overlap> rows;
    uint32_t lo = t_lo, shrink = 0;                  // shrink: the chunk's box budget is halved this many times
    bool first = true;
    while (lo < t_hi) {
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        uint64_t budget = std::min<uint64_t>(kPileMaxBoxes - 1, (uint64_t)(free_b / 4) / 20);
        if (max_boxes) budget = std::min(budget, max_boxes);
        budget = std::max<uint64_t>(1, budget >> shrink);
        uint32_t hi = lo;
        uint64_t boxes = 0;
        while (hi < t_hi && (hi == lo || boxes + reads->h_len[hi] <= budget)) boxes += reads->h_len[hi++];
        // overlaps of the chunk; the row buffer grows to what the call reports
        clk.begin(ctx->stream);
        uint64_t n_rows = 0;
        pba_overlap_stats cst[2];
        memset(cst, 0, sizeof cst);
        if (rows.size() < (size_t)(hi - lo) * 16 + 1024) rows.resize((size_t)(hi - lo) * 16 + 1024);
        for (;;) {
            st = pba_overlap_strands_table(ctx, reads, (strands & 2) ? reads_rc : nullptr, lo, hi, own.tab[0], own.tab[1], R, overlap_min,
                                           kernel, rows.data(), rows.size(), &n_rows, cst);
            if (st != PBA_OK || n_rows <= rows.size()) break;
            rows.resize(n_rows + n_rows / 8);
        }
        clk.end(ctx->stream, &prof.overlap_ms);
        if ((st == PBA_E_TOOLONG || st == PBA_E_NOMEM) && hi - lo > 1) { ++shrink; continue; }     // too many candidates for one call
        if (st != PBA_OK) return st;
        stats_add(tot[0], cst[0], first); stats_add(tot[1], cst[1], first);
        first = false;
        clk.begin(ctx->stream);
        st = pba_pileup_create(ctx, reads, lo, hi, weight, &own.pile);
        if (st == PBA_OK) st = pba_pileup_vote(ctx, own.pile, reads, reads_rc, rows.data(), n_rows, R, nullptr);
        clk.end(ctx->stream, &prof.vote_ms);
        if (st == PBA_E_INVALID && own.pile && own.pile->spent) {    // the engine's own rows did not re-run to themselves
            char keep[sizeof ctx->err];
            memcpy(keep, ctx->err, sizeof keep);
            snprintf(ctx->err, sizeof ctx->err, "pba_correct_reads: %.400s", keep);
            return PBA_E_HIP;
        }
        if (st != PBA_OK) return st;
        clk.begin(ctx->stream);
        texts.emplace_back();
        std::vector<uint64_t> off;
        st = pile_evolve_text(ctx, own.pile, &texts.back(), &d_toff, &off, rows_out ? rows_out + (lo - t_lo) : nullptr);
        clk.end(ctx->stream, &prof.evolve_ms);
        if (st != PBA_OK) return st;
        pba_pileup_destroy(own.pile); own.pile = nullptr;
        const uint64_t base = all_off.back();
        chunk_bytes.push_back(off.back());
        for (size_t k = 1; k < off.size(); ++k) all_off.push_back(base + off[k]);
        prof.n_rows += n_rows; prof.n_bases_in += boxes; ++prof.n_chunks;
        lo = hi;
    }
    clk.begin(ctx->stream);
    const uint32_t nt = t_hi - t_lo;
    if (texts.size() == 1) st = pba_seqs_from_device_text(ctx, texts[0].p, d_toff.p, nt, all_off.back(), 0, corrected);
    else {
        // the chunks' texts side by side in one buffer (none: an empty range), then packed as one set
        DevBuf all;
        HIPCHK(hipMalloc(&all.p, all_off.back() + kSlack));
        uint64_t at = 0;
        for (size_t c = 0; c < texts.size(); ++c) {
            if (chunk_bytes[c]) HIPCHK(copy_d2d((uint8_t *)all.p + at, texts[c].p, chunk_bytes[c], ctx->stream));
            at += chunk_bytes[c];
        }
        d_toff.reset();
        HIPCHK(hipMalloc(&d_toff.p, sizeof(uint64_t) * all_off.size()));
        HIPCHK(hipMemcpyAsync(d_toff.p, all_off.data(), sizeof(uint64_t) * all_off.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        texts.clear();
        st = pba_seqs_from_device_text(ctx, all.p, d_toff.p, nt, all_off.back(), 0, corrected);
    }
    clk.end(ctx->stream, &prof.evolve_ms);
    if (st != PBA_OK) return st;
    prof.n_bases_out = all_off.back();
    ctx->cprof = prof;
    if (stats) { stats[0] = tot[0]; stats[1] = tot[1]; }
    return PBA_OK;
}

}  // extern "C"
