// pba_align.hip -- alignment of explicit pairs (seq_aligner<>::align) and edit scripts: kernels and C ABI.
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
#include "pba_host.h"
#include "align_bvtrace.h"
#include "align_cigar.h"
#include "align_windows.h"

// ids (nullable): the subset of pairs / reads to process (second, full-band launch)
template <int NB>
__global__ void __launch_bounds__(PBA_WAVE * Wpb<NB>::v, Wpb<NB>::occ)
k_align_pairs(SeqSetDev A, SeqSetDev B, const pba_pair *pairs, const uint32_t *ids, uint32_t n, AlignCfg cfg,
              pba_result *out, uint32_t *queue) {
    extern __shared__ __align__(16) uint8_t lds_all[];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / PBA_WAVE));   // wave-uniform on purpose: keeps the walk in SGPRs
    uint8_t *lds = lds_all + (size_t)wave * cfg.row_cap * 2;
    for (;;) {                                // persistent wavefront: pull the next pair until the queue is dry
        const uint32_t slot = next_slot(queue);
        if (slot >= n) break;
        const uint32_t q = ids ? ids[slot] : slot;
        const pba_pair pr = pairs[q];
        const PackedFetch fa = fetch_of(A, pr.a_seq, pr.a_pos, (pr.flags & PBA_A_BACKWARD) ? -1 : 1);
        const PackedFetch fb = fetch_of(B, pr.b_seq, pr.b_pos, (pr.flags & PBA_B_BACKWARD) ? -1 : 1);
        AlnOut o;
        align_dispatch<NB>(fa, pr.a_len, fb, pr.b_len, cfg, lds, o, true);
        store_result(out + q, o);
    }
}

__global__ void __launch_bounds__(PBA_WAVE)
k_align_bytes(const uint8_t *a, int a_dir, int la, const uint8_t *b, int b_dir, int lb, AlignCfg cfg,
              pba_result *out) {
    extern __shared__ __align__(16) uint8_t lds[];
    ByteFetch fa{a, a_dir}, fb{b, b_dir};
    AlnOut o;
    align_rowsweep(fa, la, fb, lb, cfg.R, cfg.maxn, cfg.maxm, (uint16_t *)lds, cfg.row_cap, o);
    store_result(out, o);
}

// ---- traceback: full-band row sweep that also stores one parent code per band cell, then a backward walk
__global__ void __launch_bounds__(PBA_WAVE)
k_align_pairs_trace(SeqSetDev A, SeqSetDev B, const pba_pair *pairs, uint32_t n, AlignCfg cfg, pba_result *out,
                    uint8_t *par, const uint64_t *par_off) {
    extern __shared__ __align__(16) uint8_t lds[];
    const uint32_t q = blockIdx.x;
    if (q >= n) return;
    const pba_pair pr = pairs[q];
    const PackedFetch fa = fetch_of(A, pr.a_seq, pr.a_pos, (pr.flags & PBA_A_BACKWARD) ? -1 : 1);
    const PackedFetch fb = fetch_of(B, pr.b_seq, pr.b_pos, (pr.flags & PBA_B_BACKWARD) ? -1 : 1);
    AlnOut o;
    align_rowsweep(fa, pr.a_len, fb, pr.b_len, cfg.R, cfg.maxn, cfg.maxm, (uint16_t *)lds, cfg.row_cap, o, par + par_off[q]);
    store_result(out + q, o);
}

__global__ void __launch_bounds__(PBA_WAVE)
k_align_bytes_trace(const uint8_t *a, int a_dir, int la, const uint8_t *b, int b_dir, int lb, AlignCfg cfg,
                    pba_result *out, uint8_t *par, uint16_t *cst) {
    extern __shared__ __align__(16) uint8_t lds[];
    ByteFetch fa{a, a_dir}, fb{b, b_dir};
    AlnOut o;
    align_rowsweep(fa, la, fb, lb, cfg.R, cfg.maxn, cfg.maxm, (uint16_t *)lds, cfg.row_cap, o, par, cst);
    store_result(out, o);
}

// ---- traceback on the bit-vector array: the persistent loop of align_bvtrace.h (trace_pairs_loop) under each of its five
// jobs -- scripts (align_bvtrace.h: ScriptJob), votes (consensus.h: VoteJob), runs (align_cigar.h: CigarJob), per-window counts
// (align_windows.h: WindowJob), alleles at selection sites (align_alleles.h: AlleleJob).  A kernel is its job's name for the profiler and its launch bounds; the job is its argument.
// CK: the checkpoint form of the traced pass (align_bvtrace.h): scratch holds one checkpoint per 32 steps, the walk re-runs
// chunks into this wavefront's LDS tile; else every step's parent words are streamed to scratch.  Runs, windows and
// alleles: that form only.
#ifndef PBA_TR_OCC12
#define PBA_TR_OCC12 6        // waves per SIMD of the checkpoint-form trace kernels at one or two blocks per lane (tuning hook;
                              // 32 768 reads of BASELINE configs[1], same box: 4 -> 63.0 ms, 5 -> 60.0, 6 -> 50.7, 8 -> 52.3)
#endif
#define PBA_TRACED_ARGS SeqSetDev A, SeqSetDev B, const pba_pair *pairs, const uint32_t *ids, uint32_t n, AlignCfg cfg, pba_result *out, \
                        uint32_t *scratch, uint64_t wave_words, uint64_t cap_words
template <int NB, bool CK>
__global__ void __launch_bounds__(PBA_WAVE * 4, NB <= 4 ? (CK && NB <= 2 ? PBA_TR_OCC12 : 4) : 2)
k_trace_pairs(PBA_TRACED_ARGS, ScriptJob job, uint32_t *queue) {
    trace_pairs_loop<NB, CK>(A, B, pairs, ids, n, cfg, out, scratch, wave_words, cap_words, job, queue);
}
// ref_seq::try_align's align + OVERLAP_MIN gate + elect (ref_seq.h:264-267) for a batch, no script in memory
template <int NB, bool CK, bool SEG = false>
__global__ void __launch_bounds__(PBA_WAVE * 4, NB <= 4 ? (CK && NB <= 2 ? PBA_TR_OCC12 : 4) : 2)
k_vote_pairs(PBA_TRACED_ARGS, VoteJob<SEG> job, uint32_t *queue) {
    trace_pairs_loop<NB, CK>(A, B, pairs, ids, n, cfg, out, scratch, wave_words, cap_words, job, queue);
}
template <int NB>
__global__ void __launch_bounds__(PBA_WAVE * 4, NB <= 4 ? (NB <= 2 ? PBA_TR_OCC12 : 4) : 2)
k_cigar_pairs(PBA_TRACED_ARGS, CigarJob job, uint32_t *queue) {
    trace_pairs_loop<NB, true>(A, B, pairs, ids, n, cfg, out, scratch, wave_words, cap_words, job, queue);
}
template <int NB>
__global__ void __launch_bounds__(PBA_WAVE * 4, NB <= 4 ? (NB <= 2 ? PBA_TR_OCC12 : 4) : 2)
k_window_pairs(PBA_TRACED_ARGS, WindowJob job, uint32_t *queue) {
    trace_pairs_loop<NB, true>(A, B, pairs, ids, n, cfg, out, scratch, wave_words, cap_words, job, queue);
}
template <int NB>
__global__ void __launch_bounds__(PBA_WAVE * 4, NB <= 4 ? (NB <= 2 ? PBA_TR_OCC12 : 4) : 2)
k_allele_pairs(PBA_TRACED_ARGS, AlleleJob job, uint32_t *queue) {
    trace_pairs_loop<NB, true>(A, B, pairs, ids, n, cfg, out, scratch, wave_words, cap_words, job, queue);
}
#undef PBA_TRACED_ARGS

// find_path (seq_aligner.h:214-233) walked iteratively from the goal cell; one thread per pair.  The walk meets the ops
// goal-first and the caller gets them origin-first, the first min(nedit, cap) of them (pba.h): so the path is walked twice,
// once for its length K and once to put the op met k-th at o[K - 1 - k] where that is inside the cap.
__device__ __forceinline__ int trace_walk_step(const uint8_t *p, int W, int md, int &i, int &j) {
    int src;
    if (j == 0) src = 3;                       // init_cell: (i,0) has parent DELETE, (0,j) INSERT (seq_aligner.h:140-147)
    else if (i == 0) src = 2;
    else src = p[(size_t)i * W + (j - i + md)];
    if (src == 1) { --i; --j; } else if (src == 2) --j; else --i;
    return src;
}
__global__ void k_trace_walk(const pba_result *res, const uint8_t *par, const uint64_t *par_off, uint8_t *ops,
                             const uint64_t *ops_off, int32_t *nedit, uint32_t n) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const pba_result r = res[q];
    if (r.rc < 0) { nedit[q] = 0; return; }
    const uint8_t *p = par + par_off[q];
    uint8_t *o = ops + ops_off[q];
    const uint64_t capq = ops_off[q + 1] - ops_off[q];
    const int md = r.max_dst, W = 2 * md + 1;
    int i = r.matlen_a, j = r.matlen_b;
    uint64_t k = 0;
    if ((uint64_t)i + (uint64_t)j <= capq) {   // room for any path (a batch always: check_pairs): one walk, reversed in place
        while (i > 0 || j > 0) o[k++] = (uint8_t)trace_walk_step(p, W, md, i, j);
        for (uint64_t x = 0, y = k; x + 1 < y; ++x) { --y; const uint8_t t = o[x]; o[x] = o[y]; o[y] = t; }   // goal-first -> origin-first
    } else {
        while (i > 0 || j > 0) { trace_walk_step(p, W, md, i, j); ++k; }
        i = r.matlen_a; j = r.matlen_b;
        for (uint64_t x = k; x-- > 0;) {
            const int src = trace_walk_step(p, W, md, i, j);
            if (x < capq) o[x] = (uint8_t)src;
        }
    }
    nedit[q] = (int32_t)k;
}

// (the attribute belongs to the current device: remembered per ctx, so a second ctx on another GPU sets it there too)
static void tu_attrs(pba_ctx *ctx) {
    if (ctx->attr_done & 1u) return;
    ctx->attr_done |= 1u;
    PBA_BIG_LDS(k_align_pairs<0>);
    PBA_BIG_LDS(k_align_bytes);
    PBA_BIG_LDS(k_align_bytes_trace);
    PBA_BIG_LDS(k_align_pairs_trace);
}

// the test and tuning hooks of a call, from the environment (read per call: the tests set and unset them between calls)
struct TraceHooks {
    bool stream;                 // PBA_TRACE_STREAM=1: every step's parent words streamed to HBM (the round-1 form, kept for
                                 // comparison) instead of checkpoints + recomputation
    bool budget_set; uint64_t budget;   // PBA_TRACE_BUDGET_GB: tuning aid, HBM the parent bits / codes of one call may take
    bool text_rowsweep;          // PBA_TEXT_ROWSWEEP=1: test hook, every text pair through the general form (both forms are cross-checked)
};
static TraceHooks trace_hooks_from_env() {
    TraceHooks h{false, false, 0, false};
    const char *e;
    if ((e = getenv("PBA_TRACE_STREAM"))) h.stream = atoi(e) != 0;
    if ((e = getenv("PBA_TRACE_BUDGET_GB"))) { h.budget_set = true; h.budget = (uint64_t)atoll(e) << 30; }
    if ((e = getenv("PBA_TEXT_ROWSWEEP"))) h.text_rowsweep = atoi(e) != 0;
    return h;
}

// Every pair inside its sequences and the engine limit (ops_off, nullable: a_len + b_len slots for each pair's script);
// the widest band and the longest script of the batch.
static int check_pairs(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R,
                       const uint64_t *ops_off, int *mdmax, uint64_t *ops_max) {
    *mdmax = 1; *ops_max = 0;
    for (size_t q = 0; q < n; ++q) {
        const pba_pair &p = pairs[q];
        if (!pair_ok(A, p.a_seq, p.a_pos, p.a_len, p.flags & PBA_A_BACKWARD) ||
            !pair_ok(B, p.b_seq, p.b_pos, p.b_len, p.flags & PBA_B_BACKWARD))
            PBA_FAIL(PBA_E_INVALID, "pair outside its sequence (or longer than the engine limit)");
        if (ops_off && (ops_off[q + 1] < ops_off[q] || ops_off[q + 1] - ops_off[q] < (uint64_t)p.a_len + p.b_len))
            PBA_FAIL(PBA_E_INVALID, "ops_off must leave a_len + b_len slots per pair");
        if (R > 0.0 && R < 1.0) *mdmax = std::max(*mdmax, max_dst_of(p.a_len, p.b_len, R));
        *ops_max = std::max(*ops_max, (uint64_t)p.a_len + p.b_len);
    }
    return PBA_OK;
}

// the results of a batch to the caller's array, synchronised; redo (nullable): the pairs whose narrow pass could not certify
// the goal row, which go round again at the reference band
static int fetch_results(pba_ctx *ctx, const void *d_out, pba_result *out, size_t n, std::vector<uint32_t> *redo) {
    HIPCHK(hipMemcpyAsync(out, d_out, sizeof(pba_result) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (size_t q = 0; redo && q < n; ++q)
        if (out[q].rc == PBA_RC_UNCERTIFIED) redo->push_back((uint32_t)q);
    return PBA_OK;
}

// one launch of k_align_pairs over `cnt` pairs (ids: device, nullable)
static void launch_align_pairs(pba_ctx *ctx, const Plan &pl, int nb, const SeqSetDev &A, const SeqSetDev &B, const pba_pair *d_pairs,
                               const uint32_t *ids, uint32_t cnt, pba_result *d_out) {
#define PBA_PAIRS_LAUNCH(NBV)                                                                                        \
    hipLaunchKernelGGL(k_align_pairs<NBV>, dim3(persistent_grid(ctx, cnt, Wpb<NBV>::v, ll.lds)),                      \
                       dim3(PBA_WAVE * Wpb<NBV>::v), ll.lds * Wpb<NBV>::v, ctx->stream, A, B, d_pairs, ids, cnt, ll.cfg, \
                       d_out, ctx->d_queue)
    const LaunchLds ll = launch_lds(pl, nb);
    PBA_DISPATCH_NB(nb, PBA_PAIRS_LAUNCH);
#undef PBA_PAIRS_LAUNCH
}

// ---- the traced bit-vector pass on the host: sizing and launch, shared by the batch and the one-pair text entry points
static const uint64_t kTraceBudget = 96ull << 30;      // parent codes / bits resident for one call (and at most 80 % of free HBM)

// scratch the traced bit-vector pass of one pair needs (u32 words): narrow first pass or reference band
static uint64_t trace_words_of(int la, int lb, double R, int nb, bool full_band, bool ck) {
    const TextClip c = text_clip(la, lb, R);
    const int m = std::min(c.len_a, c.len_b), n = std::max(c.len_a, c.len_b);
    if (m <= 10) return (band_matrix_cells(c) + 3) / 4;                          // the row sweep's corner: byte codes
    const int w = full_band ? c.md : bv_pass1_w(c.md, nb);
    return ck ? bv_ck_words(nb, m, n, w) : bv_trace_words(nb, m, n, w);
}

// One traced pass over `cnt` pairs (sub: their host indices, nullable = the first cnt), sized: the per-wavefront scratch
// area (cap_words of parent bits for the widest pair, then ops_max + 64 goal-first ops), as many workgroups as fill the chip
// and fit `budget`, and the ctx's scratch grown to hold them.
struct TracePass { uint64_t cap_words, wave_words; uint32_t grid; };
static int trace_pass_size(pba_ctx *ctx, const pba_pair *pairs, const uint32_t *sub, uint32_t cnt, double R, int nb, bool full_band,
                           bool ck, uint64_t ops_max, size_t lds, uint64_t budget, TracePass *tp) {
    uint64_t cap_words = 128;
    for (uint32_t k = 0; k < cnt; ++k) {
        const pba_pair &p = pairs[sub ? sub[k] : k];
        cap_words = std::max(cap_words, trace_words_of(p.a_len, p.b_len, R, nb, full_band, ck));
    }
    tp->cap_words = (cap_words + 63) & ~63ull;
    tp->wave_words = tp->cap_words + ((ops_max + 64 + 255) & ~255ull) / 4;
    tp->grid = (uint32_t)std::min<uint64_t>(persistent_grid(ctx, cnt, 4, lds), budget / (tp->wave_words * 4 * 4));
    if (tp->grid == 0) PBA_FAIL(PBA_E_NOMEM, "one wavefront's parent bits exceed the traceback budget");
    return scratch_reserve(ctx, (size_t)tp->grid * 4 * tp->wave_words * 4);
}

// What every launch of a traced kernel works on, whatever its job (all pointers: device).
struct TracedLaunch {
    SeqSetDev A, B;
    const pba_pair *pairs;
    pba_result *out;
    size_t lds;                           // per wavefront
    bool ck;                              // the checkpoint form
};
// (PBA_DISPATCH_NB without its case 0: these kernels have no row-sweep form)
#define PBA_DISPATCH_BV_NB(nb, K) \
    switch (nb) { case 1: K(1); break; case 2: K(2); break; case 3: K(3); break; case 4: K(4); break; case 6: K(6); break; default: K(8); break; }
// the kernel of a job at NB blocks per lane (ck: only where the job has both forms)
template <int NB> static auto traced_kernel(const ScriptJob &, bool ck) { return ck ? k_trace_pairs<NB, true> : k_trace_pairs<NB, false>; }
template <int NB> static auto traced_kernel(const VoteJob<false> &, bool ck) { return ck ? k_vote_pairs<NB, true, false> : k_vote_pairs<NB, false, false>; }
template <int NB> static auto traced_kernel(const VoteJob<true> &, bool) { return k_vote_pairs<NB, true, true>; }
template <int NB> static auto traced_kernel(const CigarJob &, bool) { return k_cigar_pairs<NB>; }
template <int NB> static auto traced_kernel(const WindowJob &, bool) { return k_window_pairs<NB>; }
template <int NB> static auto traced_kernel(const AlleleJob &, bool) { return k_allele_pairs<NB>; }
template <class Job>
static void launch_traced(pba_ctx *ctx, const TracedLaunch &t, const Job &job, int nb, const AlignCfg &cfg, const uint32_t *ids,
                          uint32_t cnt, const TracePass &tp) {
#define PBA_TRACED(NBV)                                                                                               \
    hipLaunchKernelGGL(traced_kernel<NBV>(job, t.ck), dim3(tp.grid), dim3(PBA_WAVE * 4), t.lds * 4, ctx->stream, t.A, t.B, t.pairs, \
                       ids, cnt, cfg, t.out, (uint32_t *)ctx->d_scratch, tp.wave_words, tp.cap_words, job, ctx->d_queue)
    PBA_DISPATCH_BV_NB(nb, PBA_TRACED);
#undef PBA_TRACED
}

// (the entry points below have C linkage from their declarations in pba.h / pba_host.h)
int pba_align_batch(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R,
                    int maxn, int maxm, int kernel, pba_result *out) {
    if (!ctx || !A || !B || (!pairs && n) || (!out && n)) return PBA_E_INVALID;
    if (n == 0) return PBA_OK;
    if (n > 0x7FFFFFFFull) PBA_FAIL(PBA_E_INVALID, "too many pairs in one batch");
    if (A->non_acgt || B->non_acgt)
        PBA_FAIL(PBA_E_ALPHABET, "a sequence set holds bytes outside ACGT: the reference compares raw bytes, use pba_align_text");
    HIPCHK(hipSetDevice(ctx->device));
    tu_attrs(ctx);
    int mdmax;
    uint64_t ops_max;
    int st = check_pairs(ctx, A, B, pairs, n, R, nullptr, &mdmax, &ops_max);
    if (st != PBA_OK) return st;
    Plan pl;
    st = make_plan(ctx, R, maxn, maxm, kernel, mdmax, &pl);
    if (st != PBA_OK) return st;
    DevBuf d_pairs, d_out;
    HIPCHK(hipMalloc(&d_pairs.p, sizeof(pba_pair) * n));
    HIPCHK(hipMalloc(&d_out.p, sizeof(pba_result) * n));
    HIPCHK(hipMemcpyAsync(d_pairs.p, pairs, sizeof(pba_pair) * n, hipMemcpyHostToDevice, ctx->stream));
    auto launch = [&](int nb, const uint32_t *ids, uint32_t cnt) {
        launch_align_pairs(ctx, pl, nb, A->dev(), B->dev(), d_pairs.as<pba_pair>(), ids, cnt, d_out.as<pba_result>());
    };
    auto collect = [&](std::vector<uint32_t> &redo) { return fetch_results(ctx, d_out.p, out, n, &redo); };
    auto finish = [&](bool redone) { return redone ? fetch_results(ctx, d_out.p, out, n, nullptr) : (int)PBA_OK; };
    return narrow_then_redo(ctx, pl, nullptr, (uint32_t)n, launch, collect, finish);
}

// ---------------------------------------------------------------------------------------------
// One pair handed over as host text: what the compat seq_aligner<>::align (include/compat/seq_aligner.h) calls.
// The clip of seq_aligner.h:94-102 comes first (text_clip, pba_host.h).
// ---------------------------------------------------------------------------------------------
// the reference's size guard (seq_aligner.h:104-107: LOG, return -1) answered on the host; 1 = *out is final, nothing to launch
static inline int text_guard(pba_ctx *ctx, const TextClip &c, int maxn, int maxm, pba_result *out, const char *who) {
    if (maxn > 0 && ((long long)c.len_a >= (long long)maxn + maxm || c.md >= maxm)) {
        out->rc = -1; out->cost = 0; out->matlen_a = 0; out->matlen_b = 0;
        out->len_a = c.len_a; out->len_b = c.len_b; out->max_dst = c.md; out->diag_cost = -1;
        return 1;
    }
    if (c.len_a > kMaxSeqLen || c.len_b > kMaxSeqLen) PBA_FAIL(PBA_E_TOOLONG, who);
    return 0;
}
// elements 0 .. len-1 of an accessor in text order: element k of a backward accessor is p[-k] (dna_seq.h:211,221), so its
// elements are the bytes [p-(len-1), p] and the accessor's origin is the last of them
static inline const uint8_t *acc_low(const char *p, int fwd, int len) { return (const uint8_t *)((fwd || len == 0) ? p : p - (len - 1)); }

// 2-bit codes (reference byte layout, dna_seq.h:147-159) and the two bit planes (dev_common.h: SeqSetDev::plane) of `len`
// text bytes; false at the first byte outside "ACGT" (the raw-byte row sweep takes the pair then: the reference compares bytes)
static bool pack_acgt(const uint8_t *src, int len, uint8_t *packed, uint32_t *plane) {
    static const struct Lut { uint8_t v[256]; Lut() { memset(v, 0xFF, sizeof v); v['A'] = 0; v['C'] = 1; v['G'] = 2; v['T'] = 3; } } lut;
    for (int w = 0; w * 32 < len; ++w) {
        const int nb = std::min(32, len - w * 32);
        uint32_t plo = 0, phi = 0, bad = 0;
        uint8_t *pk = packed + (size_t)w * 8;
        for (int k = 0; k < nb; ++k) {
            const uint32_t code = lut.v[src[w * 32 + k]];
            bad |= code;
            plo |= (code & 1u) << k;
            phi |= ((code >> 1) & 1u) << k;
            pk[k >> 2] |= (uint8_t)((code & 3u) << (6 - 2 * (k & 3)));
        }
        if (bad & 0x80u) return false;
        plane[2 * w] = plo; plane[2 * w + 1] = phi;
    }
    return true;
}

// A staged pair as a two-sequence set in one pooled device buffer (sequence 0 = a, sequence 1 = b, both stored in text
// order; a backward accessor starts at its last base with the BACKWARD flag): header, packed bases with kSlack zero bytes
// around them, bit planes with kPlaneSlack zero word pairs around them -- the text layout of seq_layout.h.
struct TextStage {
    size_t o_pair, o_off, o_len, o_poff, o_ooff, o_packed, o_plane, bytes;
    uint64_t pkA, pkB, wA, wB;
};
static inline TextStage text_stage_layout(const TextClip &c) {
    TextStage t;
    t.pkA = seq_packed_bytes((uint64_t)c.len_a); t.pkB = seq_packed_bytes((uint64_t)c.len_b);
    t.wA = seq_plane_words((uint64_t)c.len_a); t.wB = seq_plane_words((uint64_t)c.len_b);
    t.o_pair = 0; t.o_off = 32; t.o_len = 64; t.o_poff = 80; t.o_ooff = 128;
    t.o_packed = 256 + kSlack;
    t.o_plane = ((t.o_packed + t.pkA + t.pkB + kSlack + 63) & ~(size_t)63) + kPlaneSlack * 8;
    t.bytes = t.o_plane + (t.wA + t.wB) * 8 + kPlaneSlack * 8;
    return t;
}

// where the results of a staged pair land (POOL_TXT_OUT): the result, nedit, then the ops
static const size_t kTxtOutOps = 64;

// The fast form of the three text entry points: both accessors hold ACGT only, so comparing 2-bit codes is comparing bytes
// and the pair runs on the bit-vector array like a pair of a batch (narrow window first, the reference band if that cannot
// certify; with `ops` the traced pass, align_bvtrace.h, in its checkpoint form if ck).  One H2D copy, one or two launches on
// one wavefront, one D2H copy; every buffer is the ctx's.  Returns 1 when the pair is not ACGT-only (nothing was launched).
static int text_pair_bitvec(pba_ctx *ctx, const char *a, int a_fwd, const char *b, int b_fwd, const TextClip &c, double R,
                            int maxn, int maxm, pba_result *out, uint8_t *ops, int32_t ops_cap, int32_t *nedit, bool want_trace,
                            bool ck) {
    if (!bitvec_supports(c.md)) return 1;
    const TextStage t = text_stage_layout(c);
    const uint64_t ops_room = (uint64_t)c.len_a + c.len_b + 64;
    // the D2H copy reuses the staging buffer (the input image has been consumed by then: same stream)
    const size_t res_bytes = kTxtOutOps + (want_trace ? ops_room : 0);
    int st = stage_reserve(ctx, std::max(t.bytes, res_bytes));
    if (st != PBA_OK) return st;
    uint8_t *h = (uint8_t *)ctx->h_stage;
    memset(h, 0, t.bytes);
    if (!pack_acgt(acc_low(a, a_fwd, c.len_a), c.len_a, h + t.o_packed, (uint32_t *)(h + t.o_plane)) ||
        !pack_acgt(acc_low(b, b_fwd, c.len_b), c.len_b, h + t.o_packed + t.pkA, (uint32_t *)(h + t.o_plane) + 2 * t.wA))
        return 1;
    Plan pl;
    st = make_plan(ctx, R, maxn, maxm, PBA_KERNEL_AUTO, c.md, &pl);
    if (st != PBA_OK) return st;
    pba_pair pr;
    pr.a_seq = 0; pr.a_pos = a_fwd || !c.len_a ? 0 : c.len_a - 1; pr.a_len = c.len_a;
    pr.b_seq = 1; pr.b_pos = b_fwd || !c.len_b ? 0 : c.len_b - 1; pr.b_len = c.len_b;
    pr.flags = (a_fwd ? 0u : PBA_A_BACKWARD) | (b_fwd ? 0u : PBA_B_BACKWARD);
    memcpy(h + t.o_pair, &pr, sizeof pr);
    const uint64_t off[3] = {0, t.pkA, t.pkA + t.pkB}, poff[3] = {0, t.wA, t.wA + t.wB}, ooff[2] = {0, ops_room};
    const uint32_t len[3] = {(uint32_t)c.len_a, (uint32_t)c.len_b, 0};
    memcpy(h + t.o_off, off, sizeof off); memcpy(h + t.o_len, len, sizeof len);
    memcpy(h + t.o_poff, poff, sizeof poff); memcpy(h + t.o_ooff, ooff, sizeof ooff);
    uint8_t *d_in = nullptr, *d_res = nullptr;
    POOL(POOL_TXT_IN, t.bytes, d_in);
    POOL(POOL_TXT_OUT, kTxtOutOps + ops_room + 64, d_res);
    HIPCHK(hipMemcpyAsync(d_in, h, t.bytes, hipMemcpyHostToDevice, ctx->stream));
    const SeqSetDev S{d_in + t.o_packed, (const uint64_t *)(d_in + t.o_off), (const uint32_t *)(d_in + t.o_len),
                      (const uint32_t *)(d_in + t.o_plane), (const uint64_t *)(d_in + t.o_poff)};
    const TracedLaunch tl{S, S, (const pba_pair *)(d_in + t.o_pair), (pba_result *)d_res, pl.lds, ck};
    const ScriptJob job{d_res + kTxtOutOps, (const uint64_t *)(d_in + t.o_ooff), (int32_t *)(d_res + 32)};
    TracePass tp{};
    auto before = [&](int pass, const std::vector<uint32_t> &) {     // whichever of the workgroup's four wavefronts takes the pair
        return want_trace ? trace_pass_size(ctx, &pr, nullptr, 1, R, pass ? pl.nb2 : pl.nb1, pass != 0, ck, ops_room - 64, pl.lds,
                                            ~0ull, &tp) : (int)PBA_OK;
    };
    auto launch = [&](int nb, const uint32_t *ids, uint32_t cnt) {
        if (want_trace) launch_traced(ctx, tl, job, nb, pl.cfg, ids, cnt, tp);
        else launch_align_pairs(ctx, pl, nb, S, S, tl.pairs, ids, cnt, tl.out);
    };
    auto fetch = [&]() {
        HIPCHK(hipMemcpyAsync(ctx->h_stage, d_res, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        memcpy(out, ctx->h_stage, sizeof(pba_result));
        return (int)PBA_OK;
    };
    auto collect = [&](std::vector<uint32_t> &redo) {
        const int rc = fetch();
        if (rc == PBA_OK && out->rc == PBA_RC_UNCERTIFIED) redo.push_back(0);
        return rc;
    };
    auto finish = [&](bool redone) {
        if (!redone) return (int)PBA_OK;
        const int rc = fetch();
        if (rc == PBA_OK && out->rc == PBA_RC_UNCERTIFIED)
            PBA_FAIL(PBA_E_HIP, "reference-band pass left a pair uncertified");     // cannot happen (align_bitvec.h)
        return rc;
    };
    st = narrow_then_redo(ctx, pl, nullptr, 1, launch, collect, finish, before);
    if (st != PBA_OK) return st;
    if (out->rc == -2) PBA_FAIL(PBA_E_TOOLONG, "pair outside what the launch was sized for");   // host sizes both: cannot happen
    if (want_trace) {
        int32_t ne = 0;
        memcpy(&ne, (const uint8_t *)ctx->h_stage + 32, sizeof ne);
        *nedit = ne;
        const int32_t ncopy = std::min(ne, ops_cap);
        if (ncopy > 0) memcpy(ops, (const uint8_t *)ctx->h_stage + kTxtOutOps, (size_t)ncopy);
    }
    return PBA_OK;
}

// The general form: raw bytes (any alphabet, case-sensitive, seq_aligner.h:136) through the reference-shaped row sweep on one
// wavefront; par / cst as align_rowsweep takes them.  Only the clipped elements are shipped.
static int text_pair_stage_bytes(pba_ctx *ctx, const char *a, int a_fwd, const char *b, int b_fwd, const TextClip &c,
                                 const uint8_t **da, const uint8_t **db) {
    const size_t ob = ((size_t)c.len_a + 31) & ~(size_t)15, bytes = ob + c.len_b + 32;
    int st = stage_reserve(ctx, bytes);
    if (st != PBA_OK) return st;
    uint8_t *h = (uint8_t *)ctx->h_stage, *d_in = nullptr;
    if (c.len_a) memcpy(h, acc_low(a, a_fwd, c.len_a), c.len_a);
    if (c.len_b) memcpy(h + ob, acc_low(b, b_fwd, c.len_b), c.len_b);
    POOL(POOL_TXT_IN, bytes, d_in);
    HIPCHK(hipMemcpyAsync(d_in, h, bytes, hipMemcpyHostToDevice, ctx->stream));
    *da = d_in + (a_fwd || !c.len_a ? 0 : c.len_a - 1);
    *db = d_in + ob + (b_fwd || !c.len_b ? 0 : c.len_b - 1);
    return PBA_OK;
}

// What the three text entry points do before they launch: arguments and R, the clip, the size guard, the device, then the
// fast form unless PBA_TEXT_ROWSWEEP forces the general one, else the row sweep's plan and the staged bytes (t->pl, da, db).
// guarded(g) sees text_guard's answer first (g = 1: the guard hit) and fast() is the entry point's call of text_pair_bitvec.
// Returns 0: staged for the row sweep; 1: *out is final; < 0: failed.
struct TextCall { TextClip c; TraceHooks hooks; Plan pl; const uint8_t *da, *db; };
template <class Guarded, class Fast>
static int text_prologue(pba_ctx *ctx, const char *who, const char *a, int a_fwd, int la, const char *b, int b_fwd, int lb, double R,
                         int maxn, int maxm, pba_result *out, TextCall *t, Guarded guarded, Fast fast) {
    if (!ctx || !out || la < 0 || lb < 0 || (!a && la) || (!b && lb)) return PBA_E_INVALID;
    if (!(R > 0.0) || !(R < 1.0)) PBA_FAIL(PBA_E_INVALID, "R must be in (0,1)");
    t->c = text_clip(la, lb, R);
    int st = guarded(text_guard(ctx, t->c, maxn, maxm, out, who));
    if (st) return st;
    HIPCHK(hipSetDevice(ctx->device));
    tu_attrs(ctx);
    t->hooks = trace_hooks_from_env();
    if (!t->hooks.text_rowsweep && (st = fast()) != 1) return st == PBA_OK ? 1 : st;
    st = make_plan(ctx, R, maxn, maxm, PBA_KERNEL_ROWSWEEP, t->c.md, &t->pl);
    if (st != PBA_OK) return st;
    return text_pair_stage_bytes(ctx, a, a_fwd, b, b_fwd, t->c, &t->da, &t->db);
}

int pba_align_text(pba_ctx *ctx, const char *a, int a_fwd, int la, const char *b, int b_fwd, int lb, double R,
                   int maxn, int maxm, pba_result *out) {
    TextCall t;
    const int st = text_prologue(ctx, "pba_align_text", a, a_fwd, la, b, b_fwd, lb, R, maxn, maxm, out, &t, [](int g) { return g; }, [&] {
        return text_pair_bitvec(ctx, a, a_fwd, b, b_fwd, t.c, R, maxn, maxm, out, nullptr, 0, nullptr, false, !t.hooks.stream);
    });
    if (st) return st < 0 ? st : PBA_OK;
    uint8_t *d_res = nullptr;
    POOL(POOL_TXT_OUT, kTxtOutOps, d_res);
    hipLaunchKernelGGL(k_align_bytes, dim3(1), dim3(PBA_WAVE), t.pl.lds, ctx->stream, t.da, a_fwd ? 1 : -1, t.c.len_a, t.db,
                       b_fwd ? 1 : -1, t.c.len_b, t.pl.cfg, (pba_result *)d_res);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_res, sizeof(pba_result), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

// ---- traceback
int pba_align_text_trace(pba_ctx *ctx, const char *a, int a_fwd, int la, const char *b, int b_fwd, int lb, double R,
                         int maxn, int maxm, pba_result *out, uint8_t *ops, int32_t ops_cap, int32_t *nedit) {
    if (!nedit || (!ops && ops_cap) || ops_cap < 0) return PBA_E_INVALID;
    TextCall t;
    const int st = text_prologue(ctx, "pba_align_text_trace", a, a_fwd, la, b, b_fwd, lb, R, maxn, maxm, out, &t,
                                 [&](int g) { *nedit = 0; return g; }, [&] {
        return text_pair_bitvec(ctx, a, a_fwd, b, b_fwd, t.c, R, maxn, maxm, out, ops, ops_cap, nedit, true, !t.hooks.stream);
    });
    if (st) return st < 0 ? st : PBA_OK;
    const TextClip &c = t.c;
    const uint64_t pb = band_matrix_cells(c);
    if (pb > kTraceBudget) PBA_FAIL(PBA_E_NOMEM, "parent codes exceed the traceback budget");
    // result, nedit and the offsets the walk reads (ops_off[0..1], par_off[0]), then the ops
    const size_t o_off = 64, o_ops = 128;
    uint8_t *d_res = nullptr, *d_par = nullptr;
    POOL(POOL_TXT_OUT, o_ops + (size_t)ops_cap + 16, d_res);
    POOL(POOL_TXT_PAR, pb + 16, d_par);
    const uint64_t offs[4] = {0, (uint64_t)ops_cap, 0, 0};
    HIPCHK(hipMemcpyAsync(d_res + o_off, offs, sizeof offs, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_align_bytes_trace, dim3(1), dim3(PBA_WAVE), t.pl.lds, ctx->stream, t.da, a_fwd ? 1 : -1, c.len_a, t.db,
                       b_fwd ? 1 : -1, c.len_b, t.pl.cfg, (pba_result *)d_res, d_par, (uint16_t *)nullptr);
    hipLaunchKernelGGL(k_trace_walk, dim3(1), dim3(64), 0, ctx->stream, (const pba_result *)d_res, (const uint8_t *)d_par,
                       (const uint64_t *)(d_res + o_off) + 2, d_res + o_ops, (const uint64_t *)(d_res + o_off),
                       (int32_t *)(d_res + 32), 1u);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_res, sizeof(pba_result), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(nedit, d_res + 32, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));                   // (offs is a host array: the copy above has completed too)
    const int32_t ncopy = std::min(*nedit, ops_cap);
    if (ncopy > 0) {
        HIPCHK(hipMemcpyAsync(ops, d_res + o_ops, (size_t)ncopy, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return PBA_OK;
}

// The reference's DP matrix of one pair (seq_aligner.h:81 `mat`, read through get_cost / get_parent :131-134 by
// locator.cpp:86 and by whoever inspects an alignment): cost[i * W + c] / parent[i * W + c] for cell (i, j), W = 2*max_dst+1,
// c = j - i + max_dst -- the reference's own diagonal-stripe layout.  Cells the call writes hold their values (init_cell's
// borders, the band of every row swept: all of them, or up to the row of the early failure, out->diag_cost / rc tell which);
// the others hold cost 0xFFFF, parent 0 (the reference leaves whatever an earlier call wrote there).
int pba_align_text_matrix(pba_ctx *ctx, const char *a, int a_fwd, int la, const char *b, int b_fwd, int lb, double R, int maxn,
                          int maxm, pba_result *out, uint16_t *cost, uint8_t *parent, uint64_t cap_cells, int32_t *rows_swept) {
    if ((!cost || !parent) && cap_cells) return PBA_E_INVALID;
    TextCall t;
    uint64_t pb = 0;                                                    // cells: (len_a + 1) * (2*max_dst + 1)
    const int st = text_prologue(ctx, "pba_align_text_matrix", a, a_fwd, la, b, b_fwd, lb, R, maxn, maxm, out, &t, [&](int g) {
        pb = band_matrix_cells(t.c);
        if (rows_swept) *rows_swept = 0;
        if (g < 0) return g;
        if (pb * 3 > kTraceBudget) PBA_FAIL(PBA_E_NOMEM, "the matrix exceeds the traceback budget");
        if (cap_cells < pb) PBA_FAIL(PBA_E_INVALID, "pba_align_text_matrix: cost / parent hold fewer than (len_a + 1) * (2*max_dst + 1) cells");
        if (g == 1) { memset(cost, 0xFF, (size_t)pb * 2); memset(parent, 0, (size_t)pb); }   // the size guard: nothing is written (seq_aligner.h:104-107)
        return g;
    }, [] { return 1; });                                               // (the matrix is the row sweep's: no fast form)
    if (st) return st < 0 ? st : PBA_OK;
    const TextClip &c = t.c;
    const int md = c.md;
    uint8_t *d_res = nullptr, *d_par = nullptr, *d_cst = nullptr;
    POOL(POOL_TXT_OUT, kTxtOutOps, d_res);
    POOL(POOL_TXT_PAR, pb + 16, d_par);
    POOL(POOL_TXT_CST, 2 * pb + 16, d_cst);
    HIPCHK(hipMemsetAsync(d_par, 0, pb, ctx->stream));
    HIPCHK(hipMemsetAsync(d_cst, 0xFF, 2 * pb, ctx->stream));
    hipLaunchKernelGGL(k_align_bytes_trace, dim3(1), dim3(PBA_WAVE), t.pl.lds, ctx->stream, t.da, a_fwd ? 1 : -1, c.len_a, t.db,
                       b_fwd ? 1 : -1, c.len_b, t.pl.cfg, (pba_result *)d_res, d_par, (uint16_t *)d_cst);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_res, sizeof(pba_result), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(cost, d_cst, 2 * pb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(parent, d_par, pb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    // init_cell (seq_aligner.h:139-150): row 0 is D(0,j) = j, INSERT, for j <= max_dst
    const uint64_t W = 2ull * md + 1;
    int swept = 0;
    for (int j = 0; j <= md; ++j) { cost[(uint64_t)md + j] = (uint16_t)j; parent[(uint64_t)md + j] = j ? 2 : 0; }
    // rows swept: every row up to len_a, or up to the early failure -- the last row whose diagonal-side cell was written
    for (swept = out->len_a; swept > 0; --swept) {
        const int jlo = swept - md > 0 ? swept - md : 0;
        if (cost[(uint64_t)swept * W + (uint64_t)(jlo - swept + md)] != 0xFFFF) break;
    }
    if (rows_swept) *rows_swept = swept;
    return PBA_OK;
}

// ---- edit scripts of a batch, or their votes
// the device side of a call of trace_batch
struct TraceBufs { DevBuf pairs, out, ops, ooff, ne; uint64_t ops_total; };

// the results of a finished call to the caller's arrays (`out` only where the last copy of it is stale), synchronised
static int trace_results(pba_ctx *ctx, const TraceBufs &d, size_t n, bool copy_out, pba_result *out, uint8_t *ops, const uint64_t *ops_off,
                         int32_t *nedit, bool vote) {
    if (copy_out) HIPCHK(hipMemcpyAsync(out, d.out.p, sizeof(pba_result) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (!vote) {
        HIPCHK(hipMemcpyAsync(nedit, d.ne.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
        if (d.ops_total) HIPCHK(hipMemcpyAsync(ops + ops_off[0], d.ops.p, d.ops_total, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

// The row-sweep form: one parent byte per band cell, every pair's codes resident at once; one launch and the walk, nothing
// to redo.
static int trace_rowsweep(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R, const Plan &pl,
                          uint64_t budget, const TraceBufs &d, pba_result *out, uint8_t *ops, const uint64_t *ops_off, int32_t *nedit) {
    (void)hipEventRecord(ctx->ev[2], ctx->stream);
    std::vector<uint64_t> par_off(n + 1, 0);
    for (size_t q = 0; q < n; ++q)
        par_off[q + 1] = par_off[q] + ((band_matrix_cells(text_clip(pairs[q].a_len, pairs[q].b_len, R)) + 15) & ~15ull);
    if (par_off[n] > budget) PBA_FAIL(PBA_E_NOMEM, "parent codes of this batch exceed the traceback budget: split it");
    DevBuf d_par, d_poff;
    HIPCHK(hipMalloc(&d_par.p, par_off[n] + 16));
    HIPCHK(hipMalloc(&d_poff.p, sizeof(uint64_t) * (n + 1)));
    HIPCHK(hipMemcpyAsync(d_poff.p, par_off.data(), sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_align_pairs_trace, dim3((uint32_t)n), dim3(PBA_WAVE), pl.lds, ctx->stream, A->dev(), B->dev(),
                       d.pairs.as<pba_pair>(), (uint32_t)n, pl.cfg, d.out.as<pba_result>(), d_par.as<uint8_t>(),
                       d_poff.as<uint64_t>());
    hipLaunchKernelGGL(k_trace_walk, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, ctx->stream, d.out.as<pba_result>(),
                       d_par.as<uint8_t>(), d_poff.as<uint64_t>(), d.ops.as<uint8_t>(), d.ooff.as<uint64_t>(),
                       d.ne.as<int32_t>(), (uint32_t)n);
    (void)hipEventRecord(ctx->ev[3], ctx->stream);
    ctx->prof.nb_first = 0; ctx->prof.n_first = (uint32_t)n; ctx->prof.nb_redo = 0; ctx->prof.n_redo = 0;
    ctx->prof.align_redo_ms = 0.f;
    HIPCHK(hipGetLastError());
    const int st = trace_results(ctx, d, n, true, out, ops, ops_off, nedit, false);
    if (st != PBA_OK) return st;
    prof_finish(ctx);
    return PBA_OK;
}

// The paths of a batch, to the one outlet `into` names (pba_host.h: TraceInto).  Scripts alone leave the device here; the other
// outlets write device arrays of the caller's.
int trace_batch(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R, int maxn, int maxm,
                int kernel, pba_result *out, const TraceInto &into) {
    const bool scripts = into.kind == TraceInto::SCRIPTS;    // else the path goes to a sink of its own: no script leaves the device
    uint8_t *const ops = into.ops;
    const uint64_t *const ops_off = into.ops_off;
    int32_t *const nedit = into.nedit;
    if (!ctx || !A || !B || (!pairs && n) || (!out && n) || (scripts && ((!ops_off && n) || (!nedit && n)))) return PBA_E_INVALID;
    if (n == 0) return PBA_OK;
    if (n > 0x7FFFFFFFull) PBA_FAIL(PBA_E_INVALID, "too many pairs in one batch");
    if (A->non_acgt || B->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "a sequence set holds bytes outside ACGT: use pba_align_text_trace");
    HIPCHK(hipSetDevice(ctx->device));
    tu_attrs(ctx);
    int mdmax;
    uint64_t ops_max;
    int st = check_pairs(ctx, A, B, pairs, n, R, scripts ? ops_off : nullptr, &mdmax, &ops_max);
    if (st != PBA_OK) return st;
    Plan pl;
    st = make_plan(ctx, R, maxn, maxm, kernel, mdmax, &pl);
    if (st != PBA_OK) return st;
    if (!scripts && pl.nb1 == 0) {
        char msg[96];
        snprintf(msg, sizeof msg, "%s from the walk need the bit-vector kernel (band too wide)", into.name());
        PBA_FAIL(PBA_E_TOOLONG, msg);
    }
    const uint64_t tmp_bytes = into.tmp_bytes(ops_max);
    TraceBufs d;
    d.ops_total = scripts ? ops_off[n] - ops_off[0] : 0;
    HIPCHK(hipMalloc(&d.pairs.p, sizeof(pba_pair) * n));
    HIPCHK(hipMalloc(&d.out.p, sizeof(pba_result) * n));
    HIPCHK(hipMalloc(&d.ops.p, d.ops_total + 16));
    HIPCHK(hipMalloc(&d.ooff.p, sizeof(uint64_t) * (n + 1)));
    HIPCHK(hipMalloc(&d.ne.p, sizeof(int32_t) * n));
    std::vector<uint64_t> rel(n + 1, 0);
    if (scripts) for (size_t q = 0; q <= n; ++q) rel[q] = ops_off[q] - ops_off[0];
    HIPCHK(hipMemcpyAsync(d.pairs.p, pairs, sizeof(pba_pair) * n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d.ooff.p, rel.data(), sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    const TraceHooks hooks = trace_hooks_from_env();
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    free_b += ctx->scratch_bytes;                            // the scratch kept from earlier calls is ours to reuse
    const uint64_t budget = hooks.budget_set ? std::min<uint64_t>(hooks.budget, (uint64_t)(free_b / 10) * 9)
                                             : std::min<uint64_t>(kTraceBudget, (uint64_t)(free_b / 10) * 8);
    if (pl.nb1 == 0) return trace_rowsweep(ctx, A, B, pairs, n, R, pl, budget, d, out, ops, ops_off, nedit);
    // bit-vector array: 2 bits per processed cell in a per-wavefront scratch area, walked by the same wavefront.
    // First launch: every pair, narrow window, scratch sized for it (so more wavefronts fit the budget); second
    // launch: the pairs that came back uncertified, reference band.
    const TracedLaunch t{A->dev(), B->dev(), d.pairs.as<pba_pair>(), d.out.as<pba_result>(), pl.lds, into.ck_only() || !hooks.stream};
    TracePass tp{};
    auto before = [&](int pass, const std::vector<uint32_t> &redo) {
        return trace_pass_size(ctx, pairs, pass ? redo.data() : nullptr, pass ? (uint32_t)redo.size() : (uint32_t)n, R,
                               pass ? pl.nb2 : pl.nb1, pass != 0, t.ck, tmp_bytes, pl.lds, budget, &tp);
    };
    auto launch = [&](int nb, const uint32_t *ids, uint32_t cnt) {          // the tag becomes the job's type here, nowhere else
        switch (into.kind) {
        case TraceInto::SCRIPTS: launch_traced(ctx, t, ScriptJob{d.ops.as<uint8_t>(), d.ooff.as<uint64_t>(), d.ne.as<int32_t>()}, nb, pl.cfg, ids, cnt, tp); break;
        case TraceInto::VOTES:
            if (into.vote.box_off) launch_traced(ctx, t, VoteJob<true>{into.vote, into.overlap_min}, nb, pl.cfg, ids, cnt, tp);
            else launch_traced(ctx, t, VoteJob<false>{into.vote, into.overlap_min}, nb, pl.cfg, ids, cnt, tp);
            break;
        case TraceInto::RUNS: launch_traced(ctx, t, CigarJob{into.slots}, nb, pl.cfg, ids, cnt, tp); break;
        case TraceInto::WINDOWS: launch_traced(ctx, t, WindowJob{into.slots}, nb, pl.cfg, ids, cnt, tp); break;
        case TraceInto::ALLELES: launch_traced(ctx, t, AlleleJob{into.slots, into.sites, into.overlap_min}, nb, pl.cfg, ids, cnt, tp); break;
        }
    };
    auto collect = [&](std::vector<uint32_t> &redo) { return fetch_results(ctx, d.out.p, out, n, &redo); };
    auto finish = [&](bool redone) { return trace_results(ctx, d, n, redone, out, ops, ops_off, nedit, !scripts); };
    return narrow_then_redo(ctx, pl, nullptr, (uint32_t)n, launch, collect, finish, before);
}

int pba_align_batch_trace(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R,
                          int maxn, int maxm, int kernel, pba_result *out, uint8_t *ops, const uint64_t *ops_off,
                          int32_t *nedit) {
    return trace_batch(ctx, A, B, pairs, n, R, maxn, maxm, kernel, out, TraceInto::scripts(ops, ops_off, nedit));
}
