// pba_host.h -- host-side objects and helpers shared by the translation units of libpba.so (pba_core.hip: context,
// sequence sets; pba_index.hip: seed index; pba_align.hip: explicit pairs and edit scripts; pba_drivers.hip: the reference's ordered
// first-success loops; pba_overlap.hip: all-vs-all; pba_cons.hip: consensus voting; pba_pileup.hip: the pile-ups' vote boxes, their votes and evolve; pba_pile_drivers.hip: read correction, contig polishing and layout consensus over them; pba_stream.hip: streamed locate and mapping; pba_layout.hip: layout; pba_clip.hip: clipping; pba_hpc.hip: homopolymer compression; pba_census.hip: seed-key census; pba_cigar.hip: run-length alignments and PAF; pba_windows.hip: per-window counts and trimmed rows; pba_sites.hip: variant sites and per-row alleles;
// pba_fastx.hip: FASTA / FASTQ in, FASTA out; pba_qual.hip: per-base evidence, its summaries and spans, FASTQ out).  Internal: nothing here is part of the C ABI (include/pba.h).
// (What host and device share about the seed index -- the visiting rule, compress / compress_masks -- is index_plan.h's.)
// Also here, once for all of them: the clip of seq_aligner.h:94-102 (text_clip), the launch plan (make_plan), the host
// protocol of every aligning entry point but the all-vs-all walk -- narrow window first, the uncertified items again at the
// reference band (narrow_then_redo) --, the owner of a set of vote boxes (VoteBoxes), a found row's accessors (row_accessors,
// walk_agrees) and the seed-round loop of spaced_seed.cpp:409-452 (seed_rounds).
#ifndef PBA_HOST_H
#define PBA_HOST_H

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <memory>
#include <new>
#include <vector>

#include "align_alleles.h"
#include "align_cigar.h"
#include "align_common.h"
#include "consensus.h"
#include "dev_common.h"
#include "pba.h"
#include "seed_index.h"
#include "seq_layout.h"

#define PBA_INTERNAL __attribute__((visibility("hidden")))
// a kernel that takes more than the default 64 KB of dynamic LDS; every translation unit does this once for the kernels
// it launches, once per ctx (tu_attrs(ctx) in each .hip: the attribute is per device, and a ctx is bound to one)
// (128 KB of dynamic LDS: the largest LDS sort and the largest band row, with room for a kernel's static arrays; a refused
// attribute must not linger as the thread's last error)
#define PBA_BIG_LDS(kernel)                                                                                            \
    do {                                                                                                               \
        if (hipFuncSetAttribute((const void *)(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024) != hipSuccess) \
            (void)hipGetLastError();                                                                                   \
    } while (0)

// ---------------------------------------------------------------------------------------------
// host-side objects
// ---------------------------------------------------------------------------------------------
// The entry / offset arrays of the index destroyed last, kept for the next build, one deep per slot (a step of the locate loop
// builds and drops one index: the hipFree / hipMalloc pair of its 40 MB cost 0.2 ms of a 48 ms step).  IXC_ENT / IXC_OFF: a
// destroyed index's arrays; IXC_ENT2: the entry buffer a build did not keep.
enum { IXC_ENT = 0, IXC_OFF, IXC_ENT2 };
struct IxCache {
    struct { void *p; size_t cap; } slot[3] = {};
    // a device array of at least `bytes`: the slot's if it is large enough, else a new one
    hipError_t take(int s, size_t bytes, void **p, size_t *cap) {
        if (slot[s].p && slot[s].cap >= bytes) { *p = slot[s].p; *cap = slot[s].cap; slot[s].p = nullptr; slot[s].cap = 0; return hipSuccess; }
        const hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) *cap = bytes; else *p = nullptr;
        return e;
    }
    // kept when the slot is empty (the work that used the array was synchronised by the call that returned its results),
    // else back to the device
    void give(int s, void *p, size_t cap) {
        if (!p) return;
        if (!slot[s].p) { slot[s].p = p; slot[s].cap = cap; }
        else (void)hipFree(p);
    }
    void release() { for (auto &x : slot) { if (x.p) (void)hipFree(x.p); x.p = nullptr; x.cap = 0; } }
};

struct pba_ctx {
    int device;
    hipStream_t own_stream, stream;
    hipDeviceProp_t prop;
    hipEvent_t ev[6];        // index begin/end, narrow launch begin/end, redo launch begin/end (narrow_then_redo, prof_finish)
    hipEvent_t ev_aux;       // "the small D2H copy queued before the last kernel has landed" (index build: sizes before the last scatter)
    uint32_t *d_queue;       // work-queue counters of the persistent aligning kernels (one per launch in flight)
    void *d_scratch;         // parent-bit scratch of the trace / vote kernels, kept between calls (tens of GB: mapping
    size_t scratch_bytes;    // it anew on every call cost seconds); grown on demand, freed with the ctx
    // Work buffers of the drivers, kept between calls for the same reason (hipMalloc / hipFree of the 11 GB candidate
    // array of a million-read target range cost more than the kernels that fill it; the 4 MB of per-read rows of a
    // locate step cost 1 ms of a 50 ms step): grown on demand (pool_reserve), released by pba_ctx_trim or with the ctx.
    struct { void *p; size_t cap; } pool[32];
    // pinned host staging of the one-pair text entry points (pba_align_text*: one H2D and one D2H copy per call)
    void *h_stage;
    size_t h_stage_cap;
    uint32_t attr_done;      // translation units whose big-LDS kernel attributes are set on this ctx's device (tu_attrs)
    IxCache ix_cache;
    pba_profile prof;
    pba_correct_profile cprof;   // the most recent pba_correct_reads
    char err[512];
};

struct pba_seqs {
    pba_ctx *ctx;
    uint32_t n, max_len;
    uint64_t packed_bytes;   // packed payload resident in HBM (incl. alignment padding)
    bool non_acgt;           // some byte outside ACGT was packed as code 3 (C2I): the packed DP would match it against T
    uint8_t *d_alloc;        // allocation; d_packed = d_alloc + kSlack
    uint8_t *d_packed;
    uint64_t *d_off;
    uint32_t *d_len;
    uint32_t *d_planes;      // allocation of the two bit planes, interleaved word by word, kPlaneSlack zero word pairs around them
    uint64_t *d_poff;        // word offset of every sequence inside a plane
    uint64_t plane_words;    // words of one plane incl. its slack
    std::vector<uint64_t> h_off;
    std::vector<uint32_t> h_len;
    bool borrowed;           // the arrays belong to a stream's slot (pba_stream.hip): pba_seqs_destroy leaves the set alone, the stream frees it
    SeqSetDev dev() const { return SeqSetDev{d_packed, d_off, d_len, d_planes + 2 * kPlaneSlack, d_poff}; }
};
// a set of n sequences with nothing on the device yet: every other field is zero, h_off / h_len hold n + 1 zeros
static inline pba_seqs *seqs_new(pba_ctx *ctx, uint32_t n) {
    pba_seqs *s = new (std::nothrow) pba_seqs();
    if (s) { s->ctx = ctx; s->n = n; s->h_off.resize((size_t)n + 1); s->h_len.resize((size_t)n + 1); }
    return s;
}

struct pba_index {
    pba_ctx *ctx;
    size_t ent_cap, off_cap;     // bytes allocated behind d_ent / d_part_off
    uint32_t mask, seq_len, visited, nhead;
    int32_t tail_top;
    int mode, logP;
    uint64_t n_entries;
    uint64_t *d_ent;
    uint32_t *d_part_off;
    // pba_index_build_set: the sequences indexed and cum[0 .. n_seqs] = the exclusive prefix sum of their lengths -- an entry's
    // ordinal is the global position cum[c] + pos.  pba_index_build: n_seqs = 1, no cum.
    uint32_t n_seqs;
    uint32_t *d_cum;
    std::vector<uint32_t> h_cum;
    IndexDev dev() const { return IndexDev{d_ent, d_part_off, logP, mask, nhead, tail_top}; }
};

static inline int ctx_fail(pba_ctx *ctx, int st, const char *what, hipError_t e) {
    if (ctx)
        snprintf(ctx->err, sizeof ctx->err, "%s: %s", what, e == hipSuccess ? pba_strerror(st) : hipGetErrorString(e));
    return st;
}
#define HIPCHK(call)                                                        \
    do {                                                                    \
        hipError_t e__ = (call);                                            \
        if (e__ != hipSuccess) return ctx_fail(ctx, PBA_E_HIP, #call, e__); \
    } while (0)
#define PBA_FAIL(st, what) return ctx_fail(ctx, (st), (what), hipSuccess)
// "who: what" where code shared by several entry points fails: who is the public function that was called
static inline int ctx_fail_as(pba_ctx *ctx, int st, const char *who, const char *what) {
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return ctx_fail(ctx, st, msg, hipSuccess);
}
// (for a callee that has written ctx->err itself)
#define PBA_TRY(call) do { const int rc__ = (call); if (rc__ != PBA_OK) return rc__; } while (0)

// engine limits
static const int kRowSweepLdsCap = 96 * 1024;   // LDS bytes one wavefront may take for its band row (kMaxSeqLen, kSlack: seq_layout.h)

// pool slots
enum { POOL_OVL_CAND = 0, POOL_OVL_TMP, POOL_OVL_ITEMS, POOL_OVL_REDO, POOL_OVL_REDO_IN, POOL_OVL_OUT, POOL_OVL_SMALL,
       POOL_LOC_ROWS, POOL_LOC_AUX, POOL_REDO_IDS, POOL_IX_OFFS, POOL_IX_WORK,
       POOL_TXT_IN, POOL_TXT_OUT, POOL_TXT_PAR, POOL_TXT_CST, POOL_LOC_IDS, POOL_LOC_CTG, POOL_LAY_WORK, POOL_LAY_ROWS,
       POOL_FX_FILE, POOL_FX_TILES, POOL_FX_LINES, POOL_FX_RECS, POOL_FX_IMG, POOL_CLIP_ARENA, POOL_CLIP_WORK, POOL_CLIP_TEXT,
       POOL_HPC_WORK, POOL_HPC_TEXT, POOL_COUNT };
static_assert(POOL_COUNT <= 32, "pba_ctx::pool has 32 slots");
// a buffer of at least `bytes` in pool slot `slot` (contents undefined); grows by reallocation with 1/8 headroom
static inline int pool_reserve(pba_ctx *ctx, int slot, size_t bytes, void **out) {
    if (ctx->pool[slot].cap < bytes) {
        if (ctx->pool[slot].p) {
            (void)hipStreamSynchronize(ctx->stream);
            (void)hipFree(ctx->pool[slot].p);
            ctx->pool[slot].p = nullptr; ctx->pool[slot].cap = 0;
        }
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&ctx->pool[slot].p, want);
        if (e != hipSuccess) { (void)hipGetLastError(); e = hipMalloc(&ctx->pool[slot].p, bytes); if (e == hipSuccess) ctx->pool[slot].cap = bytes; }
        else ctx->pool[slot].cap = want;
        if (e != hipSuccess) { ctx->pool[slot].p = nullptr; return ctx_fail(ctx, PBA_E_NOMEM, "work buffer", e); }
    }
    *out = ctx->pool[slot].p;
    return PBA_OK;
}
#define POOL(slot, bytes, ptr)                                                     \
    do {                                                                           \
        void *p__ = nullptr;                                                       \
        int st__ = pool_reserve(ctx, (slot), (bytes), &p__);                       \
        if (st__ != PBA_OK) return st__;                                           \
        (ptr) = (decltype(ptr))p__;                                                \
    } while (0)

// a pooled buffer seen through the same face as a DevBuf (not owned: the ctx keeps it)
struct BufRef {
    void *p = nullptr;
    template <class T> T *as() const { return (T *)p; }
};

// A device-to-device copy of any size: in pieces of 1 GiB.  (One hipMemcpyAsync of 37.6 GB -- the packed reads of BASELINE
// configs[4] -- copied only the size modulo 2^32 on ROCm 7.2: tools/rehearse_config4.py found the reads beyond the first
// 3.2 GB missing; tests/test_gpu_parity.py: test_packed_set_beyond_4_gib.)
static inline hipError_t copy_d2d(void *dst, const void *src, size_t bytes, hipStream_t stream) {
    const size_t piece = (size_t)1 << 30;
    for (size_t at = 0; at < bytes; at += piece) {
        const hipError_t e = hipMemcpyAsync((uint8_t *)dst + at, (const uint8_t *)src + at, std::min(piece, bytes - at), hipMemcpyDeviceToDevice, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// ... and a memset likewise
static inline hipError_t memset_big(void *dst, int v, size_t bytes, hipStream_t stream) {
    const size_t piece = (size_t)1 << 30;
    for (size_t at = 0; at < bytes; at += piece) {
        const hipError_t e = hipMemsetAsync((uint8_t *)dst + at, v, std::min(piece, bytes - at), stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Workgroups for a kernel that walks n elements with a grid-stride loop: one element per thread up to 2^30 threads.  (A
// launch's global size -- workgroups x threads -- is a 32-bit number; a launch asking for more does not fail, it runs a part.)
static inline uint32_t elem_grid(uint64_t n, uint32_t threads) {
    const uint64_t blocks = (n + threads - 1) / threads, cap = ((uint64_t)1 << 30) / threads;
    return (uint32_t)std::max<uint64_t>(1, std::min(blocks, cap));
}

// the ctx's pinned host staging buffer, at least `bytes` (one H2D / D2H copy per call of the one-pair text entry points; small
// results a host decision waits for)
static inline int stage_reserve(pba_ctx *ctx, size_t bytes) {
    if (ctx->h_stage_cap >= bytes) return PBA_OK;
    if (ctx->h_stage) { (void)hipStreamSynchronize(ctx->stream); (void)hipHostFree(ctx->h_stage); ctx->h_stage = nullptr; ctx->h_stage_cap = 0; }
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipHostMalloc(&ctx->h_stage, want, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError(); ctx->h_stage = nullptr;
        return ctx_fail(ctx, PBA_E_NOMEM, "pinned staging buffer", hipSuccess);
    }
    ctx->h_stage_cap = want;
    return PBA_OK;
}

// the ctx's scratch of the trace / vote kernels, at least `need` bytes (contents undefined)
static inline int scratch_reserve(pba_ctx *ctx, size_t need) {
    if (need <= ctx->scratch_bytes) return PBA_OK;
    if (ctx->d_scratch) { HIPCHK(hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->d_scratch); }
    ctx->d_scratch = nullptr; ctx->scratch_bytes = 0;
    HIPCHK(hipMalloc(&ctx->d_scratch, need));
    ctx->scratch_bytes = need;
    return PBA_OK;
}

// What every entry point that takes pba_strand_overlap rows checks of them on the host, before anything is uploaded (who:
// its name, in front of the message); want_dir: dir is read too; key_limits: the rows, reads and lengths must also fit the
// u64 keys of the layout's atomics (pba_layout_create, pba_layout_place; pba_clip_* keeps no key).
#define ROWS_FAIL(st, what) return ctx_fail_as(ctx, (st), who, (what))
static inline int check_overlap_rows(pba_ctx *ctx, const char *who, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows,
                                     bool want_dir, bool key_limits) {
    if (key_limits) {
        if (n_rows >= (1ull << 32)) ROWS_FAIL(PBA_E_TOOLONG, "2^32 rows or more (a key holds 32 bits of row index)");
        if (reads->n >= (1u << 28)) ROWS_FAIL(PBA_E_TOOLONG, "2^28 reads or more");
        if (reads->max_len > 0xFFFFu) ROWS_FAIL(PBA_E_TOOLONG, "a read of more than 65 535 bases (a key holds 16 bits of length)");
    }
    const int64_t n = reads->n;
    for (uint64_t k = 0; k < n_rows; ++k) {
        const pba_strand_overlap &r = rows[k];
        if (r.target < 0 || r.target >= n || r.query < 0 || r.query >= n) ROWS_FAIL(PBA_E_INVALID, "a row names a read outside the set");
        if (r.target == r.query) ROWS_FAIL(PBA_E_INVALID, "a row pairs a read with itself");
        if (r.strand != 1 && r.strand != -1) ROWS_FAIL(PBA_E_INVALID, "a row's strand is neither +1 nor -1");
        if (want_dir && r.dir != 1 && r.dir != -1) ROWS_FAIL(PBA_E_INVALID, "a row's dir is neither +1 nor -1");
        const int64_t lt = reads->h_len[r.target], lq = reads->h_len[r.query];
        if (r.t_beg < 0 || r.t_beg >= r.t_end || r.t_end > lt || r.q_beg < 0 || r.q_beg >= r.q_end || r.q_end > lq)
            ROWS_FAIL(PBA_E_INVALID, "a row's interval is empty or outside its read");
    }
    return PBA_OK;
}

// RAII for temporaries so early returns do not leak device memory
struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T> T *as() const { return (T *)p; }
    void reset() { if (p) (void)hipFree(p); p = nullptr; }
};

// The time of a stage between two events on the ctx's stream, added to *acc when the scope ends (every stage ends
// synchronised): a stage times itself, whichever way it returns.
struct StageClock {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~StageClock() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    bool init() { return hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess; }
    struct Scope {
        const StageClock &c; hipStream_t s; float *acc;
        ~Scope() {
            float ms = 0.f;
            (void)hipEventRecord(c.e1, s);
            if (hipEventSynchronize(c.e1) == hipSuccess && hipEventElapsedTime(&ms, c.e0, c.e1) == hipSuccess) *acc += ms;
        }
    };
    Scope time(hipStream_t s, float *acc) const { (void)hipEventRecord(e0, s); return Scope{*this, s, acc}; }
};

// One set of `cap` vote boxes on the device (consensus.h: sel / sup / tot, and a text byte per box where the owner keeps
// one): two of them ping-pong in a pba_cons, one is a pba_pileup's arena.
struct VoteBoxes {
    ConsDev dev{};
    void release() {
        for (void *q : {(void *)dev.sel, (void *)dev.sup, (void *)dev.tot, (void *)dev.txt})
            if (q) (void)hipFree(q);                        // (hipFree waits for the work that uses the buffer)
        dev = ConsDev{nullptr, nullptr, nullptr, nullptr};
    }
    bool alloc(size_t cap, bool txt) {                      // all or nothing; a refused hipMalloc does not linger as the last error
        if (hipMalloc((void **)&dev.sel, cap * 8) == hipSuccess && hipMalloc((void **)&dev.sup, cap * 8) == hipSuccess &&
            hipMalloc((void **)&dev.tot, cap * 4) == hipSuccess && (!txt || hipMalloc((void **)&dev.txt, cap) == hipSuccess))
            return true;
        (void)hipGetLastError();
        release();
        return false;
    }
    // boxes [first, first + k) to the host, synchronised
    int to_host(pba_ctx *ctx, size_t first, int k, uint16_t *sel, uint16_t *sup, int32_t *tot) const {
        if (k <= 0) return PBA_OK;
        HIPCHK(hipMemcpyAsync(sel, dev.sel + first, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(sup, dev.sup + first, (size_t)k * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(tot, dev.tot + first, (size_t)k * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return PBA_OK;
    }
};

// ---------------------------------------------------------------------------------------------
// host API: alignment
// ---------------------------------------------------------------------------------------------
// What align() looks at of its two accessors.  seq_aligner.h:94-102 clips the longer one to the shorter + max_dst BEFORE
// anything is sized, checked or read -- locator.cpp:80-81 hands it the whole rest of an 800 kb contig, ref_seq.h:282-286 the
// whole rest of the reference -- so the engine's own limit, the size guard and the H2D copy all see the clipped lengths.
// Same FP64 product and truncation as aln_params (dev_common.h); given (len_a, len_b) the kernels derive the same block again.
// The host's one restatement: band and scratch sizes derive from it.  (long long for the text entry points' unchecked lengths;
// for lengths pair_ok admits the sums equal the int form's.)
struct TextClip { int len_a, len_b, md; };
static inline TextClip text_clip(int la, int lb, double R) {
    TextClip c;
    if (lb >= la) { c.len_a = la; c.md = 1 + (int)((double)la * R); c.len_b = (int)std::min<long long>(lb, (long long)la + c.md); }
    else          { c.len_b = lb; c.md = 1 + (int)((double)lb * R); c.len_a = (int)std::min<long long>(la, (long long)lb + c.md); }
    return c;
}
static inline int max_dst_of(int la, int lb, double R) { return text_clip(la, lb, R).md; }
// cells of the reference's band matrix: (len_a + 1) * (2*max_dst + 1)
static inline uint64_t band_matrix_cells(const TextClip &c) { return ((uint64_t)c.len_a + 1) * (2ull * c.md + 1); }

// Launch plan for a batch whose widest band is max_dst_max.
struct Plan {
    AlignCfg cfg;
    size_t lds;
    int nb1;     // first launch: 0 = row sweep, else bit-vector array with nb1 blocks per lane (narrow band)
    int nb2;     // second launch (uncertified pairs only): bit-vector array at the reference band
};

static inline int make_plan(pba_ctx *ctx, double R, int maxn, int maxm, int kernel, int max_dst_max, Plan *pl) {
    if (!(R > 0.0) || !(R < 1.0)) PBA_FAIL(PBA_E_INVALID, "R must be in (0,1)");
    if (kernel != PBA_KERNEL_AUTO && kernel != PBA_KERNEL_ROWSWEEP && kernel != PBA_KERNEL_BITVEC)
        PBA_FAIL(PBA_E_INVALID, "unknown kernel");
    const bool bv = kernel != PBA_KERNEL_ROWSWEEP && bitvec_supports(max_dst_max);
    if (kernel == PBA_KERNEL_BITVEC && !bv) PBA_FAIL(PBA_E_TOOLONG, "band too wide for the bit-vector kernel");
    // the bit-vector kernel needs LDS only for its m <= 10 corner (a 23-cell row at most); the row sweep
    // needs the whole band row
    const int nb_hi = bv ? bv_nb_for_span(bv_full_wl(max_dst_max) + max_dst_max) : 0;     // the most blocks per lane a launch of this plan uses
    const long long W = bv ? (long long)PBA_BV_FIN_WORDS(nb_hi) * 2 : 2ll * max_dst_max + 1;   // (u16 cells: the fin words of bitvec_pass)
    const long long bytes = ((W * 2 + 15) / 16) * 16;
    if (bytes > kRowSweepLdsCap) PBA_FAIL(PBA_E_TOOLONG, "band row does not fit the per-wavefront LDS budget");
    pl->cfg.R = R; pl->cfg.maxn = maxn; pl->cfg.maxm = maxm; pl->cfg.full_band = 0;
    pl->cfg.row_cap = (int)(bytes / 2);
    pl->lds = (size_t)bytes;
    pl->nb1 = bv ? bv_nb_for_span(bv_first_wl(max_dst_max) + bv_first_w(max_dst_max)) : 0;
    pl->nb2 = bv ? bv_nb_for_span(bv_full_wl(max_dst_max) + max_dst_max) : 0;
    return PBA_OK;
}

// LDS of one launch of a score-only kernel (k_align_pairs, k_locate, k_spaced_round) in ring nb: the fin words of THAT ring, not
// of the plan's widest, and behind them the sweep's text ring (text_ring.h); in rings 1 and 2 the match-mask table with the
// fin words on it, the ring and the fin superblock word (eq_table.h).  k_locate<2> of a 15 kb batch planned for a
// re-run in ring 4 then takes 2 944 bytes per wavefront: with LocWalkLds (1 792) that is 4 736 of the 5 120 a wavefront may
// have with 32 of them on a CU's 160 KB, which the widest ring's fin words would not fit.  nb = 0 (row sweep): the plan's band row.
struct LaunchLds { size_t lds; AlignCfg cfg; };
static inline LaunchLds launch_lds(const Plan &pl, int nb) {
    LaunchLds l{pl.lds, pl.cfg};
    if (nb) {
        l.lds = ((size_t)PBA_BV_LDS_BYTES(nb) + 15) / 16 * 16;
        l.cfg.row_cap = (int)(l.lds / 2);
    }
    return l;
}

// Workgroups for a persistent launch: enough to fill every CU (up to 8 waves per SIMD, as many as the LDS
// allows), never more than there are work items.  Any residency works: the queue needs no co-residency.
static inline uint32_t persistent_grid(const pba_ctx *ctx, uint32_t n_items, int waves_per_wg, size_t lds_per_wave) {
    const uint32_t cus = (uint32_t)ctx->prop.multiProcessorCount;
    uint32_t wg_per_cu = 32u / (uint32_t)waves_per_wg;
    const size_t lds_wg = lds_per_wave * (size_t)waves_per_wg;
    if (lds_wg) wg_per_cu = std::min<uint32_t>(wg_per_cu, (uint32_t)std::max<size_t>(1, (160 * 1024) / lds_wg));
    const uint32_t need = (n_items + (uint32_t)waves_per_wg - 1) / (uint32_t)waves_per_wg;
    return std::max(1u, std::min(need, cus * wg_per_cu));
}

static inline void prof_finish(pba_ctx *ctx) {      // all launches of the call have completed (stream synchronised)
    (void)hipEventElapsedTime(&ctx->prof.align_ms, ctx->ev[2], ctx->ev[3]);
    if (ctx->prof.n_redo) (void)hipEventElapsedTime(&ctx->prof.align_redo_ms, ctx->ev[4], ctx->ev[5]);
}

// The host protocol of the aligning entry points: every item at the narrow window, then the items that came
// back PBA_RC_UNCERTIFIED again at the reference band (cfg.full_band = 1).  Owns the queue reset, ev[2..5], the profile
// fields of the two launches, the redo ids (one pooled slot) and prof_finish.  The caller supplies
//   launch(nb, ids, cnt)   one launch of its kernel over `cnt` items (ids: device, nullable = items 0 .. cnt-1)
//   collect(redo)          after the narrow launch: copy back what carries the verdicts, synchronise, list the items to redo
//   finish(redone)         after the last launch: copy back the results (again, where a redo rewrote them) and synchronise
//   before(pass, redo)     optional, before each launch: what depends on the pass (the trace kernels' scratch and grid)
struct NoPassHook { int operator()(int, const std::vector<uint32_t> &) const { return PBA_OK; } };
template <class Launch, class Collect, class Finish, class Before = NoPassHook>
static inline int narrow_then_redo(pba_ctx *ctx, Plan &pl, const uint32_t *ids, uint32_t cnt, Launch launch, Collect collect,
                                   Finish finish, Before before = Before()) {
    std::vector<uint32_t> redo;
    ctx->prof.nb_first = (uint32_t)pl.nb1; ctx->prof.n_first = cnt; ctx->prof.nb_redo = 0; ctx->prof.n_redo = 0;
    ctx->prof.align_redo_ms = 0.f;
    for (int pass = 0; pass < 2; ++pass) {
        const int nb = pass ? pl.nb2 : pl.nb1;
        if (pass) {
            uint32_t *d_ids = nullptr;
            cnt = (uint32_t)redo.size();
            POOL(POOL_REDO_IDS, sizeof(uint32_t) * cnt, d_ids);
            HIPCHK(hipMemcpyAsync(d_ids, redo.data(), sizeof(uint32_t) * cnt, hipMemcpyHostToDevice, ctx->stream));
            ids = d_ids;
            pl.cfg.full_band = 1;
            ctx->prof.nb_redo = (uint32_t)nb; ctx->prof.n_redo = cnt;
        }
        int st = before(pass, redo);
        if (st != PBA_OK) return st;
        (void)hipEventRecord(ctx->ev[pass ? 4 : 2], ctx->stream);
        HIPCHK(hipMemsetAsync(ctx->d_queue, 0, sizeof(uint32_t), ctx->stream));
        launch(nb, ids, cnt);
        (void)hipEventRecord(ctx->ev[pass ? 5 : 3], ctx->stream);
        HIPCHK(hipGetLastError());
        if (pass) break;
        st = collect(redo);
        if (st != PBA_OK) return st;
        if (redo.empty()) break;
    }
    const int st = finish(!redo.empty());
    if (st != PBA_OK) return st;
    prof_finish(ctx);
    return PBA_OK;
}

static inline bool pair_ok(const pba_seqs *S, uint32_t seq, int pos, int len, bool backward) {
    if (seq >= S->n || len < 0 || len > kMaxSeqLen || pos < 0) return false;
    const long long L = S->h_len[seq];
    if (len == 0) return pos <= L;
    return backward ? (pos < L && pos - (len - 1) >= 0) : ((long long)pos + len <= L);
}

// The accessors a found row hands to align (spaced_seed.cpp:274-276, 285; get_accessor, ref_seq.h:282-286) against the
// reference window [a_lo, a_hi) of index coordinates, whose text the pair addresses `org` further on; slen: the read's
// length.  Sets a_pos, a_len, b_pos, b_len and flags of *pr.
static inline void row_accessors(int dir, int j, int ref_pos, int a_lo, int a_hi, int org, int slen, pba_pair *pr) {
    const bool fwd = dir == 1;
    const int r_off = fwd ? ref_pos : ref_pos + 15;                             // spaced_seed.cpp:285
    pr->a_pos = r_off + org;
    pr->a_len = fwd ? a_hi - r_off : r_off - a_lo + 1;                          // get_accessor, ref_seq.h:284-285
    pr->b_pos = fwd ? j : slen - j - 1;                                         // spaced_seed.cpp:274-276, both directions
    pr->b_len = slen - j;
    pr->flags = fwd ? 0u : (PBA_A_BACKWARD | PBA_B_BACKWARD);
}
// the voting walk of a row re-ran to the row's own cost and matlens
static inline bool walk_agrees(const pba_result &o, int cost, int matlen_a, int matlen_b) {
    return o.rc >= 0 && o.cost == cost && o.matlen_a == matlen_a && o.matlen_b == matlen_b;
}

// spaced_seed's main loop (spaced_seed.cpp:409-452): rounds over the reads not found yet, the seed of a round drawn like
// the reference draws it (a fresh draw after a round that found something, else the seeds in file order; picks[] stands in
// for the values rand() returns), stop when every seed has failed in a row or after max_round.  Owns the pool, the rows'
// reset, found_round, the log and *n_rounds.  The caller supplies
//   round(mask, pool)    one round over the reads of `pool`, in order, into rows[]
//   after(done, last)    optional, once the round is logged as entry `done`; last: every seed has now failed in a row
struct NoAfterRound { int operator()(int, bool) const { return PBA_OK; } };
template <class Round, class After = NoAfterRound>
static inline int seed_rounds(uint32_t n_reads, const uint32_t *masks, int n_masks, const uint32_t *picks, int n_picks, int max_round,
                              pba_ss_row *rows, int32_t *found_round, pba_ss_round_log *log, int log_cap, int *n_rounds, Round round,
                              After after = After()) {
    std::vector<uint32_t> pool(n_reads), rest;
    for (uint32_t r = 0; r < n_reads; ++r) { pool[r] = r; found_round[r] = 0; memset(&rows[r], 0, sizeof rows[r]); rows[r].read = (int32_t)r; rows[r].j = -1; }
    int nfailure = 0, draws = 0, done = 0;
    for (int nround = 1; nround <= max_round; ++nround) {
        const uint32_t mask = nfailure == 0 ? masks[picks[draws++ % n_picks] % (uint32_t)n_masks] : masks[nfailure - 1];   // :412
        int st = round(mask, pool);
        if (st != PBA_OK) return st;
        int nmatches = 0;
        rest.clear();
        for (uint32_t r : pool) {
            if (rows[r].found) { found_round[r] = nround; ++nmatches; }                     // erased from the pool, :443
            else rest.push_back(r);
        }
        if (done < log_cap) { log[done].round = nround; log[done].mask = mask; log[done].n_tried = (int32_t)pool.size(); log[done].n_found = nmatches; }
        pool.swap(rest);
        bool last = false;
        if (nmatches != 0) nfailure = 0;                                                    // :448-451
        else last = ++nfailure == n_masks;
        st = after(done, last);
        if (st != PBA_OK) return st;
        ++done;
        if (last) break;
    }
    *n_rounds = done;
    return PBA_OK;
}

// how segments are spread over buckets by k_seg_sort (seed_index.h)
static inline SegBkt seg_bkt_range() { SegBkt b; memset(&b, 0, sizeof b); b.mode = 0; return b; }
static inline SegBkt seg_bkt_key(uint32_t mask) {
    SegBkt b; memset(&b, 0, sizeof b);
    b.mode = 1; b.mask = mask; b.care = __builtin_popcount(mask);
    compress_masks(mask, b.mv);
    return b;
}
// n_seg segments of at most max_n entries each (larger ones, and those with a bucket beyond 256 entries, are listed in
// oversize[1 ..] for the caller's global pass; oversize[0] must be zero on entry)
static inline void launch_seg_sort(pba_ctx *ctx, const uint64_t *src, uint64_t *dst, const uint32_t *seg_off, const SegRef *segs,
                                   uint64_t n_seg, uint32_t max_n, const SegBkt &bk, uint32_t *oversize, uint32_t oversize_cap) {
    // (a launch's global size -- workgroups x threads -- is a 32-bit number: at most 2^21 segments of 1 024 threads, 2^23 of 256,
    // per launch; seg_off / segs are addressed from the launch's first segment, reports carry the global index)
    const bool small = max_n <= 256 * PBA_SS_EPT;
    const uint64_t per = small ? (1ull << 23) : (1ull << 21);
    for (uint64_t s0 = 0; s0 < n_seg; s0 += per) {
        const uint32_t g = (uint32_t)std::min<uint64_t>(n_seg - s0, per);
        if (small)
            hipLaunchKernelGGL(k_seg_sort<256>, dim3(g), dim3(256), 0, ctx->stream, src, dst, seg_off ? seg_off + s0 : nullptr,
                               segs ? segs + s0 : nullptr, bk, oversize, oversize_cap, (uint32_t)s0);
        else
            hipLaunchKernelGGL(k_seg_sort<1024>, dim3(g), dim3(1024), 0, ctx->stream, src, dst, seg_off ? seg_off + s0 : nullptr,
                               segs ? segs + s0 : nullptr, bk, oversize, oversize_cap, (uint32_t)s0);
    }
}

// u32 words of scratch scan_inclusive wants for n values
static inline size_t scan_scratch_words(uint64_t n) { return (size_t)((n + PBA_SCAN_TILE - 1) / PBA_SCAN_TILE + 1); }
// In-place inclusive scan of a[0 .. n) on the ctx's stream (seed_index.h: k_scan_*): one workgroup up to PBA_SCAN_SMALL_MAX
// values, else tiles, their sums, and the carry-in added back.  scratch: scan_scratch_words(n) words.  shifted (nullable): see
// k_scan_small; true when it was written (else the caller copies).
static inline bool scan_inclusive(pba_ctx *ctx, uint32_t *a, uint64_t n, uint32_t *scratch, uint32_t *shifted = nullptr) {
    if (n && n <= PBA_SCAN_SMALL_MAX) {
        hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, ctx->stream, a, (uint32_t)n, shifted);
        return shifted != nullptr;
    }
    const uint32_t n_tiles = (uint32_t)((n + PBA_SCAN_TILE - 1) / PBA_SCAN_TILE);
    if (!n_tiles) return false;
    hipLaunchKernelGGL(k_scan_tiles, dim3(n_tiles), dim3(256), 0, ctx->stream, a, n, scratch);
    if (n_tiles > 1) {
        hipLaunchKernelGGL(k_scan_sums, dim3(1), dim3(1024), 0, ctx->stream, scratch, n_tiles);
        hipLaunchKernelGGL(k_scan_add, dim3(n_tiles), dim3(256), 0, ctx->stream, a, n, scratch);
    }
    return false;
}

// Where the paths of a call of trace_batch go: exactly one outlet, made by name.  Scripts reach the caller's host arrays; votes
// go into the boxes `vote` names (device), gated by overlap_min; runs and per-window counts into the bounded slots of `slots`
// (align_cigar.h: SlotsInto, device); alleles likewise, at the SEL sites `sites` names (align_alleles.h), gated by overlap_min.
// What the host must know of an outlet to size and launch its pass is said here.
struct TraceInto {
    enum Kind { SCRIPTS, VOTES, RUNS, WINDOWS, ALLELES } kind;
    uint8_t *ops; const uint64_t *ops_off; int32_t *nedit;
    VoteInto vote; int overlap_min;
    SlotsInto slots;
    AllelesInto sites;
    static TraceInto scripts(uint8_t *ops, const uint64_t *ops_off, int32_t *nedit) {
        TraceInto t{}; t.kind = SCRIPTS; t.ops = ops; t.ops_off = ops_off; t.nedit = nedit; return t;
    }
    static TraceInto votes(const VoteInto &v, int overlap_min) { TraceInto t{}; t.kind = VOTES; t.vote = v; t.overlap_min = overlap_min; return t; }
    static TraceInto runs(const SlotsInto &s) { TraceInto t{}; t.kind = RUNS; t.slots = s; return t; }
    static TraceInto windows(const SlotsInto &s) { TraceInto t{}; t.kind = WINDOWS; t.slots = s; return t; }
    static TraceInto alleles(const SlotsInto &s, const AllelesInto &a, int overlap_min) {
        TraceInto t{}; t.kind = ALLELES; t.slots = s; t.sites = a; t.overlap_min = overlap_min; return t;
    }
    // bytes of goal-first temporary a wavefront needs behind its parent bits (ops_max: the longest script of the batch)
    uint64_t tmp_bytes(uint64_t ops_max) const { return kind == SCRIPTS ? ops_max : (kind == RUNS ? slots.run_max * 4 : 0); }
    // the checkpoint form only (a pile-up's votes, runs, windows, alleles); the others take the streamed form under PBA_TRACE_STREAM
    bool ck_only() const { return kind == RUNS || kind == WINDOWS || kind == ALLELES || (kind == VOTES && vote.box_off); }
    // "<name> from the walk need the bit-vector kernel (band too wide)"; scripts have the row-sweep form and never say it
    const char *name() const { return kind == VOTES ? "votes" : (kind == RUNS ? "runs" : (kind == WINDOWS ? "windows" : (kind == ALLELES ? "alleles" : "scripts"))); }
};

// One row's alignment to re-run for its runs, its windows or its alleles: its pair, the batch it goes with (0: strand +1,
// 1: strand -1), the PBA_CIG_* flags that put it in the target's forward order, what the row says of it.  not_held: the pair
// is not the walk that found the row (a mapped row's voting roles, a = contig), so it is not held to the row's cost.
struct RowJob { pba_pair pr; uint64_t row; uint32_t flags; int batch; int32_t cost, matlen_a, matlen_b; int not_held; };

// ---- internal entry points that cross translation units
extern "C" {
// sort one oversize partition / candidate piece in global memory (pba_index.hip)
PBA_INTERNAL int sort_partition_global(pba_ctx *ctx, uint64_t *d_part, uint32_t n);
// an index build of at most n_upper entries takes tiles of 4 096 entries in its generic level kernels (pba_core.hip)
PBA_INTERNAL bool index_small_tiles(uint64_t n_upper);
// the paths of a batch to the outlet `into` names (pba_align.hip)
PBA_INTERNAL int trace_batch(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R,
                             int maxn, int maxm, int kernel, pba_result *out, const TraceInto &into);
// The re-run jobs of overlap / mapped rows, in row order, after the checks both the CIGAR and the window entry points make of
// their sets and rows (who: the public function's name); counts / res (nullable, n entries): zeroed, res rc = -1 (pba_cigar.hip)
PBA_INTERNAL int overlap_rows_jobs(pba_ctx *ctx, const char *who, const pba_seqs *reads, const pba_seqs *reads_rc,
                                   const pba_strand_overlap *rows, uint64_t n, double R, pba_aln_counts *counts, pba_result *res,
                                   std::vector<RowJob> *jobs);
PBA_INTERNAL int map_rows_jobs(pba_ctx *ctx, const char *who, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                               const pba_map_row *rows, uint64_t n, double R, pba_aln_counts *counts, pba_result *res,
                               std::vector<RowJob> *jobs);
// ... and of mapped rows in their VOTING roles (pba_map_row_pair: a = contig), marked not_held (pba_cigar.hip)
PBA_INTERNAL int map_rows_vote_jobs(pba_ctx *ctx, const char *who, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                                    const pba_map_row *rows, uint64_t n, double R, pba_aln_counts *counts, pba_result *res,
                                    std::vector<RowJob> *jobs);
// one locked round over a subset of the reads (pba_drivers.hip)
PBA_INTERNAL int spaced_round_subset(pba_ctx *ctx, const pba_index *ix, const pba_seqs *ref, uint32_t ref_seq, const pba_seqs *reads,
                                     double R, int max_trial, int overlap_min, int buggy_seed_at, int kernel,
                                     const uint32_t *subset, uint32_t n_subset, pba_ss_row *rows, int ref_org = 0, int maxn = 0,
                                     int maxm = 0, uint8_t *touch = nullptr);
// the body of pba_locate with the bases of its `read` / `nseq` columns and an event its launches wait for (pba_drivers.hip)
PBA_INTERNAL int locate_core(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, uint32_t target_seq, const pba_seqs *reads,
                             double R, int trials, int min_len, int maxn, int maxm, int kernel, pba_loc_row *rows,
                             pba_loc_stats *stats, int64_t read_base, int64_t nseq_base, hipEvent_t packed);
// what pba_seqs_destroy does to a set it owns, whoever owns this one: a stream frees its slots' sets with it (pba_core.hip)
PBA_INTERNAL void seqs_free(pba_seqs *s);
// k_make_planes over a set's first `words` plane words on `stream`: the arrays of `s` are on the device (pba_core.hip)
PBA_INTERNAL int planes_enqueue(pba_ctx *ctx, const pba_seqs *s, uint64_t words, hipStream_t stream);
// k_revcomp of `src` into `dst` on `stream`: dst has pba_seqs_from_text's layout of src's lengths (h_off[0 .. n] on the host,
// d_off[0 .. n] and d_len on the device); d_flip: device, nullable = every sequence.  Alignment padding is not written (pba_core.hip)
PBA_INTERNAL int revcomp_enqueue(pba_ctx *ctx, const pba_seqs *src, const pba_seqs *dst, const uint8_t *d_flip, hipStream_t stream);
// the body of pba_map_reads with the bases of its `read` / `nseq` columns and an event both walks wait for (pba_drivers.hip)
PBA_INTERNAL int map_core(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                          double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands, pba_map_row *rows,
                          pba_map_stats *stats, int64_t read_base, int64_t nseq_base, hipEvent_t packed);
// the shared tail of the text makers: d_text / d_toff on the device, h_toff the same n + 1 offsets on the host; strict: a byte
// outside ACGT is PBA_E_ALPHABET (pba_core.hip).  pba_seqs_from_fastx hands its gathered text to it (pba_fastx.hip).
PBA_INTERNAL int seqs_pack(pba_ctx *ctx, const uint8_t *d_text, const uint64_t *d_toff, const uint64_t *h_toff, uint32_t n,
                           int strict, pba_seqs **out);
// a pba_qual of n sequences under the offsets h_off[0 .. n] from four device arrays (qv u8, depth u16, agree u16, src u32) that
// become its own; they are freed where it fails (pba_qual.hip).  The write passes of pba_pileup.hip fill them.
PBA_INTERNAL int qual_adopt(pba_ctx *ctx, uint32_t n, const uint64_t *h_off, void *arr[4], pba_qual **out);
// pba_map_reads' checks of its index and target (pba_drivers.hip)
PBA_INTERNAL int map_target_ok(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target);
// a live pile-up as the site scan reads it; a spent one is PBA_E_INVALID under who's name (pba_pileup.hip).  Spent is its ONLY
// failure: correct_vote (pba_pile_drivers.hip) asks it whether a pile-up is spent, so another reason to fail needs another call
struct PileView { ConsDev C; const unsigned long long *d_box_off; const uint64_t *box_off; uint32_t t_lo, t_hi, n_reads; int weight; uint64_t n_boxes; };
PBA_INTERNAL int pile_view(pba_ctx *ctx, const char *who, const pba_pileup *p, PileView *v);
// What the drivers of pba_pile_drivers.hip take from a pile-up (pba_pileup.hip).  A pile-up holds fewer boxes than kPileMaxBoxes.
// PileText: a pile-up evolved to one contiguous device text, target k at text[off[k] .. off[k+1]); d_off: off on the device
// (nt + 1 u64).  qmax >= 0: evolve also writes the evidence of every character (qual.h), one entry per text byte.
static const uint64_t kPileMaxBoxes = (1ull << 31) - 65536;
struct PileText {
    DevBuf text, d_off;
    std::vector<uint64_t> off;
    int qmax = -1;
    DevBuf qv, depth, agree, src;
};
// evolve to *T (and the rows of rows_out, where given); the boxes are released
PBA_INTERNAL int pile_evolve_text(pba_ctx *ctx, pba_pileup *p, PileText *T, pba_correct_row *rows_out);
// the evidence arrays of T into a pba_qual of its nt sequences (they leave T)
PBA_INTERNAL int pile_text_qual(pba_ctx *ctx, PileText &T, uint32_t nt, pba_qual **qual);
}  // extern "C"

#endif
