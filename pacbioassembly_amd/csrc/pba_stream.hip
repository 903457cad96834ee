// pba_stream.hip -- streamed locate (include/pba.h: pba_loc_stream): two slots of reused storage, a copy stream of its own,
// a one-pass pack.  While the locate of batch k runs on the ctx's stream, batch k+1 is copied from pinned memory and packed
// on the copy stream.  Nothing is allocated or freed between create and destroy.  DESIGN.md 4.7.
#include "pba_host.h"
#include "pba_internal.h"

// ---------------------------------------------------------------------------------------------
// kernel: ASCII -> packed arena and bit planes in one pass
// ---------------------------------------------------------------------------------------------
// A thread owns 32 bases of one sequence: 32 bytes of text (two 16-byte loads), two packed dwords, one pair of plane words.
// A work item is one wavefront over 2 048 consecutive bases of one sequence; item[s] = work items of the sequences before s
// (host prefix, copied with the offsets), so the sequence of an item is found once per wavefront, on wave-uniform values
// (k_pack_text / k_make_planes bisect once per dword).  The last work item zeroes the slack behind the last sequence.
// The slot is reused: every dword of the used extent is written -- alignment padding and pad bits as zero, plane bits
// masked at the sequence's length -- so that nothing of an earlier batch stays where a sweep can read it.
#define PBA_PP_BASES 2048          // bases per work item: 64 lanes x 32
__global__ void __launch_bounds__(256)
k_pack_planes(const uint8_t *__restrict__ text, const uint64_t *__restrict__ text_off, const uint64_t *__restrict__ pk_off,
              const uint64_t *__restrict__ poff, const uint32_t *__restrict__ len, const uint32_t *__restrict__ item, uint32_t n,
              uint32_t n_items, uint64_t pk_total, uint64_t plane_total, uint8_t *__restrict__ packed, uint32_t *__restrict__ plane,
              uint32_t *bad) {
    const uint32_t lane = threadIdx.x & (PBA_WAVE - 1);
    const uint32_t waves_per_block = blockDim.x / PBA_WAVE;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * waves_per_block + threadIdx.x / PBA_WAVE));
    // (grid-stride over the work items: a launch's global size is a 32-bit number, see elem_grid)
    for (uint32_t it = wave0; it <= n_items; it += gridDim.x * waves_per_block) {
        if (it == n_items) {               // the slack behind the last sequence: kSlack bytes, kPlaneSlack word pairs
            *reinterpret_cast<uint4 *>(packed + pk_total + 16 * lane) = make_uint4(0, 0, 0, 0);
            *reinterpret_cast<uint2 *>(plane + 2 * (plane_total + lane)) = make_uint2(0, 0);
            continue;
        }
        uint32_t lo = 0, hi = n;           // last s with item[s] <= it (empty sequences own no item)
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (item[mid] <= it) lo = mid; else hi = mid;
        }
        const uint32_t s = lo;
        const uint32_t L = len[s];
        const uint32_t u = (it - item[s]) * PBA_WAVE + lane;      // which 32 bases of the sequence
        const int64_t left = (int64_t)L - (int64_t)u * 32;                 // bases of the sequence from this thread's first on
        const int valid = left < 32 ? (int)left : 32;
        uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (valid > 0) {                   // (may run up to 31 bytes past the sequence: the neighbour's text or the staging slack)
            const uint8_t *src = text + text_off[s] + (uint64_t)u * 32;
            __builtin_memcpy(w, src, 16);
            __builtin_memcpy(w + 4, src + 16, 16);
        }
        // Four characters at a time, no branches.  x = ch ^ 'A' is 0x00 / 0x02 / 0x06 / 0x15 for A / C / G / T; t = bits 2:1 of x is
        // 0 / 1 / 3 / 2, so t ^ (t >> 1) is the code of C2I (dna_seq.h:21) on ACGT.  Any other byte differs from the x its own t
        // stands for: it takes code 3 and raises the flag.  The multiplies gather one field per byte into the top byte (the
        // partial products fall on distinct bits: no carries).
        uint32_t be[2] = {0, 0}, plo = 0, phi = 0, odd = 0;      // be: the packed stream, base 0 in bits 31:30 of be[0]
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t x = w[j] ^ 0x41414141u;
            const uint32_t t = (x >> 1) & 0x03030303u;
            const uint32_t t0 = t & 0x01010101u, t1 = (t >> 1) & 0x01010101u, tt = t1 & ~t0;
            const uint32_t d = x ^ ((t0 << 1) | ((t0 & t1) << 2) | (tt * 0x15u));          // non-zero bytes: not ACGT
            const uint32_t nz = ((((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) >> 7) & 0x01010101u;
            const uint32_t code = (t ^ t1) | (nz * 3u);
            be[j >> 2] |= ((code * 0x40100401u) & 0xFF000000u) >> (8 * (j & 3));             // byte = c0<<6 | c1<<4 | c2<<2 | c3
            plo |= (((code & 0x01010101u) * 0x01020408u) >> 24) << (4 * j);
            phi |= ((((code >> 1) & 0x01010101u) * 0x01020408u) >> 24) << (4 * j);
            odd |= ((nz * 0x01020408u) >> 24) << (4 * j);
        }
        if (valid < 32) {                  // nothing past the end: pad bits and padding are zero
            const uint32_t m = valid > 0 ? (1u << valid) - 1u : 0u;
            const uint64_t keep = valid > 0 ? ~(~0ull >> (2 * valid)) : 0ull;
            plo &= m; phi &= m; odd &= m;
            be[0] &= (uint32_t)(keep >> 32); be[1] &= (uint32_t)keep;
        }
        const uint32_t pk[2] = {__builtin_bswap32(be[0]), __builtin_bswap32(be[1])};         // first base in bits 7:6 of the first byte
        const uint32_t notacgt = odd;
        const uint32_t pk_units = 2 * ((L + 63) / 64), pl_units = (L + 31) / 32;            // 16-byte aligned arena, word-aligned planes
        if (u < pk_units) *reinterpret_cast<uint2 *>(packed + pk_off[s] + (uint64_t)u * 8) = make_uint2(pk[0], pk[1]);
        if (u < pl_units) *reinterpret_cast<uint2 *>(plane + 2 * (poff[s] + u)) = make_uint2(plo, phi);
        if (notacgt) atomicOr(bad, 1u);
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static const uint64_t kRecordSlack = 65536;      // zero bytes behind a binary read file (pba_seqs_from_records)

struct StreamSlot {
    uint8_t *h_bytes;        // pinned: the caller's input bytes
    uint64_t *h_offs;        // pinned: the caller's offsets
    uint64_t *h_off, *h_poff;   // pinned: packed byte offset / plane word offset of every sequence
    uint32_t *h_len, *h_item, *h_bad;
    uint8_t *d_text;         // staging of the ASCII (text form)
    uint64_t *d_toff;
    uint32_t *d_item, *d_bad;
    pba_seqs *set;           // borrows the arena, the planes and off / len / poff of this slot
    hipEvent_t ev_begin, ev_h2d, ev_pack;
    uint32_t n;
    uint64_t n_bytes;
};

struct pba_loc_stream {
    pba_ctx *ctx;
    const pba_index *ix;
    const pba_seqs *target;
    uint32_t target_seq;
    double R;
    int trials, min_len, maxn, maxm, kernel, form;
    uint64_t slot_bytes, pk_cap, plane_cap;      // plane_cap: word pairs between the slacks
    uint32_t slot_reads;
    hipStream_t copy;
    hipEvent_t ev_loc0, ev_loc1;                 // the locate of a batch, on the ctx's stream
    bool have_loc1, spent;
    StreamSlot slot[2];
    int head, npend;
    int64_t read_base, nseq_base;
    pba_stream_profile prof;
};

static void stream_free(pba_loc_stream *s) {
    (void)hipSetDevice(s->ctx->device);
    if (s->copy) (void)hipStreamSynchronize(s->copy);
    (void)hipStreamSynchronize(s->ctx->stream);
    for (StreamSlot &sl : s->slot) {
        for (void *h : {(void *)sl.h_bytes, (void *)sl.h_offs, (void *)sl.h_off, (void *)sl.h_poff, (void *)sl.h_len, (void *)sl.h_item,
                        (void *)sl.h_bad})
            if (h) (void)hipHostFree(h);
        for (void *d : {(void *)sl.d_text, (void *)sl.d_toff, (void *)sl.d_item, (void *)sl.d_bad})
            if (d) (void)hipFree(d);
        if (sl.set) {
            pba_seqs *q = sl.set;
            for (void *d : {(void *)q->d_alloc, (void *)q->d_planes, (void *)q->d_off, (void *)q->d_len, (void *)q->d_poff})
                if (d) (void)hipFree(d);
            delete q;
        }
        for (hipEvent_t e : {sl.ev_begin, sl.ev_h2d, sl.ev_pack})
            if (e) (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : {s->ev_loc0, s->ev_loc1})
        if (e) (void)hipEventDestroy(e);
    if (s->copy) (void)hipStreamDestroy(s->copy);
    delete s;
}

template <class T> static bool pinned(T **p, size_t count) {
    return hipHostMalloc((void **)p, std::max<size_t>(1, count) * sizeof(T), hipHostMallocDefault) == hipSuccess;
}
template <class T> static bool device(T **p, size_t count) {
    return hipMalloc((void **)p, std::max<size_t>(1, count) * sizeof(T)) == hipSuccess;
}

static bool slot_alloc(pba_loc_stream *s, StreamSlot &sl) {
    const size_t nr = (size_t)s->slot_reads + 1, trail = s->form == PBA_STREAM_RECORDS ? kRecordSlack + kSlack : kSlack;
    const bool text = s->form == PBA_STREAM_TEXT;
    if (!pinned(&sl.h_bytes, s->slot_bytes) || !pinned(&sl.h_offs, std::max<size_t>(nr, 3)) || !pinned(&sl.h_off, nr) ||
        !pinned(&sl.h_poff, nr) || !pinned(&sl.h_len, nr) || !pinned(&sl.h_item, nr) || !pinned(&sl.h_bad, 1))
        return false;
    if (text && (!device(&sl.d_text, s->slot_bytes + 64) || !device(&sl.d_toff, nr) || !device(&sl.d_item, nr))) return false;
    if (!device(&sl.d_bad, 1)) return false;
    pba_seqs *q = new (std::nothrow) pba_seqs();
    if (!q) return false;
    sl.set = q;
    q->ctx = s->ctx; q->borrowed = true;
    q->h_off.reserve(nr); q->h_len.reserve(nr);
    const size_t arena = kSlack + s->pk_cap + trail, planes = (s->plane_cap + 2 * kPlaneSlack) * 2 * sizeof(uint32_t);
    if (!device(&q->d_alloc, arena) || !device(&q->d_planes, planes / sizeof(uint32_t)) || !device(&q->d_off, nr) ||
        !device(&q->d_len, nr) || !device(&q->d_poff, nr))
        return false;
    q->d_packed = q->d_alloc + kSlack;
    // (the slack in front of the arena and of the planes is zeroed here, once, and never written again)
    if (memset_big(q->d_alloc, 0, arena, s->copy) != hipSuccess || memset_big(q->d_planes, 0, planes, s->copy) != hipSuccess) return false;
    if (text && hipMemsetAsync(sl.d_text, 0, s->slot_bytes + 64, s->copy) != hipSuccess) return false;
    return hipEventCreate(&sl.ev_begin) == hipSuccess && hipEventCreate(&sl.ev_h2d) == hipSuccess &&
           hipEventCreate(&sl.ev_pack) == hipSuccess;
}

// the host half of a text batch: layout of pba_seqs_from_text (seqs_pack) plus the work-item prefix of k_pack_planes
static int plan_text(pba_loc_stream *s, StreamSlot &sl, uint32_t n, uint64_t *pk_total, uint64_t *words, uint32_t *items) {
    pba_ctx *ctx = s->ctx;
    if (n > s->slot_reads) PBA_FAIL(PBA_E_TOOLONG, "pba_loc_stream_submit: more reads than slot_reads");
    const uint64_t *to = sl.h_offs;
    for (uint32_t i = 0; i < n; ++i)
        if (to[i + 1] < to[i]) PBA_FAIL(PBA_E_INVALID, "pba_loc_stream_submit: offsets must be non-decreasing");
    if (to[n] > s->slot_bytes) PBA_FAIL(PBA_E_TOOLONG, "pba_loc_stream_submit: more bytes than slot_bytes");
    uint64_t pk = 0, w = 0, it = 0;
    uint32_t max_len = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t L = to[i + 1] - to[i];
        if (L > (uint64_t)kMaxSeqLen) PBA_FAIL(PBA_E_TOOLONG, "pba_loc_stream_submit: read longer than the engine limit");
        sl.h_off[i] = pk; sl.h_poff[i] = w; sl.h_len[i] = (uint32_t)L; sl.h_item[i] = (uint32_t)it;
        max_len = std::max(max_len, (uint32_t)L);
        pk += ((L + 3) / 4 + 15) & ~15ull;
        w += (L + 31) / 32;
        it += (L + PBA_PP_BASES - 1) / PBA_PP_BASES;
    }
    sl.h_off[n] = pk; sl.h_poff[n] = w; sl.h_len[n] = 0; sl.h_item[n] = (uint32_t)it;
    sl.set->max_len = max_len;
    *pk_total = pk; *words = w; *items = (uint32_t)it;
    return PBA_OK;
}

// ... of a binary read file: pba_seqs_from_records' walk; the file is the arena
static int plan_records(pba_loc_stream *s, StreamSlot &sl, uint32_t *n_out, uint64_t *pk_total, uint64_t *words) {
    pba_ctx *ctx = s->ctx;
    const uint64_t file_len = sl.h_offs[0];
    if (file_len > s->slot_bytes) PBA_FAIL(PBA_E_TOOLONG, "pba_loc_stream_submit: more bytes than slot_bytes");
    const uint32_t min_excl = (uint32_t)sl.h_offs[1], max_excl = (uint32_t)sl.h_offs[2];
    const size_t kept = pba_open_binary(sl.h_bytes, file_len, min_excl, max_excl, sl.h_off, s->slot_reads, nullptr);
    if (kept > s->slot_reads) PBA_FAIL(PBA_E_TOOLONG, "pba_loc_stream_submit: more reads than slot_reads");
    uint64_t w = 0;
    uint32_t max_len = 0;
    for (size_t i = 0; i < kept; ++i) {
        const uint64_t rec = sl.h_off[i];
        uint32_t L;
        memcpy(&L, sl.h_bytes + rec, 4);
        if (rec + 4 + ((uint64_t)L + 3) / 4 > file_len) PBA_FAIL(PBA_E_INVALID, "pba_loc_stream_submit: truncated record");
        if (L > (uint32_t)kMaxSeqLen) PBA_FAIL(PBA_E_TOOLONG, "pba_loc_stream_submit: read longer than the engine limit");
        sl.h_off[i] = rec + 4; sl.h_poff[i] = w; sl.h_len[i] = L;      // payload follows the u32 length (dna_seq.h:119-121)
        max_len = std::max(max_len, L);
        w += ((uint64_t)L + 31) / 32;
    }
    sl.h_off[kept] = file_len; sl.h_poff[kept] = w; sl.h_len[kept] = 0;
    sl.set->max_len = max_len;
    *n_out = (uint32_t)kept; *pk_total = file_len; *words = w;
    return PBA_OK;
}

static int spend(pba_loc_stream *s, int st) { s->spent = true; return st; }

extern "C" {

int pba_loc_stream_create(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, uint32_t target_seq, double R, int trials,
                          int min_len, int maxn, int maxm, int kernel, uint64_t slot_bytes, uint32_t slot_reads, int form,
                          pba_loc_stream **out) {
    if (!ctx || !ix || !target || !out || target_seq >= target->n || trials < 0) return PBA_E_INVALID;
    *out = nullptr;
    if (form != PBA_STREAM_TEXT && form != PBA_STREAM_RECORDS) PBA_FAIL(PBA_E_INVALID, "pba_loc_stream_create: unknown form");
    if (ix->mode != PBA_INDEX_ALL || ix->seq_len != target->h_len[target_seq])      // pba_locate's own checks, at the door
        PBA_FAIL(PBA_E_INVALID, "pba_locate needs a PBA_INDEX_ALL index of the target sequence");
    if (target->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_locate: a sequence set holds bytes outside ACGT");
    Plan pl;
    PBA_TRY(make_plan(ctx, R, maxn, maxm, kernel, 1, &pl));
    // work items and plane words of a batch are 32-bit counts in the kernel's prefix
    if (slot_bytes / 8 + slot_reads >= (1ull << 31)) PBA_FAIL(PBA_E_TOOLONG, "pba_loc_stream_create: slot too large");
    HIPCHK(hipSetDevice(ctx->device));
    pba_loc_stream *s = new (std::nothrow) pba_loc_stream();
    if (!s) PBA_FAIL(PBA_E_NOMEM, "pba_loc_stream");
    s->ctx = ctx; s->ix = ix; s->target = target; s->target_seq = target_seq; s->R = R; s->trials = trials; s->min_len = min_len;
    s->maxn = maxn; s->maxm = maxm; s->kernel = kernel; s->form = form; s->slot_bytes = slot_bytes; s->slot_reads = slot_reads;
    if (form == PBA_STREAM_TEXT) {         // every read rounds up to 16 packed bytes and to one plane word
        s->pk_cap = ((slot_bytes + 3) / 4 + 16ull * slot_reads + 15) & ~15ull;
        s->plane_cap = slot_bytes / 32 + slot_reads + 1;
    } else {                               // the file is the arena; four bases per payload byte
        s->pk_cap = (slot_bytes + 15) & ~15ull;
        s->plane_cap = slot_bytes / 8 + slot_reads + 1;
    }
    bool ok = hipStreamCreateWithFlags(&s->copy, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreate(&s->ev_loc0) == hipSuccess && hipEventCreate(&s->ev_loc1) == hipSuccess;
    ok = ok && slot_alloc(s, s->slot[0]) && slot_alloc(s, s->slot[1]);
    ok = ok && hipStreamSynchronize(s->copy) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        stream_free(s);
        PBA_FAIL(PBA_E_NOMEM, "pba_loc_stream_create");
    }
    *out = s;
    return PBA_OK;
}

int pba_loc_stream_buffer(pba_loc_stream *s, void **bytes, uint64_t **offsets) {
    if (!s || s->spent || !bytes || !offsets || s->npend >= 2) return PBA_E_INVALID;
    StreamSlot &sl = s->slot[(s->head + s->npend) & 1];
    *bytes = sl.h_bytes;
    *offsets = sl.h_offs;
    return PBA_OK;
}

int pba_loc_stream_submit(pba_loc_stream *s, uint32_t n) {
    if (!s || s->spent || s->npend >= 2) return PBA_E_INVALID;
    pba_ctx *ctx = s->ctx;
    StreamSlot &sl = s->slot[(s->head + s->npend) & 1];
    pba_seqs *q = sl.set;
    uint64_t pk_total = 0, words = 0;
    uint32_t items = 0;
    const bool text = s->form == PBA_STREAM_TEXT;
    PBA_TRY(text ? plan_text(s, sl, n, &pk_total, &words, &items) : plan_records(s, sl, &n, &pk_total, &words));
    // from here on the batch is accepted: a failure is the runtime's and spends the stream
    q->n = n; q->packed_bytes = pk_total; q->non_acgt = false; q->plane_words = words + 2 * kPlaneSlack;
    q->h_off.assign(sl.h_off, sl.h_off + n + 1);       // (within the capacity reserved at creation)
    q->h_len.assign(sl.h_len, sl.h_len + n + 1);
    sl.n = n; sl.n_bytes = text ? sl.h_offs[n] : pk_total;
    *sl.h_bad = 0;
    const size_t n1 = (size_t)n + 1;
    uint32_t *plane0 = q->d_planes + 2 * kPlaneSlack;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipEventRecord(sl.ev_begin, s->copy);
    if (e == hipSuccess && sl.n_bytes) e = hipMemcpyAsync(text ? sl.d_text : q->d_packed, sl.h_bytes, sl.n_bytes, hipMemcpyHostToDevice, s->copy);
    if (e == hipSuccess) e = hipEventRecord(sl.ev_h2d, s->copy);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_off, sl.h_off, sizeof(uint64_t) * n1, hipMemcpyHostToDevice, s->copy);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_poff, sl.h_poff, sizeof(uint64_t) * n1, hipMemcpyHostToDevice, s->copy);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_len, sl.h_len, sizeof(uint32_t) * n1, hipMemcpyHostToDevice, s->copy);
    if (e == hipSuccess && text) {
        e = hipMemcpyAsync(sl.d_toff, sl.h_offs, sizeof(uint64_t) * n1, hipMemcpyHostToDevice, s->copy);
        if (e == hipSuccess) e = hipMemcpyAsync(sl.d_item, sl.h_item, sizeof(uint32_t) * n1, hipMemcpyHostToDevice, s->copy);
        if (e == hipSuccess) e = hipMemsetAsync(sl.d_bad, 0, sizeof(uint32_t), s->copy);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_pack_planes, dim3(elem_grid(((uint64_t)items + 1) * PBA_WAVE, 256)), dim3(256), 0, s->copy, sl.d_text,
                               sl.d_toff, q->d_off, q->d_poff, q->d_len, sl.d_item, n, items, pk_total, words, q->d_packed, plane0, sl.d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(sl.h_bad, sl.d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, s->copy);
    } else if (e == hipSuccess) {          // the file is the packed arena: zero behind it, planes by k_make_planes, zero behind them
        e = hipMemsetAsync(q->d_packed + pk_total, 0, kRecordSlack + kSlack, s->copy);
        if (e == hipSuccess && planes_enqueue(ctx, q, words, s->copy) != PBA_OK) return spend(s, PBA_E_HIP);
        if (e == hipSuccess) e = hipMemsetAsync(plane0 + 2 * words, 0, kPlaneSlack * 2 * sizeof(uint32_t), s->copy);
    }
    if (e == hipSuccess) e = hipEventRecord(sl.ev_pack, s->copy);
    if (e != hipSuccess) return spend(s, ctx_fail(ctx, PBA_E_HIP, "pba_loc_stream_submit", e));
    ++s->npend;
    return PBA_OK;
}

int pba_loc_stream_pending(pba_loc_stream *s, const pba_seqs **set) {
    if (!s || s->spent || !set || s->npend == 0) return PBA_E_INVALID;
    pba_ctx *ctx = s->ctx;
    StreamSlot &sl = s->slot[s->head];
    const hipError_t e = hipEventSynchronize(sl.ev_pack);
    if (e != hipSuccess) return spend(s, ctx_fail(ctx, PBA_E_HIP, "pba_loc_stream_pending", e));
    sl.set->non_acgt = *sl.h_bad != 0;     // (the aligning entry points refuse such a set, as they do a resident one)
    *set = sl.set;
    return PBA_OK;
}

int pba_loc_stream_collect(pba_loc_stream *s, pba_loc_row *rows, uint32_t cap, uint32_t *n, pba_loc_stats *stats) {
    if (!s || s->spent || !n || s->npend == 0) return PBA_E_INVALID;
    pba_ctx *ctx = s->ctx;
    StreamSlot &sl = s->slot[s->head];
    if (cap < sl.n || (!rows && sl.n)) PBA_FAIL(PBA_E_INVALID, "pba_loc_stream_collect: cap below the batch size");
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipEventSynchronize(sl.ev_pack);      // the flag of the pack is read before anything is launched
    if (e != hipSuccess) return spend(s, ctx_fail(ctx, PBA_E_HIP, "pba_loc_stream_collect", e));
    pba_stream_profile pr;
    memset(&pr, 0, sizeof pr);
    pr.n_reads = sl.n; pr.n_bytes = sl.n_bytes;
    (void)hipEventElapsedTime(&pr.h2d_ms, sl.ev_begin, sl.ev_h2d);
    (void)hipEventElapsedTime(&pr.pack_ms, sl.ev_h2d, sl.ev_pack);
    // what of the upload was NOT hidden: the ctx's stream had nothing to do from the end of the locate before (or, with none
    // since this batch was submitted, from the submit) until the pack was through
    float exposed = 0.f, since_loc = 0.f;
    (void)hipEventElapsedTime(&exposed, sl.ev_begin, sl.ev_pack);
    if (s->have_loc1 && hipEventElapsedTime(&since_loc, s->ev_loc1, sl.ev_pack) == hipSuccess) exposed = std::min(exposed, since_loc);
    (void)hipGetLastError();
    pr.stall_ms = std::max(0.f, exposed);
    *n = sl.n;
    if (*sl.h_bad) {                       // dropped: its reads still take their ids
        for (uint32_t r = 0; r < sl.n; ++r) s->nseq_base += (int)sl.h_len[r] >= s->min_len;
        s->read_base += sl.n;
        s->head ^= 1; --s->npend;
        s->prof = pr;
        PBA_FAIL(PBA_E_ALPHABET, "pba_loc_stream_collect: the batch holds bytes outside ACGT");
    }
    pba_loc_row none;
    pba_loc_stats st;
    (void)hipEventRecord(s->ev_loc0, ctx->stream);
    const int rc = locate_core(ctx, s->ix, s->target, s->target_seq, sl.set, s->R, s->trials, s->min_len, s->maxn, s->maxm,
                               s->kernel, rows ? rows : &none, &st, s->read_base, s->nseq_base, sl.ev_pack);
    if (rc != PBA_OK) return spend(s, rc);
    e = hipEventRecord(s->ev_loc1, ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(s->ev_loc1);      // (the locate ended in a synchronise: nothing reads the slot any more)
    if (e != hipSuccess) return spend(s, ctx_fail(ctx, PBA_E_HIP, "pba_loc_stream_collect", e));
    s->have_loc1 = true;
    (void)hipEventElapsedTime(&pr.locate_ms, s->ev_loc0, s->ev_loc1);
    s->read_base += sl.n;
    s->nseq_base += st.n_reads_kept;
    s->head ^= 1; --s->npend;
    s->prof = pr;
    if (stats) *stats = st;
    return PBA_OK;
}

int pba_loc_stream_last_profile(const pba_loc_stream *s, pba_stream_profile *out) {
    if (!s || !out) return PBA_E_INVALID;
    *out = s->prof;
    return PBA_OK;
}

void pba_loc_stream_destroy(pba_loc_stream *s) {
    if (s) stream_free(s);
}

}  // extern "C"
