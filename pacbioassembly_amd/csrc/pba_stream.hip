// pba_stream.hip -- streamed locate and streamed mapping (include/pba.h: pba_loc_stream, pba_map_stream): two slots of reused
// storage, a copy stream of its own, a one-pass pack.  While the walk of batch k runs on the ctx's stream, batch k+1 is copied
// from pinned memory and packed on the copy stream -- for a pba_map_stream with strands & 2 on both strands.  Nothing is
// allocated or freed between create and destroy.  DESIGN.md 4.7, 4.9.
#include "pba_host.h"
#include "pba_internal.h"

// ---------------------------------------------------------------------------------------------
// kernel: ASCII -> packed arena and bit planes in one pass
// ---------------------------------------------------------------------------------------------
// A thread owns 32 bases of one sequence: 32 bytes of text (two 16-byte loads), two packed dwords, one pair of plane words.
// A work item is one wavefront over PBA_PP_BASES (seq_layout.h) consecutive bases of one sequence; item[s] = work items of the sequences before s
// (host prefix, copied with the offsets), so the sequence of an item is found once per wavefront, on wave-uniform values
// (k_pack_text / k_make_planes bisect once per dword).  The last work item zeroes the slack behind the last sequence.
// The slot is reused: every dword of the used extent is written -- alignment padding and pad bits as zero, plane bits
// masked at the sequence's length -- so that nothing of an earlier batch stays where a sweep can read it.
// RC = true writes rc(s) in the same layout (what pba_seqs_revcomp gives of the forward set) from the same text: the 32 OUTPUT
// bases 32u .. 32u + 31 of a thread are the complements of text bytes L - 1 - 32u downwards, so its window ends at L - 32u
// and, in the sequence's last unit, begins before the sequence's first byte -- the bytes there fall under the masks.
template <bool RC>
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
        if (valid > 0) {
            if constexpr (RC) {            // (may begin up to 31 bytes before the sequence: the neighbour's text or the staging's front slack)
                const uint8_t *src = text + ((int64_t)text_off[s] + (int64_t)L - 32 - (int64_t)u * 32);
                uint32_t v[8];
                __builtin_memcpy(v, src, 16);
                __builtin_memcpy(v + 4, src + 16, 16);
#pragma unroll
                for (int j = 0; j < 8; ++j) w[j] = __builtin_bswap32(v[7 - j]);   // byte order reversed within and across the two loads
            } else {                       // (may run up to 31 bytes past the sequence: the neighbour's text or the staging slack)
                const uint8_t *src = text + text_off[s] + (uint64_t)u * 32;
                __builtin_memcpy(w, src, 16);
                __builtin_memcpy(w + 4, src + 16, 16);
            }
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
            const uint32_t code = ((t ^ t1) | (nz * 3u)) ^ (RC ? 0x03030303u : 0u);         // (RC: the complement is code ^ 3)
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
// host side: the slots, under both kinds of stream
// ---------------------------------------------------------------------------------------------
static const size_t kTextFront = 64;             // staging bytes in front of the text: k_pack_planes<true> begins up to 31 bytes early

struct StreamSlot {
    uint8_t *h_bytes;        // pinned: the caller's input bytes
    uint64_t *h_offs;        // pinned: the caller's offsets
    uint64_t *h_off, *h_poff;   // pinned: packed byte offset / plane word offset of every sequence
    uint64_t *h_roff;        // pinned: packed byte offset inside the rc arena (records form; the text form's is h_off)
    uint32_t *h_len, *h_item, *h_bad;
    uint8_t *d_text_alloc;   // staging of the ASCII (text form); d_text = d_text_alloc + kTextFront
    uint8_t *d_text;
    uint64_t *d_toff;
    uint32_t *d_item, *d_bad;
    pba_seqs *set;           // borrows the arena, the planes and off / len / poff of this slot
    pba_seqs *rc;            // rc(batch): its own arena, planes and off; len / poff are the forward set's
    hipEvent_t ev_begin, ev_h2d, ev_pack;
    uint32_t n;
    uint64_t n_bytes;
};

struct StreamCore {
    pba_ctx *ctx;
    const char *name;        // "pba_loc_stream" / "pba_map_stream": who a failure is reported as
    int form, min_len;
    bool rc;                 // a slot holds rc(batch) as well
    uint64_t slot_bytes, pk_cap, rc_cap, plane_cap;      // plane_cap: word pairs between the slacks
    uint32_t slot_reads;
    hipStream_t copy;
    hipStream_t stream;                          // the ctx's stream at create: the walks run on it, and on no other (on_stream)
    hipEvent_t ev_loc0, ev_loc1;                 // the walk(s) of a batch, on the ctx's stream
    bool have_loc1, spent;
    StreamSlot slot[2];
    int head, npend;
    int64_t read_base, nseq_base;
    pba_stream_profile prof;
};

struct pba_loc_stream {
    StreamCore c;
    const pba_index *ix;
    const pba_seqs *target;
    uint32_t target_seq;
    double R;
    int trials, maxn, maxm, kernel;
};

struct pba_map_stream {
    StreamCore c;
    const pba_index *ix;
    const pba_seqs *target;
    double R;
    int trials, maxn, maxm, kernel, strands;
};

static int core_fail(StreamCore &c, int st, const char *fn, const char *what) {
    char who[64];
    snprintf(who, sizeof who, "%s_%s", c.name, fn);
    return ctx_fail_as(c.ctx, st, who, what);
}

// submit, pending and collect with the ctx on another stream than at create: refused before anything is looked at or enqueued,
// and the object stays usable (the walks of a slot are ordered among themselves and against ev_loc0 / ev_loc1 on ONE stream)
static int on_stream(StreamCore &c, const char *fn) {
    if (c.ctx->stream == c.stream) return PBA_OK;
    return core_fail(c, PBA_E_INVALID, fn, "the ctx is on another stream than at create (pba_ctx_set_stream)");
}

// (legal whatever stream the ctx is on now: what was enqueued went to the copy stream and to the stream recorded at create)
static void core_free(StreamCore &c) {
    (void)hipSetDevice(c.ctx->device);
    if (c.copy) (void)hipStreamSynchronize(c.copy);
    (void)hipStreamSynchronize(c.stream);
    for (StreamSlot &sl : c.slot) {
        for (void *h : {(void *)sl.h_bytes, (void *)sl.h_offs, (void *)sl.h_off, (void *)sl.h_poff, (void *)sl.h_roff, (void *)sl.h_len,
                        (void *)sl.h_item, (void *)sl.h_bad})
            if (h) (void)hipHostFree(h);
        for (void *d : {(void *)sl.d_text_alloc, (void *)sl.d_toff, (void *)sl.d_item, (void *)sl.d_bad})
            if (d) (void)hipFree(d);
        if (sl.rc) sl.rc->d_len = nullptr, sl.rc->d_poff = nullptr;      // (len / poff belong to the forward set)
        seqs_free(sl.rc);
        seqs_free(sl.set);
        for (hipEvent_t e : {sl.ev_begin, sl.ev_h2d, sl.ev_pack})
            if (e) (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : {c.ev_loc0, c.ev_loc1})
        if (e) (void)hipEventDestroy(e);
    if (c.copy) (void)hipStreamDestroy(c.copy);
}

template <class T> static bool pinned(T **p, size_t count) {
    return hipHostMalloc((void **)p, std::max<size_t>(1, count) * sizeof(T), hipHostMallocDefault) == hipSuccess;
}
template <class T> static bool device(T **p, size_t count) {
    return hipMalloc((void **)p, std::max<size_t>(1, count) * sizeof(T)) == hipSuccess;
}

// a borrowed set over an arena of `arena` bytes and the slot's planes, both zeroed once (the slack in front of the arena and
// of the planes is never written again)
static pba_seqs *set_alloc(StreamCore &c, pba_seqs **at, size_t arena, size_t nr) {
    pba_seqs *q = seqs_new(c.ctx, c.slot_reads);      // (h_off / h_len of every batch stay within these nr entries)
    if (!q) return nullptr;
    *at = q;
    q->n = 0; q->borrowed = true;
    const size_t planes = (c.plane_cap + 2 * kPlaneSlack) * 2 * sizeof(uint32_t);
    if (!device(&q->d_alloc, arena) || !device(&q->d_planes, planes / sizeof(uint32_t)) || !device(&q->d_off, nr)) return nullptr;
    q->d_packed = q->d_alloc + kSlack;
    if (memset_big(q->d_alloc, 0, arena, c.copy) != hipSuccess || memset_big(q->d_planes, 0, planes, c.copy) != hipSuccess) return nullptr;
    return q;
}

static bool slot_alloc(StreamCore &c, StreamSlot &sl) {
    const size_t nr = (size_t)c.slot_reads + 1;      // (a records slot keeps kSlack more behind the record slack: core_submit zeroes both)
    const size_t arena = c.form == PBA_STREAM_RECORDS ? arena_bytes(ARENA_RECORDS, c.pk_cap) + kSlack : arena_bytes(ARENA_TEXT, c.pk_cap);
    const bool text = c.form == PBA_STREAM_TEXT;
    if (!pinned(&sl.h_bytes, c.slot_bytes) || !pinned(&sl.h_offs, std::max<size_t>(nr, 3)) || !pinned(&sl.h_off, nr) ||
        !pinned(&sl.h_poff, nr) || !pinned(&sl.h_len, nr) || !pinned(&sl.h_item, nr) || !pinned(&sl.h_bad, 1))
        return false;
    if (c.rc && !text && !pinned(&sl.h_roff, nr)) return false;
    if (text && (!device(&sl.d_text_alloc, kTextFront + c.slot_bytes + 64) || !device(&sl.d_toff, nr) || !device(&sl.d_item, nr))) return false;
    if (!device(&sl.d_bad, 1)) return false;
    pba_seqs *q = set_alloc(c, &sl.set, arena, nr);
    if (!q || !device(&q->d_len, nr) || !device(&q->d_poff, nr)) return false;
    if (c.rc) {
        pba_seqs *r = set_alloc(c, &sl.rc, arena_bytes(ARENA_TEXT, c.rc_cap), nr);
        if (!r) return false;
        r->d_len = q->d_len; r->d_poff = q->d_poff;
    }
    if (text) {
        if (hipMemsetAsync(sl.d_text_alloc, 0, kTextFront + c.slot_bytes + 64, c.copy) != hipSuccess) return false;
        sl.d_text = sl.d_text_alloc + kTextFront;
    }
    return hipEventCreate(&sl.ev_begin) == hipSuccess && hipEventCreate(&sl.ev_h2d) == hipSuccess &&
           hipEventCreate(&sl.ev_pack) == hipSuccess;
}

// what both creates do once their own checks are through; on failure the caller frees the core
static int core_create(StreamCore &c, pba_ctx *ctx, const char *name, int form, int min_len, bool rc, uint64_t slot_bytes,
                       uint32_t slot_reads) {
    c.ctx = ctx; c.stream = ctx->stream; c.name = name; c.form = form; c.min_len = min_len; c.rc = rc; c.slot_bytes = slot_bytes; c.slot_reads = slot_reads;
    const SlotCaps caps = slot_caps(form == PBA_STREAM_TEXT, slot_bytes, slot_reads, rc);
    c.pk_cap = caps.pk_cap; c.rc_cap = caps.rc_cap; c.plane_cap = caps.plane_cap;
    bool ok = hipStreamCreateWithFlags(&c.copy, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipEventCreate(&c.ev_loc0) == hipSuccess && hipEventCreate(&c.ev_loc1) == hipSuccess;
    ok = ok && slot_alloc(c, c.slot[0]) && slot_alloc(c, c.slot[1]);
    ok = ok && hipStreamSynchronize(c.copy) == hipSuccess;
    if (!ok) (void)hipGetLastError();
    return ok ? PBA_OK : PBA_E_NOMEM;
}

// the host half of a text batch: the text layout of seq_layout.h with the work-item prefix of k_pack_planes
static int plan_text(StreamCore &c, StreamSlot &sl, uint32_t n, uint64_t *pk_total, uint64_t *words, uint32_t *items) {
    if (n > c.slot_reads) return core_fail(c, PBA_E_TOOLONG, "submit", "more reads than slot_reads");
    const uint64_t *to = sl.h_offs;
    for (uint32_t i = 0; i < n; ++i)
        if (to[i + 1] < to[i]) return core_fail(c, PBA_E_INVALID, "submit", "offsets must be non-decreasing");
    if (to[n] > c.slot_bytes) return core_fail(c, PBA_E_TOOLONG, "submit", "more bytes than slot_bytes");
    for (uint32_t i = 0; i < n; ++i) {
        const uint64_t L = to[i + 1] - to[i];
        if (L > (uint64_t)kMaxSeqLen) return core_fail(c, PBA_E_TOOLONG, "submit", "read longer than the engine limit");
        sl.h_len[i] = (uint32_t)L;
    }
    sl.h_len[n] = 0;
    const SeqTotals t = seq_layout(sl.h_len, n, sl.h_off, sl.h_poff, sl.h_item);
    sl.set->max_len = t.max_len;
    *pk_total = t.packed; *words = t.words; *items = (uint32_t)t.items;
    return PBA_OK;
}

// ... of a binary read file: pba_seqs_from_records' walk; the file is the arena (rc: the text layout of the same lengths beside it)
static int plan_records(StreamCore &c, StreamSlot &sl, uint32_t *n_out, uint64_t *pk_total, uint64_t *rc_total, uint64_t *words) {
    const uint64_t file_len = sl.h_offs[0];
    if (file_len > c.slot_bytes) return core_fail(c, PBA_E_TOOLONG, "submit", "more bytes than slot_bytes");
    const uint32_t min_excl = (uint32_t)sl.h_offs[1], max_excl = (uint32_t)sl.h_offs[2];
    const size_t kept = pba_open_binary(sl.h_bytes, file_len, min_excl, max_excl, sl.h_off, c.slot_reads, nullptr);
    if (kept > c.slot_reads) return core_fail(c, PBA_E_TOOLONG, "submit", "more reads than slot_reads");
    for (size_t i = 0; i < kept; ++i) {
        const uint64_t rec = sl.h_off[i];
        uint32_t L;
        memcpy(&L, sl.h_bytes + rec, 4);
        if (rec + 4 + ((uint64_t)L + 3) / 4 > file_len) return core_fail(c, PBA_E_INVALID, "submit", "truncated record");
        if (L > (uint32_t)kMaxSeqLen) return core_fail(c, PBA_E_TOOLONG, "submit", "read longer than the engine limit");
        sl.h_off[i] = rec + 4; sl.h_len[i] = L;      // payload follows the u32 length (dna_seq.h:119-121)
    }
    sl.h_off[kept] = file_len; sl.h_len[kept] = 0;
    const SeqTotals t = seq_layout(sl.h_len, kept, c.rc ? sl.h_roff : nullptr, sl.h_poff, nullptr);
    sl.set->max_len = t.max_len;
    *n_out = (uint32_t)kept; *pk_total = file_len; *rc_total = t.packed; *words = t.words;
    return PBA_OK;
}

static int spend(StreamCore &c, int st) { c.spent = true; return st; }

static int core_buffer(StreamCore &c, void **bytes, uint64_t **offsets) {
    if (c.spent || !bytes || !offsets || c.npend >= 2) return PBA_E_INVALID;
    StreamSlot &sl = c.slot[(c.head + c.npend) & 1];
    *bytes = sl.h_bytes;
    *offsets = sl.h_offs;
    return PBA_OK;
}

static int core_submit(StreamCore &c, uint32_t n) {
    if (c.spent || c.npend >= 2) return PBA_E_INVALID;
    PBA_TRY(on_stream(c, "submit"));
    pba_ctx *ctx = c.ctx;
    StreamSlot &sl = c.slot[(c.head + c.npend) & 1];
    pba_seqs *q = sl.set, *r = sl.rc;
    uint64_t pk_total = 0, rc_total = 0, words = 0;
    uint32_t items = 0;
    const bool text = c.form == PBA_STREAM_TEXT;
    PBA_TRY(text ? plan_text(c, sl, n, &pk_total, &words, &items) : plan_records(c, sl, &n, &pk_total, &rc_total, &words));
    if (text) rc_total = pk_total;
    const uint64_t *h_roff = text ? sl.h_off : sl.h_roff;
    // from here on the batch is accepted: a failure is the runtime's and spends the stream
    q->n = n; q->packed_bytes = pk_total; q->non_acgt = false; q->plane_words = words + 2 * kPlaneSlack;
    q->h_off.assign(sl.h_off, sl.h_off + n + 1);       // (within the capacity reserved at creation)
    q->h_len.assign(sl.h_len, sl.h_len + n + 1);
    if (r) {
        r->n = n; r->max_len = q->max_len; r->packed_bytes = rc_total; r->non_acgt = false; r->plane_words = q->plane_words;
        r->h_off.assign(h_roff, h_roff + n + 1);
        r->h_len.assign(sl.h_len, sl.h_len + n + 1);
    }
    sl.n = n; sl.n_bytes = text ? sl.h_offs[n] : pk_total;
    *sl.h_bad = 0;
    const size_t n1 = (size_t)n + 1;
    uint32_t *plane0 = q->d_planes + 2 * kPlaneSlack, *rplane0 = r ? r->d_planes + 2 * kPlaneSlack : nullptr;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipEventRecord(sl.ev_begin, c.copy);
    if (e == hipSuccess && sl.n_bytes) e = hipMemcpyAsync(text ? sl.d_text : q->d_packed, sl.h_bytes, sl.n_bytes, hipMemcpyHostToDevice, c.copy);
    if (e == hipSuccess) e = hipEventRecord(sl.ev_h2d, c.copy);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_off, sl.h_off, sizeof(uint64_t) * n1, hipMemcpyHostToDevice, c.copy);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_poff, sl.h_poff, sizeof(uint64_t) * n1, hipMemcpyHostToDevice, c.copy);
    if (e == hipSuccess) e = hipMemcpyAsync(q->d_len, sl.h_len, sizeof(uint32_t) * n1, hipMemcpyHostToDevice, c.copy);
    if (e == hipSuccess && r) e = hipMemcpyAsync(r->d_off, h_roff, sizeof(uint64_t) * n1, hipMemcpyHostToDevice, c.copy);
    if (e == hipSuccess && text) {
        e = hipMemcpyAsync(sl.d_toff, sl.h_offs, sizeof(uint64_t) * n1, hipMemcpyHostToDevice, c.copy);
        if (e == hipSuccess) e = hipMemcpyAsync(sl.d_item, sl.h_item, sizeof(uint32_t) * n1, hipMemcpyHostToDevice, c.copy);
        if (e == hipSuccess) e = hipMemsetAsync(sl.d_bad, 0, sizeof(uint32_t), c.copy);
        const dim3 grid(elem_grid(((uint64_t)items + 1) * PBA_WAVE, 256));
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_pack_planes<false>, grid, dim3(256), 0, c.copy, sl.d_text, sl.d_toff, q->d_off, q->d_poff, q->d_len,
                               sl.d_item, n, items, pk_total, words, q->d_packed, plane0, sl.d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess && r) {        // rc(batch) from the same staged text, into the slot's second arena and planes
            hipLaunchKernelGGL(k_pack_planes<true>, grid, dim3(256), 0, c.copy, sl.d_text, sl.d_toff, r->d_off, q->d_poff, q->d_len,
                               sl.d_item, n, items, pk_total, words, r->d_packed, rplane0, sl.d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(sl.h_bad, sl.d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, c.copy);
    } else if (e == hipSuccess) {          // the file is the packed arena: zero behind it, planes by k_make_planes, zero behind them
        e = hipMemsetAsync(q->d_packed + pk_total, 0, kRecordSlack + kSlack, c.copy);
        if (e == hipSuccess && planes_enqueue(ctx, q, words, c.copy) != PBA_OK) return spend(c, PBA_E_HIP);
        if (e == hipSuccess) e = hipMemsetAsync(plane0 + 2 * words, 0, kPlaneSlack * 2 * sizeof(uint32_t), c.copy);
        if (e == hipSuccess && r) {        // rc(batch) by k_revcomp from the file's records (it skips the alignment padding: zero first)
            e = hipMemsetAsync(r->d_packed, 0, rc_total + kSlack, c.copy);
            if (e == hipSuccess && (revcomp_enqueue(ctx, q, r, nullptr, c.copy) != PBA_OK || planes_enqueue(ctx, r, words, c.copy) != PBA_OK))
                return spend(c, PBA_E_HIP);
            if (e == hipSuccess) e = hipMemsetAsync(rplane0 + 2 * words, 0, kPlaneSlack * 2 * sizeof(uint32_t), c.copy);
        }
    }
    if (e == hipSuccess) e = hipEventRecord(sl.ev_pack, c.copy);
    if (e != hipSuccess) return spend(c, core_fail(c, PBA_E_HIP, "submit", hipGetErrorString(e)));
    ++c.npend;
    return PBA_OK;
}

// the oldest pending slot once its packs are through, the verdict of the pack on both of its sets
static int core_pending(StreamCore &c, StreamSlot **out) {
    if (c.spent || c.npend == 0) return PBA_E_INVALID;
    PBA_TRY(on_stream(c, "pending"));
    StreamSlot &sl = c.slot[c.head];
    const hipError_t e = hipEventSynchronize(sl.ev_pack);
    if (e != hipSuccess) return spend(c, core_fail(c, PBA_E_HIP, "pending", hipGetErrorString(e)));
    sl.set->non_acgt = *sl.h_bad != 0;     // (the aligning entry points refuse such a set, as they do a resident one)
    if (sl.rc) sl.rc->non_acgt = sl.set->non_acgt;
    *out = &sl;
    return PBA_OK;
}

// The collect of both kinds: the checks, the wait for the pack, the dropped batch, the profile and the running ids around
// walk(slot, read_base, nseq_base) -- the driver of the stream's kind on the ctx's stream behind slot.ev_pack.
template <class Walk>
static int core_collect(StreamCore &c, bool have_rows, uint32_t cap, uint32_t *n, Walk walk) {
    if (c.spent || !n || c.npend == 0) return PBA_E_INVALID;
    PBA_TRY(on_stream(c, "collect"));
    pba_ctx *ctx = c.ctx;
    StreamSlot &sl = c.slot[c.head];
    if (cap < sl.n || (!have_rows && sl.n)) return core_fail(c, PBA_E_INVALID, "collect", "cap below the batch size");
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipEventSynchronize(sl.ev_pack);      // the flag of the pack is read before anything is launched
    if (e != hipSuccess) return spend(c, core_fail(c, PBA_E_HIP, "collect", hipGetErrorString(e)));
    pba_stream_profile pr;
    memset(&pr, 0, sizeof pr);
    pr.n_reads = sl.n; pr.n_bytes = sl.n_bytes;
    (void)hipEventElapsedTime(&pr.h2d_ms, sl.ev_begin, sl.ev_h2d);
    (void)hipEventElapsedTime(&pr.pack_ms, sl.ev_h2d, sl.ev_pack);
    // what of the upload was NOT hidden: the ctx's stream had nothing to do from the end of the walk before (or, with none
    // since this batch was submitted, from the submit) until the pack was through
    float exposed = 0.f, since_loc = 0.f;
    (void)hipEventElapsedTime(&exposed, sl.ev_begin, sl.ev_pack);
    if (c.have_loc1 && hipEventElapsedTime(&since_loc, c.ev_loc1, sl.ev_pack) == hipSuccess) exposed = std::min(exposed, since_loc);
    (void)hipGetLastError();
    pr.stall_ms = std::max(0.f, exposed);
    *n = sl.n;
    int64_t kept = 0;
    for (uint32_t r = 0; r < sl.n; ++r) kept += (int)sl.h_len[r] >= c.min_len;
    if (*sl.h_bad) {                       // dropped: its reads still take their ids
        c.nseq_base += kept;
        c.read_base += sl.n;
        c.head ^= 1; --c.npend;
        c.prof = pr;
        return core_fail(c, PBA_E_ALPHABET, "collect", "the batch holds bytes outside ACGT");
    }
    (void)hipEventRecord(c.ev_loc0, ctx->stream);
    const int rc = walk(sl, c.read_base, c.nseq_base);
    if (rc != PBA_OK) return spend(c, rc);
    e = hipEventRecord(c.ev_loc1, ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(c.ev_loc1);       // (the walk ended in a synchronise: nothing reads the slot any more)
    if (e != hipSuccess) return spend(c, core_fail(c, PBA_E_HIP, "collect", hipGetErrorString(e)));
    c.have_loc1 = true;
    (void)hipEventElapsedTime(&pr.locate_ms, c.ev_loc0, c.ev_loc1);
    c.read_base += sl.n;
    c.nseq_base += kept;
    c.head ^= 1; --c.npend;
    c.prof = pr;
    return PBA_OK;
}

// what both creates refuse about the slot
static int slot_ok(pba_ctx *ctx, const char *who, uint64_t slot_bytes, uint32_t slot_reads, int form) {
    if (form != PBA_STREAM_TEXT && form != PBA_STREAM_RECORDS) return ctx_fail_as(ctx, PBA_E_INVALID, who, "unknown form");
    // work items and plane words of a batch are 32-bit counts in the kernel's prefix
    if (slot_bytes / 8 + slot_reads >= (1ull << 31)) return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "slot too large");
    return PBA_OK;
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// host API: streamed locate
// ---------------------------------------------------------------------------------------------
int pba_loc_stream_create(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, uint32_t target_seq, double R, int trials,
                          int min_len, int maxn, int maxm, int kernel, uint64_t slot_bytes, uint32_t slot_reads, int form,
                          pba_loc_stream **out) {
    if (!ctx || !ix || !target || !out || target_seq >= target->n || trials < 0) return PBA_E_INVALID;
    *out = nullptr;
    if (ix->mode != PBA_INDEX_ALL || ix->seq_len != target->h_len[target_seq])      // pba_locate's own checks, at the door
        PBA_FAIL(PBA_E_INVALID, "pba_locate needs a PBA_INDEX_ALL index of the target sequence");
    if (target->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_locate: a sequence set holds bytes outside ACGT");
    Plan pl;
    PBA_TRY(make_plan(ctx, R, maxn, maxm, kernel, 1, &pl));
    PBA_TRY(slot_ok(ctx, "pba_loc_stream_create", slot_bytes, slot_reads, form));
    HIPCHK(hipSetDevice(ctx->device));
    pba_loc_stream *s = new (std::nothrow) pba_loc_stream();
    if (!s) PBA_FAIL(PBA_E_NOMEM, "pba_loc_stream");
    s->ix = ix; s->target = target; s->target_seq = target_seq; s->R = R; s->trials = trials; s->maxn = maxn; s->maxm = maxm;
    s->kernel = kernel;
    if (core_create(s->c, ctx, "pba_loc_stream", form, min_len, false, slot_bytes, slot_reads) != PBA_OK) {
        core_free(s->c);
        delete s;
        PBA_FAIL(PBA_E_NOMEM, "pba_loc_stream_create");
    }
    *out = s;
    return PBA_OK;
}

int pba_loc_stream_buffer(pba_loc_stream *s, void **bytes, uint64_t **offsets) {
    return s ? core_buffer(s->c, bytes, offsets) : PBA_E_INVALID;
}

int pba_loc_stream_submit(pba_loc_stream *s, uint32_t n) { return s ? core_submit(s->c, n) : PBA_E_INVALID; }

int pba_loc_stream_pending(pba_loc_stream *s, const pba_seqs **set) {
    if (!s || !set) return PBA_E_INVALID;
    StreamSlot *sl = nullptr;
    PBA_TRY(core_pending(s->c, &sl));
    *set = sl->set;
    return PBA_OK;
}

int pba_loc_stream_collect(pba_loc_stream *s, pba_loc_row *rows, uint32_t cap, uint32_t *n, pba_loc_stats *stats) {
    if (!s) return PBA_E_INVALID;
    pba_loc_row none;
    pba_loc_stats st;
    PBA_TRY(core_collect(s->c, rows != nullptr, cap, n, [&](StreamSlot &sl, int64_t read_base, int64_t nseq_base) {
        return locate_core(s->c.ctx, s->ix, s->target, s->target_seq, sl.set, s->R, s->trials, s->c.min_len, s->maxn, s->maxm,
                           s->kernel, rows ? rows : &none, &st, read_base, nseq_base, sl.ev_pack);
    }));
    if (stats) *stats = st;
    return PBA_OK;
}

int pba_loc_stream_last_profile(const pba_loc_stream *s, pba_stream_profile *out) {
    if (!s || !out) return PBA_E_INVALID;
    *out = s->c.prof;
    return PBA_OK;
}

void pba_loc_stream_destroy(pba_loc_stream *s) {
    if (!s) return;
    core_free(s->c);
    delete s;
}

// ---------------------------------------------------------------------------------------------
// host API: streamed mapping
// ---------------------------------------------------------------------------------------------
int pba_map_stream_create(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, double R, int trials, int min_len, int maxn,
                          int maxm, int kernel, int strands, uint64_t slot_bytes, uint32_t slot_reads, int form,
                          pba_map_stream **out) {
    if (!ctx || !ix || !target || !out || trials < 0 || strands < 1 || strands > 3) return PBA_E_INVALID;
    *out = nullptr;
    PBA_TRY(map_target_ok(ctx, ix, target));                       // pba_map_reads' own checks, at the door
    if (target->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_map_reads: a sequence set holds bytes outside ACGT");
    Plan pl;
    PBA_TRY(make_plan(ctx, R, maxn, maxm, kernel, 1, &pl));
    PBA_TRY(slot_ok(ctx, "pba_map_stream_create", slot_bytes, slot_reads, form));
    HIPCHK(hipSetDevice(ctx->device));
    pba_map_stream *s = new (std::nothrow) pba_map_stream();
    if (!s) PBA_FAIL(PBA_E_NOMEM, "pba_map_stream");
    s->ix = ix; s->target = target; s->R = R; s->trials = trials; s->maxn = maxn; s->maxm = maxm; s->kernel = kernel;
    s->strands = strands;
    if (core_create(s->c, ctx, "pba_map_stream", form, min_len, (strands & 2) != 0, slot_bytes, slot_reads) != PBA_OK) {
        core_free(s->c);
        delete s;
        PBA_FAIL(PBA_E_NOMEM, "pba_map_stream_create");
    }
    *out = s;
    return PBA_OK;
}

int pba_map_stream_buffer(pba_map_stream *s, void **bytes, uint64_t **offsets) {
    return s ? core_buffer(s->c, bytes, offsets) : PBA_E_INVALID;
}

int pba_map_stream_submit(pba_map_stream *s, uint32_t n) { return s ? core_submit(s->c, n) : PBA_E_INVALID; }

int pba_map_stream_pending(pba_map_stream *s, const pba_seqs **fwd, const pba_seqs **rc) {
    if (!s || !fwd || !rc) return PBA_E_INVALID;
    StreamSlot *sl = nullptr;
    PBA_TRY(core_pending(s->c, &sl));
    *fwd = sl->set;
    *rc = sl->rc;
    return PBA_OK;
}

int pba_map_stream_collect(pba_map_stream *s, pba_map_row *rows, uint32_t cap, uint32_t *n, pba_map_stats *stats) {
    if (!s) return PBA_E_INVALID;
    pba_map_row none;
    pba_map_stats st;
    PBA_TRY(core_collect(s->c, rows != nullptr, cap, n, [&](StreamSlot &sl, int64_t read_base, int64_t nseq_base) {
        return map_core(s->c.ctx, s->ix, s->target, sl.set, sl.rc, s->R, s->trials, s->c.min_len, s->maxn, s->maxm, s->kernel,
                        s->strands, rows ? rows : &none, &st, read_base, nseq_base, sl.ev_pack);
    }));
    if (stats) *stats = st;
    return PBA_OK;
}

int pba_map_stream_last_profile(const pba_map_stream *s, pba_stream_profile *out) {
    if (!s || !out) return PBA_E_INVALID;
    *out = s->c.prof;
    return PBA_OK;
}

void pba_map_stream_destroy(pba_map_stream *s) {
    if (!s) return;
    core_free(s->c);
    delete s;
}

}  // extern "C"
