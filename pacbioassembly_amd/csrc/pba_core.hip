// pba_core.hip -- context and sequence sets: kernels and the device half of the C ABI (include/pba.h).
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
#include "pba_host.h"
#include "pba_internal.h"

// ---------------------------------------------------------------------------------------------
// kernels: packing
// ---------------------------------------------------------------------------------------------
// ASCII -> 2-bit, 16 chars per thread into one packed dword.  Thread t owns packed dword t of the
// whole set; its sequence is found by bisection over the (16-byte aligned) packed offsets.
__global__ void __launch_bounds__(256)
k_pack_text(const uint8_t *text, const uint64_t *text_off, const uint64_t *pk_off, const uint32_t *len, uint32_t n,
            uint64_t total_dwords, uint8_t *packed, int strict, uint32_t *bad) {
    // (grid-stride: a launch's global size is 32 bits -- a thread per dword of a 37 GB set would not fit; see elem_grid)
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_dwords; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t byte = t * 4;
        uint32_t lo = 0, hi = n;            // last s with pk_off[s] <= byte
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pk_off[mid] <= byte) lo = mid; else hi = mid;
        }
        const uint32_t s = lo;
        const uint32_t L = len[s];
        const uint64_t w = (byte - pk_off[s]) >> 2;          // dword index inside the sequence
        if (w * 16 >= L) continue;                           // alignment padding
        const uint8_t *src = text + text_off[s] + w * 16;
        const uint32_t nb = (uint32_t)min((uint64_t)16, (uint64_t)L - w * 16);
        uint32_t word = 0, notacgt = 0;
        for (uint32_t k = 0; k < nb; ++k) {
            const uint32_t ch = src[k];
            const uint32_t code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : 3u;   // C2I, dna_seq.h:21
            notacgt |= (code == 3u && ch != 'T');
            word |= code << (8 * (k >> 2) + 6 - 2 * (k & 3));   // byte k/4, first base in bits 7:6
        }
        *reinterpret_cast<uint32_t *>(packed + byte) = word;    // padding bytes of the last dword stay 0
        if (notacgt) atomicOr(bad, 1u);
    }
}

// Bit planes of a packed set (dev_common.h: SeqSetDev::plane): thread w owns plane word w of the whole set.
__global__ void __launch_bounds__(256)
k_make_planes(const uint8_t *packed, const uint64_t *off, const uint32_t *len, const uint64_t *poff, uint32_t n,
              uint64_t total_words, uint32_t *plane) {
    // (grid-stride: ten million 15 kb reads are 4.7 G plane words, more than a launch's 32-bit global size holds -- a thread per
    // word silently ran the first 2^32-th of them only, tools/rehearse_config4.py; see elem_grid)
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < total_words; w += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n;            // last s with poff[s] <= w
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (poff[mid] <= w) lo = mid; else hi = mid;
        }
        const uint32_t s = lo;
        const uint64_t k = w - poff[s];     // word index inside the sequence
        const uint32_t L = len[s];
        uint32_t plo = 0, phi = 0;
        if (k * 32 < L) {
            planes_from_packed(packed + off[s], (int)(k * 32), plo, phi);
            const uint32_t valid = L - (uint32_t)(k * 32);
            if (valid < 32) { plo &= (1u << valid) - 1u; phi &= (1u << valid) - 1u; }   // nothing of the neighbour's bytes
        }
        plane[2 * w] = plo;                  // the two planes side by side: one line serves both (align_bitvec.h: load_planes32)
        plane[2 * w + 1] = phi;
    }
}

// Reverse complement of a set (pba_seqs_revcomp) into pba_seqs_from_text's layout: thread t owns packed dword t of the new
// set (16 bases), found as in k_pack_text.  Output base k of sequence s is source base L - 1 - k with code ^ 3 (A<->T, C<->G)
// where flip is null or flip[s] != 0, source base k otherwise.  The 16 source bases come from one unaligned 8-byte load (the
// source may be a binary read file's byte-aligned records); reversing the order of 2-bit codes is a bit reversal followed by
// a swap of the two bits of every code.  Pad bits stay 0, as k_pack_text leaves them.
__global__ void __launch_bounds__(256)
k_revcomp(const uint8_t *src, const uint64_t *src_off, const uint64_t *pk_off, const uint32_t *len, const uint8_t *flip, uint32_t n,
          uint64_t total_dwords, uint8_t *packed) {
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total_dwords; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t byte = t * 4;
        uint32_t lo = 0, hi = n;            // last s with pk_off[s] <= byte
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (pk_off[mid] <= byte) lo = mid; else hi = mid;
        }
        const uint32_t s = lo;
        const uint32_t L = len[s];
        const uint64_t w = (byte - pk_off[s]) >> 2;          // dword index inside the sequence
        if (w * 16 >= L) continue;                           // alignment padding (zeroed with the arena)
        const uint32_t nb = (uint32_t)min((uint64_t)16, (uint64_t)L - w * 16);
        const bool rc = !flip || flip[s];
        const uint64_t p = rc ? L - w * 16 - nb : w * 16;    // lowest source base of the dword's bases
        const uint64_t be = __builtin_bswap64(ld_u64(src + src_off[s] + (p >> 2)));
        uint32_t x = (uint32_t)((be << (2 * (p & 3))) >> 32);   // source base p in bits 31:30, p + 15 in bits 1:0
        if (rc) {
            x = __builtin_bitreverse32(x);
            x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);   // base p + 15 in bits 31:30 ... p in bits 1:0
            x = ~(x << (2 * (16 - nb)));                     // base p + nb - 1 (= L - 1 - 16w) first, complemented
        }
        if (nb < 16) x &= ~(0xFFFFFFFFu >> (2 * nb));        // nothing past the end
        *reinterpret_cast<uint32_t *>(packed + byte) = __builtin_bswap32(x);   // first base in bits 7:6 of the first byte
    }
}

extern "C" {

int pba_ctx_create(int device_id, pba_ctx **out) {
    if (!out) return PBA_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PBA_E_NODEVICE;
    if (device_id < 0 || device_id >= ndev) return PBA_E_NODEVICE;
    pba_ctx *ctx = new (std::nothrow) pba_ctx();
    if (!ctx) return PBA_E_NOMEM;
    ctx->device = device_id;
    ctx->err[0] = 0;
    if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&ctx->prop, device_id) != hipSuccess) {
        delete ctx;
        return PBA_E_NODEVICE;
    }
    if (strncmp(ctx->prop.gcnArchName, "gfx950", 6) != 0) {   // the code object holds gfx950 ISA only
        delete ctx;
        return PBA_E_NODEVICE;
    }
    if (hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return PBA_E_HIP;
    }
    ctx->stream = ctx->own_stream;
    for (int i = 0; i < 6; ++i)
        if (hipEventCreate(&ctx->ev[i]) != hipSuccess) { delete ctx; return PBA_E_HIP; }
    if (hipEventCreateWithFlags(&ctx->ev_aux, hipEventDisableTiming) != hipSuccess) { delete ctx; return PBA_E_HIP; }
    memset(&ctx->prof, 0, sizeof ctx->prof);
    if (hipMalloc((void **)&ctx->d_queue, 64) != hipSuccess) { delete ctx; return PBA_E_NOMEM; }
    ctx->d_scratch = nullptr; ctx->scratch_bytes = 0;
    memset(ctx->pool, 0, sizeof ctx->pool);
    ctx->h_stage = nullptr; ctx->h_stage_cap = 0; ctx->attr_done = 0;      // (ix_cache starts empty)
    // (kernels that take more than the default 64 KB of dynamic LDS are given the attribute by the translation unit
    // that launches them: tu_attrs() in each .hip)
    *out = ctx;
    return PBA_OK;
}

void pba_ctx_destroy(pba_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamDestroy(ctx->own_stream);
    for (int i = 0; i < 6; ++i) (void)hipEventDestroy(ctx->ev[i]);
    (void)hipEventDestroy(ctx->ev_aux);
    (void)hipFree(ctx->d_queue);
    if (ctx->d_scratch) (void)hipFree(ctx->d_scratch);
    for (auto &b : ctx->pool) if (b.p) (void)hipFree(b.p);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    ctx->ix_cache.release();
    delete ctx;
}

int pba_ctx_trim(pba_ctx *ctx) {
    if (!ctx) return PBA_E_INVALID;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (auto &b : ctx->pool) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    if (ctx->h_stage) { (void)hipHostFree(ctx->h_stage); ctx->h_stage = nullptr; ctx->h_stage_cap = 0; }
    ctx->ix_cache.release();
    if (ctx->d_scratch) { (void)hipFree(ctx->d_scratch); ctx->d_scratch = nullptr; ctx->scratch_bytes = 0; }
    return PBA_OK;
}

// ---- test support: what the ctx keeps between calls, and all of it overwritten (pba.h)
int pba_ctx_kept_bytes(pba_ctx *ctx, pba_kept_bytes *out) {
    if (!ctx || !out) return PBA_E_INVALID;
    memset(out, 0, sizeof *out);
    out->n_pool = POOL_COUNT;
    for (int s = 0; s < POOL_COUNT; ++s) out->pool[s] = ctx->pool[s].p ? ctx->pool[s].cap : 0;
    for (int s = 0; s < 3; ++s) out->ix_cache[s] = ctx->ix_cache.slot[s].p ? ctx->ix_cache.slot[s].cap : 0;
    out->scratch = ctx->d_scratch ? ctx->scratch_bytes : 0;
    out->stage = ctx->h_stage ? ctx->h_stage_cap : 0;
    out->queue = 64;
    return PBA_OK;
}

int pba_ctx_scribble(pba_ctx *ctx, int byte) {
    if (!ctx) return PBA_E_INVALID;
    const int v = byte & 0xFF;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int s = 0; s < POOL_COUNT; ++s)
        if (ctx->pool[s].p) HIPCHK(memset_big(ctx->pool[s].p, v, ctx->pool[s].cap, ctx->stream));
    if (ctx->d_scratch) HIPCHK(memset_big(ctx->d_scratch, v, ctx->scratch_bytes, ctx->stream));
    for (auto &x : ctx->ix_cache.slot)
        if (x.p) HIPCHK(memset_big(x.p, v, x.cap, ctx->stream));
    HIPCHK(hipMemsetAsync(ctx->d_queue, v, 64, ctx->stream));
    if (ctx->h_stage) memset(ctx->h_stage, v, ctx->h_stage_cap);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

const char *pba_ctx_error(const pba_ctx *ctx) { return ctx ? ctx->err : "null ctx"; }

int pba_ctx_set_stream(pba_ctx *ctx, void *hip_stream) {
    if (!ctx) return PBA_E_INVALID;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return PBA_OK;
}

int pba_ctx_sync(pba_ctx *ctx) {
    if (!ctx) return PBA_E_INVALID;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

int pba_ctx_last_profile(const pba_ctx *ctx, pba_profile *out) {
    if (!ctx || !out) return PBA_E_INVALID;
    *out = ctx->prof;
    return PBA_OK;
}

int pba_ctx_device_info(const pba_ctx *ctx, char *name, size_t cap, int *n_cu, int *clock_mhz, uint64_t *hbm) {
    if (!ctx) return PBA_E_INVALID;
    if (name && cap) snprintf(name, cap, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
    if (n_cu) *n_cu = ctx->prop.multiProcessorCount;
    if (clock_mhz) *clock_mhz = ctx->prop.clockRate / 1000;
    if (hbm) *hbm = (uint64_t)ctx->prop.totalGlobalMem;
    return PBA_OK;
}

// ---------------------------------------------------------------------------------------------
// host API: sequence sets
// ---------------------------------------------------------------------------------------------
// Every maker: its own checks, which fill h_off / h_len up to entry n; its own arena (seqs_arena) and where the payload comes
// from; seqs_finish, with its pack step if it has one.  The layout is seq_layout.h's.
void seqs_free(pba_seqs *s) {
    if (!s) return;
    (void)hipSetDevice(s->ctx->device);
    for (void *d : {(void *)s->d_planes, (void *)s->d_poff, (void *)s->d_alloc, (void *)s->d_off, (void *)s->d_len}) if (d) (void)hipFree(d);
    delete s;
}

// (a stream's set is left alone: pba_loc_stream_destroy frees the slot it looks into)
void pba_seqs_destroy(pba_seqs *s) { if (s && !s->borrowed) seqs_free(s); }

// a set under construction: freed with whatever it holds so far unless the maker hands it out (release)
typedef std::unique_ptr<pba_seqs, void (*)(pba_seqs *)> SeqsGuard;

// The arena of a set, `bytes` packed bytes between the kind's slacks.  Zeroed throughout -- the pack kernels skip the alignment
// padding, a file image is copied over it -- but for device-packed bytes, which are copied over everything between the slacks.
static int seqs_arena(pba_ctx *ctx, pba_seqs *s, ArenaKind kind, uint64_t bytes) {
    s->packed_bytes = bytes;
    HIPCHK(hipMalloc((void **)&s->d_alloc, arena_bytes(kind, bytes)));
    s->d_packed = s->d_alloc + kSlack;
    if (kind != ARENA_DEVICE_PACKED) HIPCHK(memset_big(s->d_alloc, 0, arena_bytes(kind, bytes), ctx->stream));
    else {
        HIPCHK(hipMemsetAsync(s->d_alloc, 0, kSlack, ctx->stream));
        HIPCHK(hipMemsetAsync(s->d_packed + bytes, 0, kSlack, ctx->stream));
    }
    return PBA_OK;
}

int planes_enqueue(pba_ctx *ctx, const pba_seqs *s, uint64_t words, hipStream_t stream) {
    if (!words) return PBA_OK;
    hipLaunchKernelGGL(k_make_planes, dim3(elem_grid(words, 256)), dim3(256), 0, stream, s->d_packed, s->d_off, s->d_len, s->d_poff,
                       s->n, words, s->d_planes + 2 * kPlaneSlack);
    HIPCHK(hipGetLastError());
    return PBA_OK;
}

// The one way a set is finished, on the ctx's stream: off / len / poff to the device (n + 1 entries each), the maker's pack
// step where it has one (it reads them and writes the arena), the zeroed planes, k_make_planes, and the synchronise that lets
// the host prefix and whatever the maker staged go.
static int seqs_finish(pba_ctx *ctx, pba_seqs *s, const std::function<int()> &pack = nullptr) {
    const size_t n1 = (size_t)s->n + 1;
    std::vector<uint64_t> poff(n1);
    const SeqTotals t = seq_layout(s->h_len.data(), s->n, nullptr, poff.data(), nullptr);
    s->max_len = t.max_len; s->plane_words = t.words + 2 * kPlaneSlack;
    HIPCHK(hipMalloc((void **)&s->d_off, sizeof(uint64_t) * n1));
    HIPCHK(hipMalloc((void **)&s->d_len, sizeof(uint32_t) * n1));
    HIPCHK(hipMalloc((void **)&s->d_poff, sizeof(uint64_t) * n1));
    HIPCHK(hipMemcpyAsync(s->d_off, s->h_off.data(), sizeof(uint64_t) * n1, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(s->d_len, s->h_len.data(), sizeof(uint32_t) * n1, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(s->d_poff, poff.data(), sizeof(uint64_t) * n1, hipMemcpyHostToDevice, ctx->stream));
    if (pack) PBA_TRY(pack());
    HIPCHK(hipMalloc((void **)&s->d_planes, s->plane_words * 2 * sizeof(uint32_t)));
    HIPCHK(memset_big(s->d_planes, 0, s->plane_words * 2 * sizeof(uint32_t), ctx->stream));
    PBA_TRY(planes_enqueue(ctx, s, t.words, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

// shared tail of the text constructors (these two, and pba_seqs_from_fastx): d_text / d_toff are on the device, h_toff on the host
int seqs_pack(pba_ctx *ctx, const uint8_t *d_text, const uint64_t *d_toff, const uint64_t *h_toff, uint32_t n,
              int strict, pba_seqs **out) {
    SeqsGuard g(seqs_new(ctx, n), seqs_free);
    pba_seqs *s = g.get();
    if (!s) PBA_FAIL(PBA_E_NOMEM, "pba_seqs");
    for (uint32_t i = 0; i < n; ++i) {
        if (h_toff[i + 1] < h_toff[i] || h_toff[i + 1] - h_toff[i] > 0x7FFFFFF0ull)
            PBA_FAIL(PBA_E_INVALID, "offsets must be non-decreasing and each sequence < 2^31 bases");
        s->h_len[i] = (uint32_t)(h_toff[i + 1] - h_toff[i]);
    }
    PBA_TRY(seqs_arena(ctx, s, ARENA_TEXT, seq_layout(s->h_len.data(), n, s->h_off.data(), nullptr, nullptr).packed));
    PBA_TRY(seqs_finish(ctx, s, [&]() -> int {
        DevBuf bad;
        if (hipMalloc(&bad.p, 4) != hipSuccess) PBA_FAIL(PBA_E_NOMEM, "hipMalloc");
        (void)hipMemsetAsync(bad.p, 0, 4, ctx->stream);
        const uint64_t total_dwords = s->packed_bytes / 4;
        if (total_dwords)
            hipLaunchKernelGGL(k_pack_text, dim3(elem_grid(total_dwords, 256)), dim3(256), 0, ctx->stream, d_text, d_toff, s->d_off,
                               s->d_len, n, total_dwords, s->d_packed, strict, bad.as<uint32_t>());
        uint32_t h_bad = 0;
        hipError_t e = hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) return ctx_fail(ctx, PBA_E_HIP, "k_pack_text", e);
        if (strict && h_bad) PBA_FAIL(PBA_E_ALPHABET, "pba_seqs_from_text");
        s->non_acgt = h_bad != 0;
        return PBA_OK;
    }));
    *out = g.release();
    return PBA_OK;
}

int pba_seqs_from_text(pba_ctx *ctx, const char *text, const uint64_t *offsets, uint32_t n, int strict_acgt,
                       pba_seqs **out) {
    if (!ctx || !offsets || !out || (!text && n && offsets[n] > offsets[0])) return PBA_E_INVALID;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t total = n ? offsets[n] : 0;
    DevBuf d_text, d_toff;
    HIPCHK(hipMalloc(&d_text.p, total + kSlack));
    HIPCHK(hipMalloc(&d_toff.p, sizeof(uint64_t) * (n + 1)));
    if (total) HIPCHK(hipMemcpyAsync(d_text.p, text, total, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_toff.p, offsets, sizeof(uint64_t) * (n + 1), hipMemcpyHostToDevice, ctx->stream));
    return seqs_pack(ctx, d_text.as<uint8_t>(), d_toff.as<uint64_t>(), offsets, n, strict_acgt, out);
}

int pba_seqs_from_device_text(pba_ctx *ctx, const void *d_text, const void *d_offsets, uint32_t n, uint64_t total_bytes,
                              uint32_t max_len, pba_seqs **out) {
    (void)total_bytes; (void)max_len;
    if (!ctx || !d_offsets || !out || (!d_text && n)) return PBA_E_INVALID;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<uint64_t> h_toff(n + 1);
    HIPCHK(hipMemcpyAsync(h_toff.data(), d_offsets, sizeof(uint64_t) * (n + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return seqs_pack(ctx, (const uint8_t *)d_text, (const uint64_t *)d_offsets, h_toff.data(), n, 0, out);
}

int pba_seqs_from_records(pba_ctx *ctx, const uint8_t *file, size_t file_len, uint32_t min_excl, uint32_t max_excl,
                          pba_seqs **out) {
    if (!ctx || !out || (!file && file_len)) return PBA_E_INVALID;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    size_t total = 0;
    const size_t kept = pba_open_binary(file, file_len, min_excl, max_excl, nullptr, 0, &total);
    if (kept > 0x7FFFFFFFull) PBA_FAIL(PBA_E_TOOLONG, "too many records");
    std::vector<uint64_t> recs(kept + 1);
    pba_open_binary(file, file_len, min_excl, max_excl, recs.data(), kept, nullptr);
    SeqsGuard g(seqs_new(ctx, (uint32_t)kept), seqs_free);
    pba_seqs *s = g.get();
    if (!s) PBA_FAIL(PBA_E_NOMEM, "pba_seqs");
    for (size_t i = 0; i < kept; ++i) {
        uint32_t L;
        memcpy(&L, file + recs[i], 4);
        if (recs[i] + 4 + ((uint64_t)L + 3) / 4 > file_len) PBA_FAIL(PBA_E_INVALID, "truncated record");
        s->h_off[i] = recs[i] + 4;      // payload follows the u32 length (dna_seq.h:119-121)
        s->h_len[i] = L;
    }
    s->h_off[kept] = file_len;
    // the file image goes up as it is (no re-packing), over an arena zeroed to the end of its slack
    PBA_TRY(seqs_arena(ctx, s, ARENA_RECORDS, file_len));
    if (file_len) HIPCHK(hipMemcpyAsync(s->d_packed, file, file_len, hipMemcpyHostToDevice, ctx->stream));
    PBA_TRY(seqs_finish(ctx, s));
    *out = g.release();
    return PBA_OK;
}

int pba_seqs_export(pba_ctx *ctx, const pba_seqs *s, void *d_dst, uint64_t cap, uint64_t *offsets) {
    if (!ctx || !s || !offsets || (!d_dst && s->packed_bytes)) return PBA_E_INVALID;
    if (cap < s->packed_bytes) PBA_FAIL(PBA_E_INVALID, "pba_seqs_export: buffer smaller than pba_seqs_packed_bytes");
    HIPCHK(hipSetDevice(ctx->device));
    if (s->packed_bytes) HIPCHK(copy_d2d(d_dst, s->d_packed, s->packed_bytes, ctx->stream));
    for (uint32_t i = 0; i < s->n; ++i) offsets[i] = s->h_off[i];
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

int pba_seqs_from_device_packed(pba_ctx *ctx, const void *d_packed, uint64_t n_bytes, const uint64_t *offsets, const uint32_t *lengths,
                                uint32_t n, int non_acgt, pba_seqs **out) {
    if (!ctx || !out || (!d_packed && n_bytes) || (n && (!offsets || !lengths))) return PBA_E_INVALID;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    SeqsGuard g(seqs_new(ctx, n), seqs_free);
    pba_seqs *s = g.get();
    if (!s) PBA_FAIL(PBA_E_NOMEM, "pba_seqs");
    s->non_acgt = non_acgt != 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets[i] + ((uint64_t)lengths[i] + 3) / 4 > n_bytes) PBA_FAIL(PBA_E_INVALID, "pba_seqs_from_device_packed: sequence outside the buffer");
        s->h_off[i] = offsets[i]; s->h_len[i] = lengths[i];
    }
    s->h_off[n] = n_bytes;
    // like a binary read file: the bytes go in as they are, offsets point into them; zeroed slack on both sides for the streaming reads
    PBA_TRY(seqs_arena(ctx, s, ARENA_DEVICE_PACKED, n_bytes));
    if (n_bytes) HIPCHK(copy_d2d(s->d_packed, d_packed, n_bytes, ctx->stream));
    PBA_TRY(seqs_finish(ctx, s));
    *out = g.release();
    return PBA_OK;
}

int revcomp_enqueue(pba_ctx *ctx, const pba_seqs *src, const pba_seqs *dst, const uint8_t *d_flip, hipStream_t stream) {
    const uint64_t total_dwords = dst->h_off[dst->n] / 4;
    if (!total_dwords) return PBA_OK;
    hipLaunchKernelGGL(k_revcomp, dim3(elem_grid(total_dwords, 256)), dim3(256), 0, stream, src->d_packed, src->d_off, dst->d_off,
                       dst->d_len, d_flip, dst->n, total_dwords, dst->d_packed);
    HIPCHK(hipGetLastError());
    return PBA_OK;
}

int pba_seqs_revcomp(pba_ctx *ctx, const pba_seqs *src, const uint8_t *flip, pba_seqs **out) {
    if (!ctx || !src || !out) return PBA_E_INVALID;
    *out = nullptr;
    if (src->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_seqs_revcomp: the set holds bytes outside ACGT (code 3 has no complement)");
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t n = src->n;
    SeqsGuard g(seqs_new(ctx, n), seqs_free);
    pba_seqs *s = g.get();
    if (!s) PBA_FAIL(PBA_E_NOMEM, "pba_seqs");
    s->h_len = src->h_len;
    PBA_TRY(seqs_arena(ctx, s, ARENA_TEXT, seq_layout(s->h_len.data(), n, s->h_off.data(), nullptr, nullptr).packed));
    DevBuf d_flip;                                            // (outlives its copy: seqs_finish synchronises)
    if (flip && n) {
        HIPCHK(hipMalloc(&d_flip.p, n));
        HIPCHK(hipMemcpyAsync(d_flip.p, flip, n, hipMemcpyHostToDevice, ctx->stream));
    }
    PBA_TRY(seqs_finish(ctx, s, [&] { return revcomp_enqueue(ctx, src, s, flip ? d_flip.as<uint8_t>() : nullptr, ctx->stream); }));
    *out = g.release();
    return PBA_OK;
}

int pba_seqs_non_acgt(const pba_seqs *s) { return s && s->non_acgt ? 1 : 0; }

uint32_t pba_seqs_count(const pba_seqs *s) { return s ? s->n : 0; }
uint32_t pba_seqs_max_len(const pba_seqs *s) { return s ? s->max_len : 0; }
uint64_t pba_seqs_packed_bytes(const pba_seqs *s) { return s ? s->packed_bytes : 0; }

int pba_seqs_lengths(const pba_seqs *s, uint32_t *lengths, uint32_t cap) {
    if (!s || !lengths) return PBA_E_INVALID;
    for (uint32_t i = 0; i < s->n && i < cap; ++i) lengths[i] = s->h_len[i];
    return PBA_OK;
}

int pba_seqs_get_text(pba_ctx *ctx, const pba_seqs *s, uint32_t i, char *text, size_t cap) {
    if (!ctx || !s || !text || i >= s->n) return PBA_E_INVALID;
    const uint32_t L = s->h_len[i];
    if (cap <= L) return PBA_E_INVALID;
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<uint8_t> pk(((size_t)L + 3) / 4 + 1);
    if (L) HIPCHK(hipMemcpyAsync(pk.data(), s->d_packed + s->h_off[i], ((size_t)L + 3) / 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    static const char base[4] = {'A', 'C', 'G', 'T'};
    for (uint32_t k = 0; k < L; ++k) text[k] = base[(pk[k >> 2] >> (6 - 2 * (k & 3))) & 3];
    text[L] = 0;
    return PBA_OK;
}

// The seed index (pba_index.hip) takes its generic level kernels' tile from here.  Small inputs: tiles of 4 096 entries (one chunk per
// thread) instead of 16 384 -- a 5 Mb target is 305 big tiles on 256 CUs.  (The rule stays in this file, in this form:
// tests/test_gpu_index.py reads its switch from the text below.)
bool index_small_tiles(uint64_t n_upper) { return n_upper <= (32ull << 20); }

}  // extern "C"
