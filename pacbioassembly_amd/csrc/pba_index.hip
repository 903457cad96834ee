// pba_index.hip -- the seed-hit index: the host half of its build (in stages, from one plan: index_plan.h), scan, dump and find.
// The kernels are seed_index.h's.  Everything here fails loudly (PBA_E_HIP): there is no CPU path behind these entry points.
#include "pba_host.h"

// an index under construction: destroyed with whatever it holds so far unless the builder hands it out (release)
typedef std::unique_ptr<pba_index, void (*)(pba_index *)> IndexGuard;

static uint32_t seg_grid(const ScanSeg &sg, int iters = PBA_IX_TILE_ITERS) {
    const uint64_t chunks = ((uint64_t)sg.hi + 15) / 16 - sg.lo / 16;
    return (uint32_t)((chunks + PBA_IX_TILE_THREADS * iters - 1) / (PBA_IX_TILE_THREADS * iters));
}

static pba_index *index_new(pba_ctx *ctx, uint32_t mask, uint32_t len, int mode, const VisitPlan &v) {
    pba_index *ix = new (std::nothrow) pba_index();
    if (!ix) return nullptr;
    ix->ctx = ctx; ix->mask = mask; ix->seq_len = len; ix->visited = v.visited; ix->nhead = v.nhead;
    ix->tail_top = v.tail_top; ix->mode = mode; ix->n_entries = 0; ix->d_ent = nullptr; ix->d_part_off = nullptr;
    ix->ent_cap = ix->off_cap = 0;
    ix->logP = 0;
    ix->n_seqs = 1; ix->d_cum = nullptr;
    return ix;
}

// device array of at least `bytes` for a new index: the cached one if it is large enough (a refused hipMalloc keeps the message
// it has always had, though the function whose variables it names is gone: callers may match on it)
static int ix_take(pba_ctx *ctx, int slot, size_t bytes, void **out, size_t *cap) {
    const hipError_t e = ctx->ix_cache.take(slot, bytes, out, cap);
    if (e != hipSuccess) return ctx_fail(ctx, PBA_E_HIP, "hipMalloc(out, bytes)", e);
    return PBA_OK;
}

// ---------------------------------------------------------------------------------------------
// the build, in stages
// ---------------------------------------------------------------------------------------------
// Level 1's source: a packed sequence walked in its visiting order, or (list non-null) the flat entry list of the exchange
// form, which goes through the generic level kernels (all-ones entries = padding).
struct Level1Src { const uint8_t *d_seq; uint32_t len, mask; const VisitPlan *v; const uint64_t *list; };
// the sizes of the 2^bits level-1 bins added to cnt1[bin] ...
// (level 1 keeps its tiles of 16 384 positions at any size: with 4 096 the per-bin reservations of four times the
// workgroups cost more than the idle CUs -- 13 -> 26 us and 35 -> 43 us at 5 Mb)
static void seq_count(pba_ctx *ctx, const Level1Src &s, int bits, uint32_t *cnt1) {
    for (int i = 0; i < s.v->nseg; ++i)
        hipLaunchKernelGGL(k_seed_count<PBA_IX_TILE_ITERS>, dim3(seg_grid(s.v->segs[i])), dim3(PBA_IX_TILE_THREADS), 0, ctx->stream,
                           s.d_seq, s.len, s.mask, s.v->segs[i], bits, cnt1);
}
// ... and the entries scattered into dst through cursor[bin]
static void seq_scatter(pba_ctx *ctx, const Level1Src &s, int bits, uint32_t *cursor, uint64_t *dst) {
    for (int i = 0; i < s.v->nseg; ++i)
        hipLaunchKernelGGL(k_seed_scatter<PBA_IX_TILE_ITERS>, dim3(seg_grid(s.v->segs[i])), dim3(PBA_IX_TILE_THREADS), 0, ctx->stream,
                           s.d_seq, s.len, s.mask, s.v->segs[i], bits, cursor, dst);
}

// the entry buffer the index does not keep: back to the ctx's cache when the build ends, whichever way
struct SpareEnt { pba_ctx *ctx; void *p = nullptr; size_t cap = 0; ~SpareEnt() { ctx->ix_cache.give(IXC_ENT2, p, cap); } };

// the device and host arrays of one build
struct IndexBufs {
    uint64_t *ent[2];        // the levels ping-pong: level k writes ent[k & 1]; [0] is the index's, [1] the spare
    uint32_t *offs, *work;   // the two pooled arenas (index_plan.h)
    uint32_t tile;           // entries of a tile of the generic level kernels
    uint32_t *h_stat;        // pinned (read after ev_aux): [0] largest partition <= the LDS sort's cap, [1] partitions beyond it, [2] entries
};

// Two entry buffers from the ctx's one-deep cache of index arrays (in a loop of build / destroy the two just swap roles) --
// the second only where a second level reads the first --, the pooled arenas, the offsets arena zeroed by one memset.
static int index_buffers(pba_ctx *ctx, pba_index *ix, const IndexPlan &pl, uint64_t n_upper, SpareEnt &spare, IndexBufs &B) {
    const size_t ent_bytes = sizeof(uint64_t) * (n_upper + 1);
    PBA_TRY(ix_take(ctx, IXC_ENT, ent_bytes, (void **)&ix->d_ent, &ix->ent_cap));   // (the index owns it from here on: error paths free it with the index)
    if (pl.n_levels > 1) PBA_TRY(ix_take(ctx, IXC_ENT2, ent_bytes, &spare.p, &spare.cap));
    B.ent[0] = ix->d_ent; B.ent[1] = (uint64_t *)spare.p;
    B.tile = index_small_tiles(n_upper) ? 4096u : (uint32_t)PBA_IX_TILE_POS;
    POOL(POOL_IX_OFFS, sizeof(uint32_t) * pl.offs_words, B.offs);
    HIPCHK(hipMemsetAsync(B.offs, 0, sizeof(uint32_t) * pl.offs_words, ctx->stream));
    POOL(POOL_IX_WORK, sizeof(uint32_t) * pl.work_words, B.work);
    PBA_TRY(stage_reserve(ctx, 64));
    B.h_stat = (uint32_t *)ctx->h_stage;
    return PBA_OK;
}

// What a generic level (every level but a sequence's first) reads: the entries `src` grouped by the top done bits of their
// hash, tile_pre[g] = tiles of the groups before g.  *grid: >= the tiles there are; the rest exit.
static int level_source(pba_ctx *ctx, const IndexPlan &pl, int k, const uint64_t *src, uint64_t n_upper, const IndexBufs &B,
                        LvlSrc *L, uint32_t *grid) {
    uint32_t *const tile_pre = B.work + pl.tile_pre;
    L->src = src; L->done = k ? pl.done[k - 1] : 0; L->bits = pl.bits[k];
    L->n_groups = (uint32_t)(1ull << L->done); L->tile = B.tile; L->tile_pre = tile_pre;
    if (k == 0) {                                                          // one group: the whole list
        uint32_t *const list_off = B.offs + pl.list_off;
        const uint32_t h[2] = {0u, (uint32_t)n_upper}, t[2] = {0u, (uint32_t)((n_upper + B.tile - 1) / B.tile)};
        HIPCHK(hipMemcpyAsync(list_off, h, sizeof h, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(tile_pre, t, sizeof t, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));                         // (h, t are locals)
        L->off_prev = list_off;
    } else {
        L->off_prev = B.offs + pl.lvl_off[k - 1];
        hipLaunchKernelGGL(k_lvl_tiles, dim3((L->n_groups + 255) / 256), dim3(256), 0, ctx->stream, L->off_prev, L->n_groups, B.tile, tile_pre + 1);
        scan_inclusive(ctx, tile_pre + 1, L->n_groups, B.work + pl.scan);
    }
    *grid = (uint32_t)(n_upper / B.tile + L->n_groups + 1);
    return PBA_OK;
}

// The level loop: count, scan (the offsets of the level, and the cursors the scatter consumes), scatter.
static int index_partition(pba_ctx *ctx, const IndexPlan &pl, const Level1Src &s, uint64_t n_upper, const IndexBufs &B) {
    uint32_t *const cursor = B.work + pl.cursor;
    for (int k = 0; k < pl.n_levels; ++k) {
        uint32_t *const off_k = B.offs + pl.lvl_off[k];
        const uint64_t bins = 1ull << pl.done[k];
        LvlSrc L;
        uint32_t grid = 0;
        if (k > 0 || s.list) PBA_TRY(level_source(ctx, pl, k, k ? B.ent[(k - 1) & 1] : s.list, n_upper, B, &L, &grid));
        if (grid) hipLaunchKernelGGL(k_lvl_count, dim3(grid), dim3(PBA_IX_TILE_THREADS), 0, ctx->stream, L, off_k + 1);
        else seq_count(ctx, s, pl.bits[k], off_k + 1);
        if (!scan_inclusive(ctx, off_k + 1, bins, B.work + pl.scan, cursor))
            HIPCHK(hipMemcpyAsync(cursor, off_k, sizeof(uint32_t) * bins, hipMemcpyDeviceToDevice, ctx->stream));
        if (k == pl.n_levels - 1) {
            // The partitions' sizes are final once the last level has been counted: the totals the host decides by (entries,
            // the largest partition the LDS sort takes, partitions beyond it) are queued for the host BEFORE the last scatter
            // and read while it runs -- the sort is launched without the chip waiting for a host round trip (75 us of a
            // 330 us build at 5 Mb).
            hipLaunchKernelGGL(k_part_max, dim3((uint32_t)((pl.P + 255) / 256)), dim3(256), 0, ctx->stream, off_k, (uint32_t)pl.P, B.offs + pl.stat);
            HIPCHK(hipMemcpyAsync(B.h_stat, B.offs + pl.stat, 12, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipEventRecord(ctx->ev_aux, ctx->stream));
        }
        if (grid) hipLaunchKernelGGL(k_lvl_scatter, dim3(grid), dim3(PBA_IX_TILE_THREADS), 0, ctx->stream, L, cursor, B.ent[k & 1]);
        else seq_scatter(ctx, s, pl.bits[k], cursor, B.ent[k & 1]);
    }
    return PBA_OK;
}

// Every partition sorted by key, then insertion order: k_seg_sort (buckets by the key's gathered care bits, sorted in
// wavefront registers); what it leaves -- partitions beyond 16 384 entries or with a bucket beyond 256: low-complexity
// targets -- goes through the global bitonic pass.
static int index_sort(pba_ctx *ctx, pba_index *ix, const IndexPlan &pl, const IndexBufs &B) {
    const uint64_t P = pl.P;
    uint32_t *const ov = B.offs + pl.ov;
    launch_seg_sort(ctx, ix->d_ent, ix->d_ent, ix->d_part_off, nullptr, P, std::max(B.h_stat[0], B.h_stat[1] ? 0xFFFFFFFFu : 0u),
                    seg_bkt_key(ix->mask), ov, pl.ov_cap);
    std::vector<uint32_t> h_ov(1 + pl.ov_cap, 0);
    HIPCHK(hipMemcpyAsync(h_ov.data(), ov, sizeof(uint32_t) * (1 + pl.ov_cap), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    if (!h_ov[0]) return PBA_OK;
    std::vector<uint32_t> h_off(P + 1);
    HIPCHK(hipMemcpyAsync(h_off.data(), ix->d_part_off, sizeof(uint32_t) * (P + 1), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<uint32_t> todo;
    if (h_ov[0] > pl.ov_cap) { for (uint64_t q = 0; q < P; ++q) todo.push_back((uint32_t)q); }   // (list overflow: check them all)
    else todo.assign(h_ov.begin() + 1, h_ov.begin() + 1 + h_ov[0]);
    std::sort(todo.begin(), todo.end());
    todo.erase(std::unique(todo.begin(), todo.end()), todo.end());
    for (uint32_t q : todo)
        if (h_off[q + 1] - h_off[q] > 1) PBA_TRY(sort_partition_global(ctx, ix->d_ent + h_off[q], h_off[q + 1] - h_off[q]));
    return PBA_OK;
}

// The build: the partition levels and the sort of at most n_upper entries (positions visited / slots of the gathered list).
static int index_levels(pba_ctx *ctx, pba_index *ix, uint64_t n_upper, const Level1Src &s) {
    if (n_upper > 0xFFFFFFF0ull) PBA_FAIL(PBA_E_TOOLONG, "more than 2^32 index entries");
    const IndexPlan pl = index_plan(n_upper);
    ix->logP = pl.logP;
    SpareEnt spare{ctx};
    IndexBufs B;
    PBA_TRY(index_buffers(ctx, ix, pl, n_upper, spare, B));
    (void)hipEventRecord(ctx->ev[0], ctx->stream);
    PBA_TRY(index_partition(ctx, pl, s, n_upper, B));
    // totals: entries, the largest partition the LDS sort takes, partitions beyond it (queued before the last scatter)
    HIPCHK(hipEventSynchronize(ctx->ev_aux));
    HIPCHK(hipGetLastError());
    ix->n_entries = B.h_stat[2];
    PBA_TRY(ix_take(ctx, IXC_OFF, sizeof(uint32_t) * (pl.P + 1), (void **)&ix->d_part_off, &ix->off_cap));
    HIPCHK(hipMemcpyAsync(ix->d_part_off, B.offs + pl.lvl_off[pl.n_levels - 1], sizeof(uint32_t) * (pl.P + 1), hipMemcpyDeviceToDevice, ctx->stream));
    // the index keeps the buffer the last level wrote; the other one is the spare
    if ((pl.n_levels - 1) & 1) {
        ix->d_ent = B.ent[1]; spare.p = B.ent[0];
        std::swap(ix->ent_cap, spare.cap);
    }
    if (ix->n_entries) PBA_TRY(index_sort(ctx, ix, pl, B));
    (void)hipEventRecord(ctx->ev[1], ctx->stream);
    (void)hipEventSynchronize(ctx->ev[1]);
    HIPCHK(hipGetLastError());
    (void)hipEventElapsedTime(&ctx->prof.index_ms, ctx->ev[0], ctx->ev[1]);
    return PBA_OK;
}

extern "C" {

void pba_index_destroy(pba_index *ix) {
    if (!ix) return;
    pba_ctx *ctx = ix->ctx;
    (void)hipSetDevice(ctx->device);
    ctx->ix_cache.give(IXC_ENT, ix->d_ent, ix->ent_cap);
    ctx->ix_cache.give(IXC_OFF, ix->d_part_off, ix->off_cap);
    if (ix->d_cum) (void)hipFree(ix->d_cum);
    delete ix;
}

uint64_t pba_index_entries(const pba_index *ix) { return ix ? ix->n_entries : 0; }
uint32_t pba_index_visited(const pba_index *ix) { return ix ? ix->visited : 0; }
uint32_t pba_index_seqs(const pba_index *ix) { return ix ? ix->n_seqs : 0; }

// sort one oversize partition in global memory
int sort_partition_global(pba_ctx *ctx, uint64_t *d_part, uint32_t n) {
    uint32_t N = 2;
    while (N < n) N <<= 1;
    DevBuf tmp;
    HIPCHK(hipMalloc(&tmp.p, sizeof(uint64_t) * N));
    HIPCHK(hipMemcpyAsync(tmp.p, d_part, sizeof(uint64_t) * n, hipMemcpyDeviceToDevice, ctx->stream));
    if (N > n)
        hipLaunchKernelGGL(k_fill_u64, dim3((N - n + 255) / 256), dim3(256), 0, ctx->stream, tmp.as<uint64_t>(), n, N,
                           ~0ull);
    for (uint32_t k = 2; k <= N; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1)
            hipLaunchKernelGGL(k_bitonic_step, dim3((N / 2 + 255) / 256), dim3(256), 0, ctx->stream, tmp.as<uint64_t>(),
                               N, k, j);
    HIPCHK(hipMemcpyAsync(d_part, tmp.p, sizeof(uint64_t) * n, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}


int pba_index_build(pba_ctx *ctx, const pba_seqs *target, uint32_t seq, uint32_t mask, int mode, pba_index **out) {
    if (!ctx || !target || !out || seq >= target->n) return PBA_E_INVALID;
    if (mode != PBA_INDEX_ALL && mode != PBA_INDEX_HEAD_TAIL) return PBA_E_INVALID;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t len = target->h_len[seq];
    if (len > 0x7FFFFFF0u) PBA_FAIL(PBA_E_TOOLONG, "target sequence");
    const VisitPlan v = visit_plan(len, mode);
    IndexGuard ix(index_new(ctx, mask, len, mode, v), pba_index_destroy);
    if (!ix) PBA_FAIL(PBA_E_NOMEM, "pba_index");
    uint64_t npos = 0;
    for (int s = 0; s < v.nseg; ++s) npos += v.segs[s].hi - v.segs[s].lo;
    PBA_TRY(index_levels(ctx, ix.get(), npos, Level1Src{target->d_packed + target->h_off[seq], len, mask, &v, nullptr}));
    *out = ix.release();
    return PBA_OK;
}

int pba_index_scan(pba_ctx *ctx, const pba_seqs *target, uint32_t seq, uint32_t mask, int mode, uint32_t part,
                   uint32_t nparts, void *d_entries, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !target || !d_entries || !n_out || seq >= target->n || nparts == 0 || part >= nparts) return PBA_E_INVALID;
    if (mode != PBA_INDEX_ALL && mode != PBA_INDEX_HEAD_TAIL) return PBA_E_INVALID;
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t len = target->h_len[seq];
    const VisitPlan v = visit_plan(len, mode);
    // this rank's contiguous slice of the ordinal space [0, visited)
    const uint64_t nv = v.nseg ? (uint64_t)v.segs[v.nseg - 1].ord0 + (v.segs[v.nseg - 1].hi - v.segs[v.nseg - 1].lo) : 0;
    const uint64_t o_lo = nv * part / nparts, o_hi = nv * (part + 1) / nparts;
    DevBuf counter;
    HIPCHK(hipMalloc(&counter.p, 8));
    HIPCHK(hipMemsetAsync(counter.p, 0, 8, ctx->stream));
    const uint8_t *d_seq = target->d_packed + target->h_off[seq];
    for (int s = 0; s < v.nseg; ++s) {
        const ScanSeg &g = v.segs[s];
        const uint64_t g_lo = g.ord0, g_hi = (uint64_t)g.ord0 + (g.hi - g.lo);
        const uint64_t a = std::max(o_lo, g_lo), b = std::min(o_hi, g_hi);
        if (a >= b) continue;
        ScanSeg c;
        c.descending = g.descending; c.ord0 = (uint32_t)a;
        if (!g.descending) { c.lo = g.lo + (uint32_t)(a - g_lo); c.hi = g.lo + (uint32_t)(b - g_lo); }
        else { c.lo = g.hi - (uint32_t)(b - g_lo); c.hi = g.hi - (uint32_t)(a - g_lo); }
        hipLaunchKernelGGL(k_seed_emit, dim3(seg_grid(c)), dim3(PBA_IX_TILE_THREADS), 0, ctx->stream, d_seq, len, mask, c,
                           (uint64_t *)d_entries, (unsigned long long)cap, counter.as<unsigned long long>());
    }
    HIPCHK(hipGetLastError());
    unsigned long long h_n = 0;
    HIPCHK(hipMemcpyAsync(&h_n, counter.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (h_n > cap) PBA_FAIL(PBA_E_INVALID, "pba_index_scan: entry buffer too small");
    *n_out = h_n;
    return PBA_OK;
}

int pba_index_from_entries(pba_ctx *ctx, const void *d_entries, uint64_t n, uint32_t mask, int mode, uint32_t seq_len,
                           pba_index **out) {
    if (!ctx || !out || (!d_entries && n)) return PBA_E_INVALID;
    if (mode != PBA_INDEX_ALL && mode != PBA_INDEX_HEAD_TAIL) return PBA_E_INVALID;
    *out = nullptr;
    HIPCHK(hipSetDevice(ctx->device));
    const VisitPlan v = visit_plan(seq_len, mode);
    IndexGuard ix(index_new(ctx, mask, seq_len, mode, v), pba_index_destroy);
    if (!ix) PBA_FAIL(PBA_E_NOMEM, "pba_index");
    PBA_TRY(index_levels(ctx, ix.get(), n, Level1Src{nullptr, 0, 0, nullptr, (const uint64_t *)d_entries}));
    *out = ix.release();
    return PBA_OK;
}

// PBA_INDEX_ALL over every sequence of a set: one segmented emit (k_seed_emit_set) into a flat list, then the levels and
// the sort of the exchange form.  An entry's ordinal is its global position, so dump / find / the locate kernel read it
// through ix_pos_of like any PBA_INDEX_ALL ordinal.
int pba_index_build_set(pba_ctx *ctx, const pba_seqs *target, uint32_t mask, pba_index **out) {
    if (!ctx || !target || !out) return PBA_E_INVALID;
    *out = nullptr;
    const uint32_t n = target->n;
    uint64_t total = 0;
    for (uint32_t c = 0; c < n; ++c) total += target->h_len[c];
    if (total >= 0x7FFFFFF0ull) PBA_FAIL(PBA_E_TOOLONG, "pba_index_build_set: the set holds 2^31 bases or more");
    HIPCHK(hipSetDevice(ctx->device));
    VisitPlan v = visit_plan(0, PBA_INDEX_ALL);
    v.visited = (uint32_t)total;
    IndexGuard ix(index_new(ctx, mask, (uint32_t)total, PBA_INDEX_ALL, v), pba_index_destroy);
    if (!ix) PBA_FAIL(PBA_E_NOMEM, "pba_index");
    ix->n_seqs = n;
    ix->h_cum.resize((size_t)n + 1);
    // the tile table: (sequence, first chunk) of every PBA_IX_TILE_THREADS x PBA_IX_TILE_ITERS chunks of a sequence
    std::vector<SetTile> tiles;
    const uint32_t per = PBA_IX_TILE_THREADS * PBA_IX_TILE_ITERS;
    uint32_t g = 0;
    for (uint32_t c = 0; c < n; ++c) {
        ix->h_cum[c] = g;
        const uint32_t L = target->h_len[c], chunks = (uint32_t)(((uint64_t)L + 15) / 16);
        for (uint32_t c0 = 0; c0 < chunks; c0 += per) tiles.push_back(SetTile{c, c0});
        g += L;
    }
    ix->h_cum[n] = g;
    HIPCHK(hipMalloc((void **)&ix->d_cum, sizeof(uint32_t) * ((size_t)n + 1)));
    HIPCHK(hipMemcpyAsync(ix->d_cum, ix->h_cum.data(), sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, ctx->stream));
    DevBuf d_tiles, d_list, counter;
    HIPCHK(hipMalloc(&d_list.p, sizeof(uint64_t) * (total + 1)));
    HIPCHK(hipMalloc(&counter.p, 8));
    HIPCHK(hipMemsetAsync(counter.p, 0, 8, ctx->stream));
    if (!tiles.empty()) {
        HIPCHK(hipMalloc(&d_tiles.p, sizeof(SetTile) * tiles.size()));
        HIPCHK(hipMemcpyAsync(d_tiles.p, tiles.data(), sizeof(SetTile) * tiles.size(), hipMemcpyHostToDevice, ctx->stream));
        // (a launch's global size is a 32-bit number: at most 2^23 workgroups of 256 threads per launch)
        for (size_t t0 = 0; t0 < tiles.size(); t0 += (size_t)1 << 23) {
            const uint32_t grid = (uint32_t)std::min<size_t>(tiles.size() - t0, (size_t)1 << 23);
            hipLaunchKernelGGL(k_seed_emit_set, dim3(grid), dim3(PBA_IX_TILE_THREADS), 0, ctx->stream, target->d_packed, target->d_off,
                               target->d_len, ix->d_cum, d_tiles.as<SetTile>() + t0, mask, d_list.as<uint64_t>(),
                               (unsigned long long)total, counter.as<unsigned long long>());
        }
        HIPCHK(hipGetLastError());
    }
    unsigned long long h_n = 0;
    HIPCHK(hipMemcpyAsync(&h_n, counter.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));                  // (h_cum's, tiles' and h_n's copies have landed)
    if (h_n > total) PBA_FAIL(PBA_E_HIP, "pba_index_build_set: more entries than positions");
    PBA_TRY(index_levels(ctx, ix.get(), h_n, Level1Src{nullptr, 0, 0, nullptr, d_list.as<uint64_t>()}));
    *out = ix.release();
    return PBA_OK;
}

int pba_index_dump(pba_ctx *ctx, const pba_index *ix, uint32_t *keys, int32_t *pos, uint64_t cap, uint64_t *n) {
    if (!ctx || !ix || !n) return PBA_E_INVALID;
    HIPCHK(hipSetDevice(ctx->device));
    *n = ix->n_entries;
    if (!keys || !pos) return PBA_OK;
    std::vector<uint64_t> ent(ix->n_entries + 1);
    if (ix->n_entries)
        HIPCHK(hipMemcpyAsync(ent.data(), ix->d_ent, sizeof(uint64_t) * ix->n_entries, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ent.resize(ix->n_entries);
    // partitions are sorted; this merges them by key -- on the host, so a dump does not witness the order the device left (a
    // partition it left unsorted, an entry in the wrong partition, dumps the same): pba_index_find does
    std::sort(ent.begin(), ent.end());
    for (uint64_t i = 0; i < ent.size() && i < cap; ++i) {
        keys[i] = (uint32_t)(ent[i] >> 32);
        pos[i] = ix_ord_pos(ix->nhead, ix->tail_top, (uint32_t)ent[i]);
    }
    return PBA_OK;
}

int pba_index_find(pba_ctx *ctx, const pba_index *ix, const uint32_t *keys, uint32_t n_keys, uint64_t *hit_off,
                   int32_t *hit_pos, uint64_t hit_cap) {
    if (!ctx || !ix || !hit_off || (!keys && n_keys)) return PBA_E_INVALID;
    HIPCHK(hipSetDevice(ctx->device));
    hit_off[0] = 0;
    if (!n_keys) return PBA_OK;
    DevBuf d_keys, d_beg, d_cnt, d_off, d_pos;
    HIPCHK(hipMalloc(&d_keys.p, 4ull * n_keys));
    HIPCHK(hipMalloc(&d_beg.p, 4ull * n_keys));
    HIPCHK(hipMalloc(&d_cnt.p, 4ull * n_keys));
    HIPCHK(hipMemcpyAsync(d_keys.p, keys, 4ull * n_keys, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_find_count, dim3((n_keys + 255) / 256), dim3(256), 0, ctx->stream, ix->dev(),
                       d_keys.as<uint32_t>(), n_keys, d_beg.as<uint32_t>(), d_cnt.as<uint32_t>());
    std::vector<uint32_t> cnt(n_keys);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, 4ull * n_keys, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (uint32_t q = 0; q < n_keys; ++q) hit_off[q + 1] = hit_off[q] + cnt[q];
    const uint64_t total = hit_off[n_keys];
    if (!hit_pos || !total) return PBA_OK;
    const uint64_t ncopy = std::min(total, hit_cap);
    HIPCHK(hipMalloc(&d_off.p, 8ull * (n_keys + 1)));
    HIPCHK(hipMalloc(&d_pos.p, 4ull * (ncopy + 1)));
    HIPCHK(hipMemcpyAsync(d_off.p, hit_off, 8ull * (n_keys + 1), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_find_fill, dim3((n_keys + 255) / 256), dim3(256), 0, ctx->stream, ix->dev(), d_beg.as<uint32_t>(),
                       d_off.as<uint64_t>(), n_keys, d_pos.as<int32_t>(), ncopy);
    HIPCHK(hipMemcpyAsync(hit_pos, d_pos.p, 4ull * ncopy, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    return PBA_OK;
}

}  // extern "C"
