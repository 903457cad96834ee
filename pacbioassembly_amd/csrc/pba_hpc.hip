// pba_hpc.hip -- homopolymer compression: a set with every run collapsed to one base, the run starts kept on the device, and
// overlap / map rows found in compressed space lifted back to original coordinates (pba_hpc_*).  Host side; the
// kernels are in hpc.h.  One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
//
// The sequences go through in consecutive ranges ("chunks") of at most max_bases input bases, so that every 32-bit counter of
// a chunk stays below 2^31.  First every chunk's heads are counted per tile (k_hpc_heads) and the tile counts scanned
// (scan_inclusive); the chunks' totals size the map and the text.  Then every chunk's k_hpc_emit writes bases and run starts
// at their global rank, and the first rank of each sequence comes back (one copy, one synchronise per chunk): those are the
// text offsets.  The text is packed by pba_seqs_from_device_text, as pba_clip_apply packs its reads.  The rank of a head does
// not depend on the cut.  Work buffers are pooled (POOL_HPC_*); the object owns the map on the device and the lengths on the host.
#include "pba_host.h"

#include "hpc.h"

extern "C" {

struct pba_hpc {
    int device;
    uint32_t n;
    std::vector<uint32_t> h_len_in, h_len_out;
    std::vector<uint64_t> h_hoff;                // rank of every sequence's first head, and the total: also the text offsets
    DevBuf map;                                  // one allocation: hoff[0 .. n] (u64), then S of every head (u32) at its rank
    pba_hpc_stats stats;
    const unsigned long long *d_hoff() const { return map.as<unsigned long long>(); }
    uint32_t *d_starts() const { return (uint32_t *)(map.as<uint8_t>() + 8 * ((size_t)n + 1)); }
};

static const uint64_t kHpcMaxBases = 0x7FFFFFF0ull;           // input bases of one chunk: its head counts and word indices are 32-bit

int pba_seqs_hpc(pba_ctx *ctx, const pba_seqs *src, uint64_t max_bases, pba_seqs **out, pba_hpc **map, pba_hpc_stats *stats) {
    if (!ctx || !src || !out) return PBA_E_INVALID;
    *out = nullptr;
    if (map) *map = nullptr;
    if (src->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_seqs_hpc: the set holds bytes outside ACGT (code 3 stands for N as well as T: a run of TNT would collapse)");
    HIPCHK(hipSetDevice(ctx->device));
    StageClock clk;
    if (!clk.init()) PBA_FAIL(PBA_E_HIP, "pba_seqs_hpc: hipEventCreate");
    std::unique_ptr<pba_hpc, void (*)(pba_hpc *)> m(new (std::nothrow) pba_hpc(), pba_hpc_destroy);
    if (!m) PBA_FAIL(PBA_E_NOMEM, "pba_hpc");
    const uint32_t n = src->n;
    const size_t N = std::max<size_t>(n, 1);
    m->device = ctx->device; m->n = n;
    m->h_len_in.assign(src->h_len.begin(), src->h_len.begin() + n);
    m->h_len_out.assign(n, 0);
    m->h_hoff.assign((size_t)n + 1, 0);
    memset(&m->stats, 0, sizeof m->stats);
    pba_hpc_stats &s = m->stats;
    s.n_seqs = n;
    hipStream_t st = ctx->stream;

    // the cut, decided on the host from the lengths; the plane words of every sequence as every maker lays them out
    std::vector<uint64_t> poff((size_t)n + 1);
    const SeqTotals tot = seq_layout(m->h_len_in.data(), n, nullptr, poff.data(), nullptr);
    s.max_len_in = tot.max_len;
    const uint64_t limit = max_bases ? std::min(max_bases, kHpcMaxBases) : kHpcMaxBases;
    struct Chunk { uint32_t lo, hi, n_words, n_tiles; uint64_t tile_at; };
    std::vector<Chunk> chunks;
    uint64_t tiles_all = 0, tiles_widest = 0;
    for (uint32_t lo = 0; lo < n;) {
        uint32_t hi = lo + 1;
        uint64_t bases = m->h_len_in[lo];
        while (hi < n && bases + m->h_len_in[hi] <= limit) bases += m->h_len_in[hi++];
        if (bases > kHpcMaxBases) PBA_FAIL(PBA_E_TOOLONG, "pba_seqs_hpc: a sequence of 0x7FFFFFF0 bases or more");
        s.n_bases_in += bases;
        Chunk c;
        c.lo = lo; c.hi = hi; c.n_words = (uint32_t)(poff[hi] - poff[lo]);          // (words <= bases)
        c.n_tiles = (c.n_words + HPC_TILE_WORDS - 1) / HPC_TILE_WORDS; c.tile_at = tiles_all;
        tiles_all += c.n_tiles; tiles_widest = std::max<uint64_t>(tiles_widest, c.n_tiles);
        chunks.push_back(c);
        lo = hi;
    }
    s.n_chunks = (uint32_t)chunks.size();

    size_t carve = 0;
    auto take = [&carve](size_t bytes) { const size_t at = carve; carve += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_first = take(8 * N), o_tiles = take(4 * std::max<uint64_t>(tiles_all, 1)), o_scan = take(4 * scan_scratch_words(tiles_widest));
    uint8_t *work = nullptr;
    POOL(POOL_HPC_WORK, carve, work);
    unsigned long long *first = (unsigned long long *)(work + o_first);
    uint32_t *tiles = (uint32_t *)(work + o_tiles), *scan = (uint32_t *)(work + o_scan);
    const SeqSetDev S = src->dev();

    std::vector<uint32_t> h_total(chunks.size(), 0);          // the heads of every chunk: the last entry of its scanned tiles
    {
        const auto timed = clk.time(st, &s.heads_ms);
        for (size_t k = 0; k < chunks.size(); ++k) {
            const Chunk &c = chunks[k];
            if (!c.n_tiles) continue;
            hipLaunchKernelGGL(k_hpc_heads, dim3(c.n_tiles), dim3(HPC_THREADS), 0, st, S, c.lo, c.hi, (uint64_t)poff[c.lo], c.n_words,
                               tiles + c.tile_at);
            (void)scan_inclusive(ctx, tiles + c.tile_at, c.n_tiles, scan);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&h_total[k], tiles + c.tile_at + c.n_tiles - 1, 4, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
    }
    uint64_t H = 0;
    for (uint32_t t : h_total) H += t;
    s.n_bases_out = H;

    HIPCHK(hipMalloc(&m->map.p, 8 * ((size_t)n + 1) + 4 * std::max<uint64_t>(H, 1)));
    char *text = nullptr;
    POOL(POOL_HPC_TEXT, (size_t)H + kSlack, text);
    uint64_t rank0 = 0;
    std::vector<unsigned long long> h_first;
    for (size_t k = 0; k < chunks.size(); ++k) {
        const Chunk &c = chunks[k];
        const auto timed = clk.time(st, &s.emit_ms);
        h_first.assign(c.hi - c.lo, 0ull);
        if (c.n_tiles) {
            hipLaunchKernelGGL(k_hpc_emit, dim3(c.n_tiles), dim3(HPC_THREADS), 0, st, S, c.lo, c.hi, (uint64_t)poff[c.lo], c.n_words,
                               tiles + c.tile_at, (unsigned long long)rank0, text, m->d_starts(), first);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h_first.data(), first + c.lo, 8 * (size_t)(c.hi - c.lo), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        // an empty sequence has no word and no lane: it begins where the next sequence with a base begins, or at the chunk's end
        uint64_t next = rank0 + h_total[k];
        for (uint32_t r = c.hi; r-- > c.lo;) {
            if (m->h_len_in[r]) next = h_first[r - c.lo];
            m->h_hoff[r] = next;
        }
        rank0 += h_total[k];
    }
    m->h_hoff[n] = H;
    for (uint32_t r = 0; r < n; ++r) {
        m->h_len_out[r] = (uint32_t)(m->h_hoff[r + 1] - m->h_hoff[r]);
        s.max_len_out = std::max(s.max_len_out, m->h_len_out[r]);
    }
    HIPCHK(hipMemcpyAsync(m->map.p, m->h_hoff.data(), 8 * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    {
        const auto timed = clk.time(st, &s.pack_ms);
        PBA_TRY(pba_seqs_from_device_text(ctx, text, m->map.p, n, H, s.max_len_out, out));
    }
    if (stats) *stats = s;
    if (map) *map = m.release();
    return PBA_OK;
}

uint32_t pba_hpc_count(const pba_hpc *m) { return m ? m->n : 0; }

int pba_hpc_lengths(const pba_hpc *m, uint32_t *len_in, uint32_t *len_out, uint32_t cap) {
    if (!m) return PBA_E_INVALID;
    for (uint32_t i = 0; i < m->n && i < cap; ++i) {
        if (len_in) len_in[i] = m->h_len_in[i];
        if (len_out) len_out[i] = m->h_len_out[i];
    }
    return PBA_OK;
}

int pba_hpc_run_starts(pba_ctx *ctx, const pba_hpc *m, uint32_t seq, uint32_t *starts, uint32_t cap, uint32_t *n_out) {
    if (!ctx || !m || !n_out || (!starts && cap)) return PBA_E_INVALID;
    *n_out = 0;
    if (seq >= m->n) PBA_FAIL(PBA_E_INVALID, "pba_hpc_run_starts: no such sequence");
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t H = m->h_len_out[seq];
    const uint32_t k = std::min(cap, H);
    if (k) HIPCHK(hipMemcpyAsync(starts, m->d_starts() + m->h_hoff[seq], 4 * (size_t)k, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (cap > H) starts[H] = m->h_len_in[seq];
    *n_out = H + 1;
    return PBA_OK;
}

// the lengths of a map's original sequences into the pooled work buffer at `at`: what index H of a look-up reads
static int hpc_map_dev(pba_ctx *ctx, const pba_hpc *m, uint8_t *work, size_t at, HpcMapDev *dev) {
    if (m->n) HIPCHK(hipMemcpyAsync(work + at, m->h_len_in.data(), 4 * (size_t)m->n, hipMemcpyHostToDevice, ctx->stream));
    *dev = HpcMapDev{m->d_hoff(), m->d_starts(), (const uint32_t *)(work + at)};
    return PBA_OK;
}

int pba_hpc_lift_overlaps(pba_ctx *ctx, const pba_hpc *m, const pba_strand_overlap *rows, uint64_t n, pba_strand_overlap *out) {
    if (!ctx || !m || ((!rows || !out) && n)) return PBA_E_INVALID;
    // check_overlap_rows reads a set's count and host lengths: the compressed ones, as the map remembers them
    pba_seqs lens{};
    lens.n = m->n; lens.max_len = m->stats.max_len_out;
    lens.h_len = m->h_len_out;
    PBA_TRY(check_overlap_rows(ctx, "pba_hpc_lift_overlaps", &lens, rows, n, true, false));
    if (!n) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t *work = nullptr, *d_rows = nullptr;
    POOL(POOL_HPC_WORK, 4 * std::max<size_t>(m->n, 1), work);
    POOL(POOL_LAY_ROWS, sizeof(pba_strand_overlap) * n, d_rows);
    hipStream_t st = ctx->stream;
    HpcMapDev dev;
    PBA_TRY(hpc_map_dev(ctx, m, work, 0, &dev));
    HIPCHK(hipMemcpyAsync(d_rows, rows, sizeof(pba_strand_overlap) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hpc_lift_overlaps, dim3(elem_grid(n, 256)), dim3(256), 0, st, (const pba_strand_overlap *)d_rows, n, dev,
                       (pba_strand_overlap *)d_rows);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_rows, sizeof(pba_strand_overlap) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));                         // (the lengths must outlive their copy)
    return PBA_OK;
}

int pba_hpc_lift_map_rows(pba_ctx *ctx, const pba_hpc *reads_map, const pba_hpc *target_map, const pba_map_row *rows, uint64_t n,
                          pba_map_row *out) {
    if (!ctx || !reads_map || !target_map || ((!rows || !out) && n)) return PBA_E_INVALID;
    const char *who = "pba_hpc_lift_map_rows";
    for (uint64_t k = 0; k < n; ++k) {
        const pba_map_row &r = rows[k];
        if (!r.found) continue;
        if (r.strand != 1 && r.strand != -1) ROWS_FAIL(PBA_E_INVALID, "a found row's strand is neither +1 nor -1");
        if (r.read < 0 || (uint32_t)r.read >= reads_map->n) ROWS_FAIL(PBA_E_INVALID, "a row names a read outside reads_map");
        if (r.contig < 0 || (uint32_t)r.contig >= target_map->n) ROWS_FAIL(PBA_E_INVALID, "a row names a contig outside target_map");
        const int64_t hr = reads_map->h_len_out[r.read], hc = target_map->h_len_out[r.contig];
        if (r.r_beg < 0 || r.r_beg >= r.r_end || r.r_end > hr || r.c_beg < 0 || r.c_beg >= r.c_end || r.c_end > hc)
            ROWS_FAIL(PBA_E_INVALID, "a row's interval is empty or outside its compressed sequence");
    }
    if (!n) return PBA_OK;
    HIPCHK(hipSetDevice(ctx->device));
    uint8_t *work = nullptr, *d_rows = nullptr;
    const size_t at_t = (4 * std::max<size_t>(reads_map->n, 1) + 255) & ~(size_t)255;
    POOL(POOL_HPC_WORK, at_t + 4 * std::max<size_t>(target_map->n, 1), work);
    POOL(POOL_LAY_ROWS, sizeof(pba_map_row) * n, d_rows);
    hipStream_t st = ctx->stream;
    HpcMapDev dr, dt;
    PBA_TRY(hpc_map_dev(ctx, reads_map, work, 0, &dr));
    PBA_TRY(hpc_map_dev(ctx, target_map, work, at_t, &dt));
    HIPCHK(hipMemcpyAsync(d_rows, rows, sizeof(pba_map_row) * n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hpc_lift_map_rows, dim3(elem_grid(n, 256)), dim3(256), 0, st, (const pba_map_row *)d_rows, n, dr, dt,
                       (pba_map_row *)d_rows);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_rows, sizeof(pba_map_row) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return PBA_OK;
}

int pba_hpc_last_stats(const pba_hpc *m, pba_hpc_stats *out) {
    if (!m || !out) return PBA_E_INVALID;
    *out = m->stats;
    return PBA_OK;
}

void pba_hpc_destroy(pba_hpc *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}

}  // extern "C"
