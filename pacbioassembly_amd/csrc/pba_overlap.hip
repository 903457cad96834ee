// pba_overlap.hip -- all-vs-all overlap: host side of csrc/overlap.h.
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
//
// A call (overlap_table) fills one OvlCall and runs these stages on it, each leaving what the next one reads:
//   ovl_size_fused    k_pt_ctx (once per table), k_ovl_scan (census and / or writing)  -> h_off / h_valid, d_cand = survivors of 32 rows
//   ovl_size_rowsweep k_ovl_count, k_ovl_fill (the cross-check form: no prefilter)      -> h_off / h_slice, d_cand = every slot, `big`
//   ovl_sort_slices   k_seg_sort, k_ovl_split (big), sort_partition_global (reported)   -> every target's slice in the reference's try order
//   ovl_make_items    k_ovl_items                                                       -> d_items / n_items, d_out / dev_cap, d_redo / redo_cap, counters 0..3 cleared
//   ovl_walk          k_ovl_walk / k_ovl_walk_rc in the rings nb1, nb_mid, nb2          -> d_out rows, counters overlaps / pairs
//   ovl_collect       k_ovl_after (fused: pairs = past the gate - behind a success)     -> caller's rows by (target, query), stats
// The environment hooks of the tests and tools are read by ovl_hooks_from_env() only, once per call, and decide for that
// call only; what a probe table remembers between calls is written through tab_attach_records / tab_learn_* only.
#include "pba_host.h"
#include "overlap.h"

#include <memory>

// (the attribute belongs to the current device: remembered per ctx, so a second ctx on another GPU sets it there too)
static void tu_attrs(pba_ctx *ctx) {
    if (ctx->attr_done & 4u) return;
    ctx->attr_done |= 4u;
    PBA_BIG_LDS(k_ovl_walk<0>);
    PBA_BIG_LDS(k_ovl_walk_rc<0>);
}

// a kernel template over the probe table's form (overlap.h: HASHED)
#define PBA_PT_LAUNCH(hashed, KERNEL, grid, block, lds, stream, ...)                                  \
    do {                                                                                              \
        if (hashed) hipLaunchKernelGGL(KERNEL<true>, grid, block, lds, stream, __VA_ARGS__);          \
        else hipLaunchKernelGGL(KERNEL<false>, grid, block, lds, stream, __VA_ARGS__);                \
    } while (0)

// the probe table of a read set (overlap.h: ProbeTab), built once and scanned by every target range
struct pba_probe_table {
    // what the table is: set by pba_probe_table_create
    int device = 0;
    ProbeTab T = {};               // (prec stays null here: the records are attached below)
    bool hashed = false;
    uint32_t t2 = 0;
    uint64_t n_entries = 0;
    float build_ms = 0;
    // the record set attached on first use (overlap.h: k_pt_ctx) and the read set it was filled from (reads == nullptr: not
    // yet): the QUERY set of the calls that scan the table (the set whose probes filled it: the reads, or their reverse
    // complement); a table belongs to one read set, and the arena's address and size are compared too, should a set have
    // been replaced at the same address
    mutable struct { const pba_seqs *reads; const uint8_t *packed; uint64_t bytes; uint4 *prec; } rec = {nullptr, nullptr, 0, nullptr};
    // what earlier target ranges taught it about this read set: the largest candidate slice of a target in the last counted
    // range of >= 1 024 targets (0: none yet), and whether the narrow window certifies its overlaps under (R, ring) -- the
    // next ranges skip the census and the sample (three launches and their tails per call)
    mutable struct { uint32_t slice_max; int wide_known; double wide_R; int wide_nb1; } learned = {0, -1, 0.0, 0};   // wide_known -1: not sampled yet, 0: start narrow, 1: wider
};

static ProbeTab tab_dev(const pba_probe_table *tab) { ProbeTab T = tab->T; T.prec = tab->rec.prec; return T; }

// the records of the probe table from the query set, once per table
static int tab_attach_records(pba_ctx *ctx, const pba_probe_table *tab, const pba_seqs *qset) {
    if (tab->rec.reads == qset && tab->rec.packed == qset->d_packed && tab->rec.bytes == qset->packed_bytes) return PBA_OK;
    if (!tab->rec.prec) HIPCHK(hipMalloc((void **)&tab->rec.prec, sizeof(uint4) * ((uint64_t)tab->n_entries + 1)));
    if (tab->n_entries)
        hipLaunchKernelGGL(k_pt_ctx, dim3((uint32_t)((tab->n_entries + 255) / 256)), dim3(256), 0, ctx->stream, tab_dev(tab), qset->dev(),
                           (uint32_t)tab->n_entries);
    HIPCHK(hipGetLastError());
    tab->rec.reads = qset; tab->rec.packed = qset->d_packed; tab->rec.bytes = qset->packed_bytes;
    return PBA_OK;
}
// what a later range goes by: the largest slice of a counted range
static void tab_learn_slices(const pba_probe_table *tab, uint32_t nt, uint32_t largest) {
    if (nt >= 1024 || tab->learned.slice_max == 0) tab->learned.slice_max = std::max(largest, 1u);
}
// equal room for every target of a range of nt: pct % of the largest need seen, + 64 (0: no census yet, switched off, or too
// much to hand out blindly)
static uint32_t tab_room_for(const pba_probe_table *tab, uint32_t nt, int pct, uint64_t max_cand) {
    if (tab->learned.slice_max == 0 || pct <= 0) return 0;
    const uint64_t room = (uint64_t)tab->learned.slice_max * (uint64_t)pct / 100 + 64;
    return room * nt < max_cand ? (uint32_t)room : 0;
}
static void tab_learn_wide(const pba_probe_table *tab, bool wide, double R, int nb1) {
    tab->learned.wide_known = wide ? 1 : 0; tab->learned.wide_R = R; tab->learned.wide_nb1 = nb1;
}
// -1: no sample under (R, ring) yet; 0 / 1: start narrow / wider
static int tab_wide_decision(const pba_probe_table *tab, double R, int nb1) {
    return tab->learned.wide_R == R && tab->learned.wide_nb1 == nb1 ? tab->learned.wide_known : -1;
}

static int check_max_trial(pba_ctx *ctx, int max_trial) {
    if (max_trial < 1 || 2 * max_trial >= (1 << PBA_OVL_JD_BITS)) PBA_FAIL(PBA_E_INVALID, "max_trial must be in [1, 63]");
    return PBA_OK;
}
static int check_strand_sets(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc) {
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        PBA_FAIL(PBA_E_INVALID, "pba_overlap_strands: reads_rc differs from reads in count or lengths");
    if (reads->non_acgt || (reads_rc && reads_rc->non_acgt)) PBA_FAIL(PBA_E_ALPHABET, "pba_overlap_strands: the read set holds bytes outside ACGT");
    return PBA_OK;
}

// the probe table of every read of `set`, built here (the single-GPU form of pba_overlap_all)
static int own_table(pba_ctx *ctx, const pba_seqs *set, uint32_t mask, int max_trial, pba_probe_table **tab) {
    HIPCHK(hipSetDevice(ctx->device));                       // (the entry buffer belongs on the ctx's card, whoever calls)
    const uint64_t pcap = (uint64_t)set->n * 2u * (uint32_t)max_trial;
    DevBuf d_pent;
    HIPCHK(hipMalloc(&d_pent.p, sizeof(uint64_t) * (pcap + 1)));
    uint64_t n_pent = 0;
    PBA_TRY(pba_overlap_probes(ctx, set, 0, set->n, mask, max_trial, d_pent.p, pcap, &n_pent));
    return pba_probe_table_create(ctx, d_pent.p, n_pent, mask, max_trial, tab);
}

// ---------------------------------------------------------------------------------------------
// host API: probes and their table
// ---------------------------------------------------------------------------------------------
extern "C" {
int pba_overlap_probes(pba_ctx *ctx, const pba_seqs *reads, uint32_t q_lo, uint32_t q_hi, uint32_t mask, int max_trial,
                       void *d_entries, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !reads || !d_entries || !n_out || q_lo > q_hi || q_hi > reads->n) return PBA_E_INVALID;
    PBA_TRY(check_max_trial(ctx, max_trial));
    if (reads->n >= (1u << 24)) PBA_FAIL(PBA_E_TOOLONG, "at most 2^24 reads");
    HIPCHK(hipSetDevice(ctx->device));
    tu_attrs(ctx);
    const uint32_t t2 = 2u * (uint32_t)max_trial;
    const uint64_t slots = (uint64_t)(q_hi - q_lo) * t2;
    DevBuf counter;
    HIPCHK(hipMalloc(&counter.p, 8));
    HIPCHK(hipMemsetAsync(counter.p, 0, 8, ctx->stream));
    if (slots)
        hipLaunchKernelGGL(k_probe_emit, dim3((uint32_t)((slots + 255) / 256)), dim3(256), 0, ctx->stream, reads->dev(), q_lo,
                           q_hi - q_lo, t2, mask, (uint64_t *)d_entries, (unsigned long long)cap,
                           counter.as<unsigned long long>());
    unsigned long long h_n = 0;
    HIPCHK(hipMemcpyAsync(&h_n, counter.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    if (h_n > cap) PBA_FAIL(PBA_E_INVALID, "pba_overlap_probes: entry buffer too small");
    *n_out = h_n;
    return PBA_OK;
}

int pba_overlap_all(pba_ctx *ctx, const pba_seqs *reads, uint32_t t_lo, uint32_t t_hi, uint32_t mask, double R,
                    int max_trial, int overlap_min, int kernel, pba_overlap *out, uint64_t cap, uint64_t *n_out,
                    pba_overlap_stats *stats) {
    if (!ctx || !reads || !n_out) return PBA_E_INVALID;
    PBA_TRY(check_max_trial(ctx, max_trial));
    HIPCHK(hipSetDevice(ctx->device));
    tu_attrs(ctx);
    pba_probe_table *tab = nullptr;
    PBA_TRY(own_table(ctx, reads, mask, max_trial, &tab));
    const int rc = pba_overlap_all_table(ctx, reads, t_lo, t_hi, tab, R, overlap_min, kernel, out, cap, n_out, stats);
    pba_probe_table_destroy(tab);
    return rc;
}

int pba_overlap_all_probes(pba_ctx *ctx, const pba_seqs *reads, uint32_t t_lo, uint32_t t_hi, const void *d_probe_entries,
                           uint64_t n_probe_slots, uint32_t mask, double R, int max_trial, int overlap_min, int kernel,
                           pba_overlap *out, uint64_t cap, uint64_t *n_out, pba_overlap_stats *stats) {
    if (!ctx || !n_out) return PBA_E_INVALID;
    pba_probe_table *tab = nullptr;
    PBA_TRY(pba_probe_table_create(ctx, d_probe_entries, n_probe_slots, mask, max_trial, &tab));
    const int rc = pba_overlap_all_table(ctx, reads, t_lo, t_hi, tab, R, overlap_min, kernel, out, cap, n_out, stats);
    pba_probe_table_destroy(tab);
    return rc;
}

void pba_probe_table_destroy(pba_probe_table *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    const ProbeTab T = tab_dev(t);
    for (void *p : {(void *)T.start, (void *)T.pid, (void *)T.pkey, (void *)T.presence, (void *)T.prec})
        if (p) (void)hipFree(p);
    delete t;
}

uint64_t pba_probe_table_entries(const pba_probe_table *t) { return t ? t->n_entries : 0; }

int pba_probe_table_create(pba_ctx *ctx, const void *d_probe_entries, uint64_t n_probe_slots, uint32_t mask, int max_trial,
                           pba_probe_table **out) {
    if (!ctx || !out || (!d_probe_entries && n_probe_slots)) return PBA_E_INVALID;
    *out = nullptr;
    PBA_TRY(check_max_trial(ctx, max_trial));
    if (n_probe_slots >= PBA_OVL_MAX_PROBES) PBA_FAIL(PBA_E_TOOLONG, "probe table: 2^32 probe slots or more (reads x 2 x max_trial)");
    HIPCHK(hipSetDevice(ctx->device));
    pba_probe_table *t = new (std::nothrow) pba_probe_table();
    if (!t) PBA_FAIL(PBA_E_NOMEM, "pba_probe_table");
    t->device = ctx->device; t->t2 = 2u * (uint32_t)max_trial;
    struct Guard { pba_probe_table *p; ~Guard() { pba_probe_table_destroy(p); } } guard{t};
    const int care = __builtin_popcount(mask);
    t->hashed = care > PBA_PT_MAX_BITS;
    ProbeTab &T = t->T;
    T.mask = mask; T.bits = t->hashed ? PBA_PT_MAX_BITS : care;
    if (!t->hashed) compress_masks(mask, T.mv);
    const uint64_t B = 1ull << T.bits, pres_words = std::max<uint64_t>(1, B / 32);
    HIPCHK(hipMalloc((void **)&T.start, sizeof(uint32_t) * (B + 1)));
    HIPCHK(hipMalloc((void **)&T.presence, sizeof(uint32_t) * pres_words));
    HIPCHK(hipMemsetAsync(T.start, 0, sizeof(uint32_t) * (B + 1), ctx->stream));
    HIPCHK(hipMemsetAsync(T.presence, 0, sizeof(uint32_t) * pres_words, ctx->stream));
    (void)hipEventRecord(ctx->ev[0], ctx->stream);
    const uint64_t n = n_probe_slots;
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    const uint64_t *ent = (const uint64_t *)d_probe_entries;
    if (grid) PBA_PT_LAUNCH(t->hashed, k_pt_count, dim3(grid), dim3(256), 0, ctx->stream, ent, n, T);
    // start[b + 1] = entries of bucket b  ->  inclusive scan  ->  start[b] = first entry of bucket b
    DevBuf d_tiles, d_cursor;
    HIPCHK(hipMalloc(&d_tiles.p, sizeof(uint32_t) * scan_scratch_words(B)));
    scan_inclusive(ctx, T.start + 1, B, d_tiles.as<uint32_t>());
    uint32_t total = 0;
    HIPCHK(hipMemcpyAsync(&total, T.start + B, sizeof total, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    t->n_entries = total;
    HIPCHK(hipMalloc((void **)&T.pid, sizeof(uint32_t) * ((uint64_t)total + 1)));
    if (t->hashed) HIPCHK(hipMalloc((void **)&T.pkey, sizeof(uint32_t) * ((uint64_t)total + 1)));
    if (total) {
        HIPCHK(hipMalloc(&d_cursor.p, sizeof(uint32_t) * B));
        HIPCHK(hipMemcpyAsync(d_cursor.p, T.start, sizeof(uint32_t) * B, hipMemcpyDeviceToDevice, ctx->stream));
        PBA_PT_LAUNCH(t->hashed, k_pt_fill, dim3(grid), dim3(256), 0, ctx->stream, ent, n, T, d_cursor.as<uint32_t>(), t->t2);
    }
    (void)hipEventRecord(ctx->ev[1], ctx->stream);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    (void)hipEventElapsedTime(&t->build_ms, ctx->ev[0], ctx->ev[1]);
    guard.p = nullptr;
    *out = t;
    return PBA_OK;
}
}  // extern "C"

// ---------------------------------------------------------------------------------------------
// one call: targets [t_lo, t_lo + nt) of `reads` against the probe table of the queries `qset`
// ---------------------------------------------------------------------------------------------
// the test and tuning hooks of a call, from the environment (read per call: the tests set and unset them between calls)
struct OvlHooks { uint64_t max_cand; int capfill_pct; uint32_t room; size_t sample_min; bool sample_min_set; int wide; /* -1 unset */ };
static OvlHooks ovl_hooks_from_env() {
    OvlHooks h{PBA_OVL_MAX_CANDIDATES, 125, 0, 4096, false, -1};
    const char *e;
    if ((e = getenv("PBA_OVL_MAX_CANDIDATES"))) h.max_cand = std::min<uint64_t>(h.max_cand, (uint64_t)atoll(e));   // the limit of a call at test sizes
    if ((e = getenv("PBA_OVL_CAPFILL_PCT"))) h.capfill_pct = atoi(e);     // 0 = never equal room (a full census per range), small = overflow and fall back
    if ((e = getenv("PBA_OVL_ROOM"))) h.room = (uint32_t)std::max(0, atoi(e));   // this much room for every target of every range (the overflow path at will)
    if ((e = getenv("PBA_OVL_SAMPLE_MIN"))) { h.sample_min = (size_t)std::max(1L, atol(e)); h.sample_min_set = true; }   // small inputs through the sampled decision
    if ((e = getenv("PBA_OVL_WIDE"))) h.wide = atoi(e) != 0 ? 1 : 0;      // tuning: start this call narrow / in the wider ring, no sample
    return h;
}

// the slots of a call's counter buffer
enum OvlCnt {
    CNT_OVERLAPS = 0, CNT_PAIRS = 1, CNT_PARKED = 2,   // the walk: rows written, pairs tried (row-sweep form), runs parked by the current launch
    CNT_SEED_MATCHES = 4, CNT_PAST_GATE = 5,           // k_ovl_scan: candidates, and those past the gate
    CNT_AFTER_SUCCESS = 6, CNT_SLOTS = 8               // k_ovl_after: candidates behind a success
};

struct OvlCall {
    pba_ctx *ctx;
    const pba_seqs *reads, *qset;
    uint32_t t_lo, nt;
    const pba_probe_table *tab;
    ProbeTab T;                                  // the table as the kernels see it
    Plan pl;
    bool fused;                                  // the bit-vector kernels: first 32 rows in the scan, survivors only in memory
    OvlCfg ocfg;
    OvlHooks hooks;
    DevBuf d_cnt;
    // (the big arrays of a call live in the ctx's pool: mapping gigabytes anew for each target range of a table took longer
    // than everything the kernels do)
    BufRef d_slice, d_off, d_valid, d_ipre, d_cand, d_out, d_redo, d_items;
    std::vector<uint32_t> h_slice, h_off, h_valid;   // per target: slots needed, first slot, candidates the walk sees
    std::vector<uint32_t> big;                   // row-sweep form: targets whose slice outgrows one LDS sort
    uint32_t biggest_small = 2;
    uint64_t total = 0;                          // slots listed
    uint64_t n_cand = 0, n_ok = 0;               // fused form: the scan's seed matches, and those past the gate
    uint64_t cap = 0, dev_cap = 0, redo_cap = 0; // rows the caller takes, the device list holds, runs the redo list holds
    uint64_t n_items = 0;
    int nb_mid = 0;                              // the widest ring between the narrow one and the reference band's (0: none)
    bool launched = false;                       // the walk has had its first launch (ctx->prof names it)
    pba_overlap_stats st;

    unsigned long long *cnt(OvlCnt k) const { return d_cnt.as<unsigned long long>() + k; }
    hipError_t cnt_clear(OvlCnt first, int n) const { return hipMemsetAsync(cnt(first), 0, 8 * (size_t)n, ctx->stream); }
    hipError_t cnt_read(OvlCnt first, int n, unsigned long long *h) const {
        return hipMemcpyAsync(h, cnt(first), 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream);
    }
};

static const char *const kTooManyCandidates = "pba_overlap_all: 2^32 candidates or more in one target range; use smaller ranges";

// one launch of the scan over `grid` targets, every stride-th of the range: needed[] into h_slice, survivors written or not
static int ovl_scan(OvlCall &c, bool write, uint32_t cap_slots, uint32_t grid, uint32_t stride) {
    pba_ctx *ctx = c.ctx;
    const PreChecks pre_t = PreChecks::on_host(c.ocfg.R);
    const size_t plane_lds = sizeof(uint32_t) * 2 * ((size_t)c.reads->max_len / 32 + 2);     // the target's bit planes (k_ovl_scan)
    HIPCHK(c.cnt_clear(CNT_SEED_MATCHES, 2));
    const uint32_t *so = write ? c.d_off.as<uint32_t>() : nullptr;
    PBA_PT_LAUNCH(c.tab->hashed, k_ovl_scan, dim3(grid), dim3(PBA_WAVE * PBA_OVL_WAVES), plane_lds, ctx->stream, c.T, c.reads->dev(), c.t_lo, stride, so,
                  c.d_cand.as<uint64_t>(), cap_slots, c.d_slice.as<uint32_t>(), c.ocfg, pre_t, c.cnt(CNT_SEED_MATCHES));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c.h_slice.data(), c.d_slice.p, sizeof(uint32_t) * grid, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

// Fused form.  How much room a target's survivors need is not known before its candidates have been through their 32 rows:
// a census (the scan without writing) and exact slices, or equal room from what the table remembers, exact on overflow.
static int ovl_size_fused(OvlCall &c) {
    pba_ctx *ctx = c.ctx;
    const uint32_t nt = c.nt;
    const uint64_t max_cand = c.hooks.max_cand;
    PBA_TRY(tab_attach_records(ctx, c.tab, c.qset));
    c.T = tab_dev(c.tab);
    uint32_t room = tab_room_for(c.tab, nt, c.hooks.capfill_pct, max_cand);
    if (c.hooks.room > 0 && (uint64_t)c.hooks.room * nt < max_cand) room = c.hooks.room;   // (a forced room is held to the same limit)
    bool have_exact = false;
    if (room == 0) {
        // census: all targets of a small range, every k-th of a big one (a sixteenth of the work; what it misses the
        // overflow path catches)
        uint32_t n_s = c.hooks.capfill_pct > 0 ? std::min<uint32_t>(nt, std::max<uint32_t>(64u, nt / 16u)) : nt;
        const uint32_t stride = nt / n_s;
        if (stride == 1) n_s = nt;                           // (no sample worth the name: every target)
        PBA_TRY(ovl_scan(c, false, 0, n_s, stride));
        if (stride == 1) have_exact = true;
        else {
            uint32_t mx = 0;
            for (uint32_t i = 0; i < n_s; ++i) mx = std::max(mx, c.h_slice[i]);
            room = mx + mx / 2 + 64;
            if ((uint64_t)room * nt >= max_cand) { PBA_TRY(ovl_scan(c, false, 0, nt, 1)); have_exact = true; }   // (too much room to hand out blindly)
        }
    }
    for (int attempt = 0; attempt < 2; ++attempt) {
        uint64_t extent = 0;
        if (have_exact) {
            uint32_t mx = 0;
            for (uint32_t i = 0; i < nt; ++i) {
                c.h_off[i] = (uint32_t)extent; extent += c.h_slice[i]; mx = std::max(mx, c.h_slice[i]);
                if (extent >= max_cand) PBA_FAIL(PBA_E_TOOLONG, kTooManyCandidates);
            }
            tab_learn_slices(c.tab, nt, mx);
        } else {
            for (uint32_t i = 0; i < nt; ++i) c.h_off[i] = (uint32_t)((uint64_t)i * room);
            extent = (uint64_t)nt * room;
        }
        c.h_off[nt] = (uint32_t)extent;
        HIPCHK(hipMemcpyAsync(c.d_off.p, c.h_off.data(), sizeof(uint32_t) * (nt + 1), hipMemcpyHostToDevice, ctx->stream));
        POOL(POOL_OVL_CAND, sizeof(uint64_t) * (extent + 1), c.d_cand.p);
        PBA_TRY(ovl_scan(c, true, have_exact ? 0xFFFFFFFFu : room, nt, 1));
        if (have_exact) break;
        bool over = false;
        uint32_t mx = 0;
        for (uint32_t i = 0; i < nt; ++i) { over = over || c.h_slice[i] > room; mx = std::max(mx, c.h_slice[i]); }
        if (!over) { c.st.cap_fill = 1; tab_learn_slices(c.tab, nt, mx); break; }
        c.st.cap_overflow = 1;                               // a target outgrew its room: once more, with what each one needed
        have_exact = true;
    }
    unsigned long long h_tot[2] = {0, 0};
    HIPCHK(c.cnt_read(CNT_SEED_MATCHES, 2, h_tot));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    c.n_cand = h_tot[0]; c.n_ok = h_tot[1];
    for (uint32_t i = 0; i < nt; ++i) { c.h_valid[i] = c.h_slice[i]; c.total += c.h_slice[i]; }
    HIPCHK(hipMemcpyAsync(c.d_valid.p, c.h_valid.data(), sizeof(uint32_t) * nt, hipMemcpyHostToDevice, ctx->stream));
    c.st.n_prefiltered = c.n_ok - c.total;
    return PBA_OK;
}

// Row-sweep form: count the slice of the candidate array every target needs, prefix, fill
static int ovl_size_rowsweep(OvlCall &c) {
    pba_ctx *ctx = c.ctx;
    const uint32_t nt = c.nt;
    const dim3 block(PBA_WAVE * PBA_OVL_WAVES);
    PBA_PT_LAUNCH(c.tab->hashed, k_ovl_count, dim3(nt), block, 0, ctx->stream, c.T, c.reads->dev(), c.t_lo, nt, c.d_slice.as<uint32_t>());
    HIPCHK(hipMemcpyAsync(c.h_slice.data(), c.d_slice.p, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    for (uint32_t i = 0; i < nt; ++i) {
        c.h_off[i] = (uint32_t)c.total;
        c.total += c.h_slice[i];
        if (c.total >= c.hooks.max_cand) PBA_FAIL(PBA_E_TOOLONG, kTooManyCandidates);
        if (c.h_slice[i] <= PBA_IX_LDS_SORT_CAP) c.biggest_small = std::max(c.biggest_small, c.h_slice[i]);
        else c.big.push_back(i);
    }
    c.h_off[nt] = (uint32_t)c.total;
    HIPCHK(hipMemcpyAsync(c.d_off.p, c.h_off.data(), sizeof(uint32_t) * (nt + 1), hipMemcpyHostToDevice, ctx->stream));
    POOL(POOL_OVL_CAND, sizeof(uint64_t) * (c.total + 1), c.d_cand.p);
    // the candidates (all-ones where a slot belongs to the target's own probe or to another key)
    if (c.total) {
        PBA_PT_LAUNCH(c.tab->hashed, k_ovl_fill, dim3(nt), block, 0, ctx->stream, c.T, c.reads->dev(), c.t_lo, nt, c.d_off.as<uint32_t>(),
                      c.d_cand.as<uint64_t>(), c.d_valid.as<uint32_t>());
        HIPCHK(hipMemcpyAsync(c.h_valid.data(), c.d_valid.p, sizeof(uint32_t) * nt, hipMemcpyDeviceToHost, ctx->stream));
    } else {
        HIPCHK(hipMemsetAsync(c.d_valid.p, 0, sizeof(uint32_t) * (nt + 1), ctx->stream));
    }
    return PBA_OK;
}

// what k_seg_sort reported back, as sorted indices (a full list means "check everything")
static std::vector<uint32_t> listed(const uint32_t *ov, uint32_t ov_cap, uint64_t n_seg) {
    std::vector<uint32_t> v;
    if (ov[0] > ov_cap) { v.resize(n_seg); for (uint64_t i = 0; i < n_seg; ++i) v[i] = (uint32_t)i; }
    else v.assign(ov + 1, ov + 1 + ov[0]);
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

// In LDS, in place; the big ones (row-sweep form only) piece by piece through a second buffer.  What k_seg_sort reports
// back (a slice with one bucket beyond 256 entries, or beyond one workgroup) goes through the global bitonic pass.
static int ovl_sort_slices(OvlCall &c) {
    pba_ctx *ctx = c.ctx;
    const uint32_t nt = c.nt, ov_cap = 4096;
    uint64_t *const cand = c.d_cand.as<uint64_t>();
    DevBuf d_ov;
    HIPCHK(hipMalloc(&d_ov.p, sizeof(uint32_t) * (1 + ov_cap) * 2));
    uint32_t *const ov_small = d_ov.as<uint32_t>(), *const ov_piece = ov_small + 1 + ov_cap;
    HIPCHK(hipMemsetAsync(d_ov.p, 0, sizeof(uint32_t) * (1 + ov_cap) * 2, ctx->stream));
    std::vector<SegRef> h_pieces;
    if (c.fused) {
        // (equal-room slices have gaps: the segments are given one by one)
        std::vector<SegRef> h_seg(nt);
        uint32_t biggest = 2;
        for (uint32_t i = 0; i < nt; ++i) { h_seg[i] = SegRef{c.h_off[i], c.h_valid[i]}; biggest = std::max(biggest, c.h_valid[i]); }
        BufRef d_seg;
        POOL(POOL_OVL_TMP, sizeof(SegRef) * ((size_t)nt + 1), d_seg.p);
        HIPCHK(hipMemcpyAsync(d_seg.p, h_seg.data(), sizeof(SegRef) * nt, hipMemcpyHostToDevice, ctx->stream));
        launch_seg_sort(ctx, cand, cand, nullptr, d_seg.as<SegRef>(), nt, std::min<uint32_t>(biggest, PBA_IX_LDS_SORT_CAP), seg_bkt_range(),
                        ov_small, ov_cap);
        HIPCHK(hipStreamSynchronize(ctx->stream));           // h_seg
    } else
        launch_seg_sort(ctx, cand, cand, c.d_off.as<uint32_t>(), nullptr, nt, c.big.empty() ? c.biggest_small : 0xFFFFFFFFu, seg_bkt_range(),
                        ov_small, ov_cap);
    if (!c.fused && !c.big.empty()) {
        c.st.n_big_targets = (uint32_t)c.big.size();
        DevBuf d_big, d_pieces, d_pc;
        BufRef d_tmp;
        const uint32_t sub_mul = (uint32_t)std::min<uint64_t>(0xFFFFFFFFull, ((uint64_t)PBA_OVL_SUB << 32) / c.reads->n);   // fine bucket = umulhi(q, sub_mul)
        POOL(POOL_OVL_TMP, sizeof(uint64_t) * (c.total + 1), d_tmp.p);
        HIPCHK(hipMalloc(&d_big.p, sizeof(uint32_t) * c.big.size()));
        HIPCHK(hipMalloc(&d_pieces.p, sizeof(OvlPiece) * c.big.size() * PBA_OVL_SUB));
        HIPCHK(hipMalloc(&d_pc.p, 8));
        HIPCHK(hipMemsetAsync(d_pc.p, 0, 8, ctx->stream));
        HIPCHK(hipMemcpyAsync(d_big.p, c.big.data(), sizeof(uint32_t) * c.big.size(), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_ovl_split, dim3((uint32_t)c.big.size()), dim3(1024), 0, ctx->stream, d_big.as<uint32_t>(), c.d_off.as<uint32_t>(),
                           cand, d_tmp.as<uint64_t>(), sub_mul, d_pieces.as<OvlPiece>(), d_pc.as<uint32_t>(), d_pc.as<uint32_t>() + 1);
        uint32_t h_pc[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(h_pc, d_pc.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipGetLastError());
        launch_seg_sort(ctx, d_tmp.as<uint64_t>(), cand, nullptr, d_pieces.as<SegRef>(), h_pc[0], 0xFFFFFFFFu, seg_bkt_range(), ov_piece, ov_cap);
        h_pieces.resize(h_pc[0]);
        HIPCHK(hipMemcpyAsync(h_pieces.data(), d_pieces.p, sizeof(SegRef) * h_pc[0], hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipGetLastError());
    }
    std::vector<uint32_t> h_ov((1 + ov_cap) * 2, 0);
    HIPCHK(hipMemcpyAsync(h_ov.data(), d_ov.p, sizeof(uint32_t) * (1 + ov_cap) * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    const std::vector<uint32_t> &h_n = c.fused ? c.h_valid : c.h_slice;
    for (uint32_t i : listed(h_ov.data(), ov_cap, nt))       // slices with an overfull bucket, or beyond one workgroup (the row-sweep form cuts those into pieces)
        if (h_n[i] > 1 && (c.fused || h_n[i] <= PBA_IX_LDS_SORT_CAP)) PBA_TRY(sort_partition_global(ctx, cand + c.h_off[i], h_n[i]));
    for (uint32_t i : listed(h_ov.data() + 1 + ov_cap, ov_cap, h_pieces.size()))   // pieces beyond one sort, or with an overfull bucket
        if (i < h_pieces.size() && h_pieces[i].n > 1) PBA_TRY(sort_partition_global(ctx, cand + h_pieces[i].off, h_pieces[i].n));
    return PBA_OK;
}

// Work items of the walk: (target, first candidate of a group of 64), expanded on the device from the per-target item counts
// (building and copying 22 M of them from the host took longer than a scan pass); the device lists of rows and parked runs
static int ovl_make_items(OvlCall &c, uint64_t n_valid) {
    pba_ctx *ctx = c.ctx;
    const uint32_t nt = c.nt;
    // (the device list holds every success -- there are no more of them than listed candidates -- whatever the caller's cap:
    // k_ovl_after goes through all of them)
    c.dev_cap = c.fused ? std::max<uint64_t>(c.cap, n_valid) : c.cap;
    POOL(POOL_OVL_OUT, sizeof(pba_overlap) * (c.dev_cap + 1), c.d_out.p);
    HIPCHK(c.cnt_clear(CNT_OVERLAPS, 4));
    HIPCHK(hipMemsetAsync(ctx->d_queue, 0, 4, ctx->stream));
    // every (target, query) run can park at most once per stage, and there are no more runs than candidates
    c.redo_cap = std::max<uint64_t>(1024, n_valid);
    POOL(POOL_OVL_REDO, sizeof(uint2) * c.redo_cap, c.d_redo.p);
    std::vector<uint32_t> h_ipre(nt + 1);
    uint64_t n_items = 0;
    for (uint32_t i = 0; i < nt; ++i) { h_ipre[i] = (uint32_t)n_items; n_items += (c.h_valid[i] + PBA_WAVE - 1) / PBA_WAVE; }
    if (n_items >= 0xFFFFFFFFull) PBA_FAIL(PBA_E_TOOLONG, "pba_overlap_all: too many work items per call, use a smaller target range");
    h_ipre[nt] = (uint32_t)n_items;
    c.n_items = n_items;
    HIPCHK(hipMemcpyAsync(c.d_ipre.p, h_ipre.data(), sizeof(uint32_t) * (nt + 1), hipMemcpyHostToDevice, ctx->stream));
    POOL(POOL_OVL_ITEMS, sizeof(uint2) * (n_items + 1), c.d_items.p);
    if (n_items)
        hipLaunchKernelGGL(k_ovl_items, dim3((uint32_t)((n_items + 255) / 256)), dim3(256), 0, ctx->stream, c.d_ipre.as<uint32_t>(),
                           c.d_off.as<uint32_t>(), nt, (uint32_t)n_items, c.d_items.as<uint2>());
    HIPCHK(hipStreamSynchronize(ctx->stream));                   // h_ipre must outlive its copy
    return PBA_OK;
}

#define PBA_OVL_WALK_K(KERNEL, NBV, ...)                                                                              \
    hipLaunchKernelGGL((KERNEL<NBV>), dim3(persistent_grid(ctx, n_items, (NBV) ? 4 : 1, lds)),                        \
                       dim3(PBA_WAVE * ((NBV) ? 4 : 1)), lds * ((NBV) ? 4 : 1), ctx->stream, __VA_ARGS__, c.t_lo, n_items, \
                       items, c.d_off.as<uint32_t>(), c.d_valid.as<uint32_t>(), c.d_cand.as<uint64_t>(), c.ocfg, full_band, \
                       redo_in, c.d_redo.as<uint2>(), (unsigned long long)c.redo_cap, c.cnt(CNT_PARKED),              \
                       c.d_out.as<pba_overlap>(), (unsigned long long)c.dev_cap, c.cnt(CNT_OVERLAPS), c.cnt(CNT_PAIRS), \
                       ctx->d_queue)
#define PBA_OVL_WALK(NBV)                                                                                             \
    do {                                                                                                              \
        if (c.qset == c.reads) PBA_OVL_WALK_K(k_ovl_walk, NBV, c.reads->dev());                                       \
        else PBA_OVL_WALK_K(k_ovl_walk_rc, NBV, c.reads->dev(), c.qset->dev());                                       \
    } while (0)
// one launch of the walk in the ring nb: n_items entries of the group list `items` (redo_in == nullptr), or of parked runs
static int ovl_walk_once(OvlCall &c, int nb, const uint2 *items, uint32_t n_items, int full_band, const uint2 *redo_in) {
    pba_ctx *ctx = c.ctx;
    const size_t lds = c.pl.lds;
    HIPCHK(hipMemsetAsync(ctx->d_queue, 0, 4, ctx->stream));
    HIPCHK(c.cnt_clear(CNT_PARKED, 1));
    PBA_DISPATCH_NB(nb, PBA_OVL_WALK);
    HIPCHK(hipGetLastError());
    // the ctx profile of the most recent walk: its first launch, and the last one that resumed parked runs
    pba_profile &pr = ctx->prof;
    if (redo_in) { pr.nb_redo = (uint32_t)nb; pr.n_redo = n_items; }
    else if (!c.launched) { pr.nb_first = (uint32_t)nb; pr.n_first = n_items; }
    c.launched = true;
    return PBA_OK;
}

// items [lo, hi) in the ring nb_first with its first-pass window, then what that parked in the widest ring below the
// reference band's (its window takes all the room the ring has, bv_pass1_w: at 15 kb NB = 3 holds 4 072 of max_dst
// 4 501), then what is still parked at the reference band; *parked = the number parked by the first stage
static int ovl_narrow_then_redo(OvlCall &c, int nb_first, size_t lo, size_t hi, uint64_t *parked) {
    pba_ctx *ctx = c.ctx;
    *parked = 0;
    if (hi <= lo) return PBA_OK;
    PBA_TRY(ovl_walk_once(c, nb_first, c.d_items.as<uint2>() + lo, (uint32_t)(hi - lo), 0, nullptr));
    for (int stage = 0; stage < 2; ++stage) {
        unsigned long long h_redo = 0;
        HIPCHK(c.cnt_read(CNT_PARKED, 1, &h_redo));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (h_redo > c.redo_cap) PBA_FAIL(PBA_E_NOMEM, "pba_overlap_all: more uncertified (target, query) runs than the redo list holds");
        if (stage == 0) *parked = h_redo;
        if (!h_redo) return PBA_OK;
        if (stage == 0 && c.nb_mid <= nb_first) continue;    // no ring between this one and the reference band's
        BufRef d_in;
        POOL(POOL_OVL_REDO_IN, sizeof(uint2) * h_redo, d_in.p);
        HIPCHK(hipMemcpyAsync(d_in.p, c.d_redo.p, sizeof(uint2) * h_redo, hipMemcpyDeviceToDevice, ctx->stream));
        PBA_TRY(ovl_walk_once(c, stage == 0 ? c.nb_mid : c.pl.nb2, nullptr, (uint32_t)h_redo, /*full_band=*/stage == 1, d_in.as<uint2>()));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return PBA_OK;
}

// Whether the narrow window pays depends on how far the reads are from each other, which only the data tells: a sample of
// the items goes through narrow-then-redo, and if most of its successful runs had to be parked the rest starts wider.
static int ovl_walk(OvlCall &c) {
    pba_ctx *ctx = c.ctx;
    const Plan &pl = c.pl;
    for (int nb : {1, 2, 3, 4, 6})
        if (nb > pl.nb1 && nb < pl.nb2) c.nb_mid = nb;
    const size_t n_all = (size_t)c.n_items;
    // this call's decision: the hook's, or what a sample of an earlier range taught the table (never with a forced sample size)
    const int wide = c.hooks.wide >= 0 ? c.hooks.wide : tab_wide_decision(c.tab, c.ocfg.R, pl.nb1);
    const bool decided = wide >= 0 && !c.hooks.sample_min_set;
    const size_t n_sample = pl.nb1 == 0 ? n_all : (decided ? 0 : std::min(n_all, std::max<size_t>(c.hooks.sample_min, n_all / 32)));
    uint64_t parked = 0;
    PBA_TRY(ovl_narrow_then_redo(c, pl.nb1, 0, n_sample, &parked));
    uint64_t parked_total = parked;
    if (n_sample < n_all) {
        unsigned long long h_ov = 0;
        if (!decided) {
            HIPCHK(c.cnt_read(CNT_OVERLAPS, 1, &h_ov));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (n_sample >= 4096) tab_learn_wide(c.tab, 2 * parked_total > h_ov, c.ocfg.R, pl.nb1);   // a sample worth remembering
        }
        parked = 0;
        c.st.wide_first = (decided ? wide == 1 : 2 * parked_total > h_ov) ? 1 : 0;   // most overlaps of the sample needed more than the narrow window
        if (c.st.wide_first && !c.nb_mid) PBA_TRY(ovl_walk_once(c, pl.nb2, c.d_items.as<uint2>() + n_sample, (uint32_t)(n_all - n_sample), 1, nullptr));
        else PBA_TRY(ovl_narrow_then_redo(c, c.st.wide_first ? c.nb_mid : pl.nb1, n_sample, n_all, &parked));
        parked_total += parked;
    }
    c.st.n_redo = parked_total;
    HIPCHK(hipGetLastError());
    return PBA_OK;
}

// rows by (target, query): the walk's wavefronts emit in the order they finish.  A counting pass over the range's targets,
// then the few rows of a target by query (a comparison sort of the whole list was 12 ms per 200 000 rows on the host: a
// tenth of a 200 k-read pass)
static void order_rows_by_target_query(pba_overlap *out, uint64_t got, uint32_t t_lo, uint32_t nt) {
    if (got < 2) return;
    std::vector<uint32_t> first(nt + 1, 0);
    for (uint64_t i = 0; i < got; ++i) {
        const uint32_t tl = (uint32_t)out[i].target - t_lo;
        if (tl >= nt) {                                      // (a row outside the range: the plain sort)
            std::sort(out, out + got, [](const pba_overlap &x, const pba_overlap &y) {
                return x.target != y.target ? x.target < y.target : x.query < y.query;
            });
            return;
        }
        ++first[tl + 1];
    }
    for (uint32_t t = 0; t < nt; ++t) first[t + 1] += first[t];
    std::vector<pba_overlap> tmp(out, out + got);
    std::vector<uint32_t> at(first.begin(), first.end() - 1);
    for (uint64_t i = 0; i < got; ++i) out[at[(uint32_t)tmp[i].target - t_lo]++] = tmp[i];
    for (uint32_t t = 0; t < nt; ++t)
        if (first[t + 1] - first[t] > 1)
            std::sort(out + first[t], out + first[t + 1], [](const pba_overlap &x, const pba_overlap &y) { return x.query < y.query; });
}

// Pairs, rows, statistics.  Row-sweep form: the walk counted what it tried.  Fused form: the scan counted every candidate
// past the gate as a pair; what lies behind the first success of a run was never tried (overlap.h: k_ovl_after)
static int ovl_collect(OvlCall &c, pba_overlap *out, uint64_t *n_out) {
    pba_ctx *ctx = c.ctx;
    unsigned long long h_cnt[2] = {0, 0}, h_after = 0;
    HIPCHK(c.cnt_read(CNT_OVERLAPS, 2, h_cnt));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (c.fused && h_cnt[0]) {
        const uint32_t n_ov = (uint32_t)std::min<uint64_t>(h_cnt[0], c.dev_cap);
        PBA_PT_LAUNCH(c.tab->hashed, k_ovl_after, dim3((n_ov + 3) / 4), dim3(PBA_WAVE * 4), 0, ctx->stream, c.T, c.reads->dev(), c.qset->dev(),
                      c.d_out.as<pba_overlap>(), n_ov, c.T.mask, c.ocfg.t2, c.ocfg.overlap_min, c.cnt(CNT_AFTER_SUCCESS));
        HIPCHK(hipGetLastError());
        HIPCHK(c.cnt_read(CNT_AFTER_SUCCESS, 1, &h_after));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    (void)hipEventRecord(ctx->ev[5], ctx->stream);
    const uint64_t got = std::min<uint64_t>(h_cnt[0], c.cap);
    if (got) HIPCHK(hipMemcpyAsync(out, c.d_out.p, sizeof(pba_overlap) * got, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    order_rows_by_target_query(out, got, c.t_lo, c.nt);
    *n_out = h_cnt[0];
    c.st.n_overlaps = h_cnt[0];
    c.st.n_pairs = c.fused ? c.n_ok - h_after : h_cnt[1];
    (void)hipEventElapsedTime(&c.st.scan_ms, ctx->ev[2], ctx->ev[3]);
    (void)hipEventElapsedTime(&c.st.sort_ms, ctx->ev[3], ctx->ev[4]);
    (void)hipEventElapsedTime(&c.st.walk_ms, ctx->ev[4], ctx->ev[5]);
    return PBA_OK;
}

// targets [t_lo, t_hi) of `reads` against the probe table of the queries `qset` (reads itself, or a set of the same count and
// lengths whose bases the queries are walked with: pba_overlap_strands)
static int overlap_table(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *qset, uint32_t t_lo, uint32_t t_hi,
                         const pba_probe_table *tab, double R, int overlap_min, int kernel, pba_overlap *out, uint64_t cap,
                         uint64_t *n_out, pba_overlap_stats *stats) {
    if (!ctx || !reads || !qset || !tab || !n_out || (!out && cap) || t_lo > t_hi || t_hi > reads->n) return PBA_E_INVALID;
    if (qset->n != reads->n) return PBA_E_INVALID;
    if (reads->n >= PBA_OVL_MAX_READS) PBA_FAIL(PBA_E_TOOLONG, "pba_overlap_all: at most 2^24 reads");
    if ((uint64_t)reads->n * tab->t2 >= PBA_OVL_MAX_PROBES) PBA_FAIL(PBA_E_TOOLONG, "pba_overlap_all: reads x 2 x max_trial must stay below 2^32");
    if (reads->max_len > (uint32_t)kMaxSeqLen) PBA_FAIL(PBA_E_TOOLONG, "read longer than the engine limit");
    if (reads->non_acgt || qset->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_overlap_all: the read set holds bytes outside ACGT");
    HIPCHK(hipSetDevice(ctx->device));
    tu_attrs(ctx);
    *n_out = 0;
    OvlCall c;
    c.ctx = ctx; c.reads = reads; c.qset = qset; c.t_lo = t_lo; c.nt = t_hi - t_lo; c.tab = tab; c.T = tab_dev(tab); c.cap = cap;
    c.hooks = ovl_hooks_from_env();
    memset(&c.st, 0, sizeof c.st);
    ctx->prof.nb_first = ctx->prof.n_first = ctx->prof.nb_redo = ctx->prof.n_redo = 0;
    c.st.n_probe_entries = tab->n_entries;
    c.st.table_ms = tab->build_ms;
    const uint32_t nt = c.nt;
    if (nt == 0 || reads->n < 2) { if (stats) *stats = c.st; return PBA_OK; }
    PBA_TRY(make_plan(ctx, R, 0, 0, kernel, 1 + (int)(reads->max_len * R), &c.pl));
    c.fused = c.pl.nb1 != 0;
    c.ocfg.R = R; c.ocfg.overlap_min = overlap_min; c.ocfg.row_cap = c.pl.cfg.row_cap; c.ocfg.t2 = tab->t2;
    HIPCHK(hipMalloc(&c.d_cnt.p, 8 * CNT_SLOTS));
    HIPCHK(c.cnt_clear(CNT_OVERLAPS, CNT_SLOTS));
    uint32_t *d_small = nullptr;                             // room for five arrays of nt + 1, four in use
    POOL(POOL_OVL_SMALL, sizeof(uint32_t) * 5 * ((size_t)nt + 1), d_small);
    c.d_slice.p = d_small; c.d_off.p = d_small + ((size_t)nt + 1); c.d_valid.p = d_small + 2 * ((size_t)nt + 1); c.d_ipre.p = d_small + 3 * ((size_t)nt + 1);
    c.h_slice.resize(nt + 1); c.h_off.resize(nt + 1); c.h_valid.resize(nt + 1);
    (void)hipEventRecord(ctx->ev[2], ctx->stream);
    PBA_TRY(c.fused ? ovl_size_fused(c) : ovl_size_rowsweep(c));
    (void)hipEventRecord(ctx->ev[3], ctx->stream);
    if (c.total) PBA_TRY(ovl_sort_slices(c));
    (void)hipEventRecord(ctx->ev[4], ctx->stream);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipGetLastError());
    uint64_t n_valid = 0;
    for (uint32_t i = 0; i < nt; ++i) n_valid += c.h_valid[i];
    c.st.n_candidates = c.fused ? c.n_cand : n_valid;
    c.st.n_listed = n_valid;
    PBA_TRY(ovl_make_items(c, n_valid));
    PBA_TRY(ovl_walk(c));
    PBA_TRY(ovl_collect(c, out, n_out));
    if (stats) *stats = c.st;
    return PBA_OK;
}

extern "C" {
int pba_overlap_all_table(pba_ctx *ctx, const pba_seqs *reads, uint32_t t_lo, uint32_t t_hi, const pba_probe_table *tab, double R,
                          int overlap_min, int kernel, pba_overlap *out, uint64_t cap, uint64_t *n_out, pba_overlap_stats *stats) {
    return overlap_table(ctx, reads, reads, t_lo, t_hi, tab, R, overlap_min, kernel, out, cap, n_out, stats);
}

// ---------------------------------------------------------------------------------------------
// host API: both strands.  The -1 pass is the forward machinery with the queries' bases taken from the reverse complement
// of the reads (overlap.h: Q), against the probe table of that set; the rows of the two passes are merged and given
// intervals on the forward strand of each read.
// ---------------------------------------------------------------------------------------------
// a row of one pass -> a strand row.  Intervals from the accessors of spaced_seed.cpp:274-276 and ref_seq.h:282-286: forward,
// the target from the hit and the query from j; backward, the target up to hit + 16 and the query up to slen - j.  A -1 row's
// query interval is in the coordinates of rc(q) and is mapped back to q's forward strand.
static pba_strand_overlap strand_row(const pba_overlap &o, int strand, int qlen) {
    pba_strand_overlap r;
    r.target = o.target; r.query = o.query; r.strand = strand;
    r.j = o.j; r.dir = o.dir; r.ref_pos = o.ref_pos; r.cost = o.cost; r.matlen_a = o.matlen_a; r.matlen_b = o.matlen_b;
    int b0, b1;
    if (o.dir > 0) { r.t_beg = o.ref_pos; r.t_end = o.ref_pos + o.matlen_a; b0 = o.j; b1 = o.j + o.matlen_b; }
    else { r.t_beg = o.ref_pos + 16 - o.matlen_a; r.t_end = o.ref_pos + 16; b0 = qlen - o.j - o.matlen_b; b1 = qlen - o.j; }
    r.q_beg = strand > 0 ? b0 : qlen - b1;
    r.q_end = strand > 0 ? b1 : qlen - b0;
    return r;
}

int pba_overlap_strands_table(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                              const pba_probe_table *tab_fwd, const pba_probe_table *tab_rc, double R, int overlap_min,
                              int kernel, pba_strand_overlap *out, uint64_t cap, uint64_t *n_out, pba_overlap_stats stats[2]) {
    if (!ctx || !reads || !n_out || (!out && cap) || (!tab_fwd && !tab_rc) || (tab_rc && !reads_rc)) return PBA_E_INVALID;
    PBA_TRY(check_strand_sets(ctx, reads, reads_rc));
    *n_out = 0;
    pba_overlap_stats st[2];
    memset(st, 0, sizeof st);
    // (each pass may find up to cap rows; the rows are not initialised: at a million reads cap is tens of millions)
    std::unique_ptr<pba_overlap[]> rows[2];
    uint64_t n[2] = {0, 0};
    const pba_probe_table *tabs[2] = {tab_fwd, tab_rc};
    const pba_seqs *qsets[2] = {reads, reads_rc};
    for (int k = 0; k < 2; ++k) {
        if (!tabs[k]) continue;
        rows[k].reset(new (std::nothrow) pba_overlap[std::max<uint64_t>(cap, 1)]);
        if (!rows[k]) PBA_FAIL(PBA_E_NOMEM, "pba_overlap_strands: rows of a pass");
        PBA_TRY(overlap_table(ctx, reads, qsets[k], t_lo, t_hi, tabs[k], R, overlap_min, kernel, rows[k].get(), cap, &n[k], &st[k]));
    }
    // merge by (target, query), +1 before -1 (each pass is sorted by (target, query))
    const pba_overlap *a = rows[0].get(), *b = rows[1].get();
    const uint64_t na = std::min(n[0], cap), nb = std::min(n[1], cap);
    uint64_t i = 0, k = 0, o = 0;
    for (; o < cap && (i < na || k < nb); ++o) {
        const bool take_a = k >= nb || (i < na && (a[i].target != b[k].target ? a[i].target < b[k].target : a[i].query <= b[k].query));
        if (take_a) { out[o] = strand_row(a[i], 1, (int)reads->h_len[a[i].query]); ++i; }
        else { out[o] = strand_row(b[k], -1, (int)reads->h_len[b[k].query]); ++k; }
    }
    *n_out = n[0] + n[1];
    if (stats) { stats[0] = st[0]; stats[1] = st[1]; }
    return PBA_OK;
}

int pba_overlap_strands(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                        uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands,
                        pba_strand_overlap *out, uint64_t cap, uint64_t *n_out, pba_overlap_stats stats[2]) {
    if (!ctx || !reads || !n_out || (!out && cap)) return PBA_E_INVALID;
    if (strands < 1 || strands > 3) PBA_FAIL(PBA_E_INVALID, "pba_overlap_strands: strands must be 1 (+1), 2 (-1) or 3 (both)");
    PBA_TRY(check_strand_sets(ctx, reads, reads_rc));
    PBA_TRY(check_max_trial(ctx, max_trial));
    HIPCHK(hipSetDevice(ctx->device));
    struct Own {
        pba_seqs *rc = nullptr;
        pba_probe_table *tab[2] = {nullptr, nullptr};
        ~Own() { pba_probe_table_destroy(tab[0]); pba_probe_table_destroy(tab[1]); if (rc) pba_seqs_destroy(rc); }
    } own;
    if ((strands & 2) && !reads_rc) {
        PBA_TRY(pba_seqs_revcomp(ctx, reads, nullptr, &own.rc));
        reads_rc = own.rc;
    }
    if (strands & 1) PBA_TRY(own_table(ctx, reads, mask, max_trial, &own.tab[0]));
    if (strands & 2) PBA_TRY(own_table(ctx, reads_rc, mask, max_trial, &own.tab[1]));
    return pba_overlap_strands_table(ctx, reads, (strands & 2) ? reads_rc : nullptr, t_lo, t_hi, own.tab[0], own.tab[1], R,
                                     overlap_min, kernel, out, cap, n_out, stats);
}
}  // extern "C"
