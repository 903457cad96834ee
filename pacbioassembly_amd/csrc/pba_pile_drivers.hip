// pba_pile_drivers.hip -- the drivers over pile-ups (csrc/pba_pileup.hip): pba_correct_reads chains overlap -> vote ->
// evolve over a read set (pba_correct_reads_phased: with the rows of the other copy phased out between two votes),
// pba_polish_contigs polishes a contig set from its mapped reads round after round, and
// pba_layout_consensus votes a layout's reads onto its contigs from their placements.  Host code only: no kernel is
// launched from here, and the pile-up is reached through its public calls and through pile_evolve_text / PileText
// (pba_host.h).  The three drivers share their run state (PileRun), the budget of a range and its greedy take, the
// stitching of the ranges' texts and evidence, and the two contig drivers one round over the ranges of a contig set
// (contig_round).  Everything here fails loudly (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry
// points.
#include "pba_host.h"

#include <deque>

extern "C" {

// ---------------------------------------------------------------------------------------------
// pba_correct_reads: overlap -> vote -> evolve over a read set, in chunks of targets whose boxes fit the card
// ---------------------------------------------------------------------------------------------
static void stats_add(pba_overlap_stats &a, const pba_overlap_stats &b, bool first) {
    if (first) { a = b; return; }
    a.n_candidates += b.n_candidates; a.n_pairs += b.n_pairs; a.n_overlaps += b.n_overlaps; a.n_redo += b.n_redo;
    a.scan_ms += b.scan_ms; a.sort_ms += b.sort_ms; a.walk_ms += b.walk_ms; a.n_big_targets += b.n_big_targets;
    a.n_prefiltered += b.n_prefiltered; a.cap_fill += b.cap_fill; a.cap_overflow += b.cap_overflow; a.n_listed += b.n_listed;
    a.wide_first = std::max(a.wide_first, b.wide_first);
}

// what every driver below keeps across one call: the read sets, the pile-up of the range in hand, the texts evolved so far
struct PileRun {
    pba_ctx *ctx;
    const pba_seqs *reads, *reads_rc;            // reads_rc: the caller's, or `rc`
    pba_seqs *rc = nullptr;                      // owned: the reverse complement, the range's pile-up
    pba_pileup *pile = nullptr;
    StageClock clk;
    std::deque<PileText> chunks;                 // the evolved text of every range so far
    std::vector<pba_correct_row> crows;          // per contig (the contig drivers)
    int qmax = -1;                               // >= 0: the next chunks evolve with their evidence (the *_qual drivers)
    ~PileRun() { pba_pileup_destroy(pile); if (rc) pba_seqs_destroy(rc); }
    // the reverse complement of the reads, made once where the caller gave none
    int need_rc() {
        if (reads_rc) return PBA_OK;
        PBA_TRY(pba_seqs_revcomp(ctx, reads, nullptr, &rc));
        reads_rc = rc;
        return PBA_OK;
    }
    // the pile-up's boxes to the next text of `chunks` (and its rows of rows_out), timed into *ms; the pile-up is gone after it
    int evolve_chunk(float *ms, pba_correct_row *rows_out) {
        if (!chunks.empty()) chunks.back().d_off.reset();    // only the last chunk's offsets are used again (stitch_chunks)
        {
            const auto timed = clk.time(ctx->stream, ms);
            chunks.emplace_back();
            chunks.back().qmax = qmax;
            PBA_TRY(pile_evolve_text(ctx, pile, &chunks.back(), rows_out));
        }
        pba_pileup_destroy(pile); pile = nullptr;            // (host memory only by now: not part of the stage's time)
        return PBA_OK;
    }
};

// The boxes of one pile-up.  room: a quarter of the free memory at 20 bytes a box, fewer than kPileMaxBoxes; budget: room
// under max_boxes, where set, halved `shrink` times, one box at least.
struct PileBudget { uint64_t room, budget; };
static int pile_budget(pba_ctx *ctx, uint64_t max_boxes, uint32_t shrink, PileBudget *b) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    b->room = std::min<uint64_t>(kPileMaxBoxes - 1, (uint64_t)(free_b / 4) / 20);
    b->budget = std::max<uint64_t>(1, (max_boxes ? std::min(b->room, max_boxes) : b->room) >> shrink);
    return PBA_OK;
}

// sequences [lo, *hi) of S, below `end`, and their *boxes: consecutive ones while they fit the budget, one at least
static void pile_take(const pba_seqs *S, uint32_t lo, uint32_t end, uint64_t budget, uint32_t *hi, uint64_t *boxes) {
    *hi = lo; *boxes = 0;
    while (*hi < end && (*hi == lo || *boxes + S->h_len[*hi] <= budget)) *boxes += S->h_len[(*hi)++];
}

// what lives across one call of pba_correct_reads
struct CorrectRun : PileRun {
    uint32_t t_lo, t_hi;
    double R;
    int overlap_min, kernel, strands, weight;
    pba_probe_table *tab[2] = {nullptr, nullptr};   // owned
    pba_correct_profile prof;
    pba_overlap_stats tot[2];                    // summed over the chunks
    std::vector<pba_strand_overlap> rows;        // the chunk's overlaps (n_rows of them); grows to what a call reports
    uint64_t n_rows = 0;
    ~CorrectRun() { pba_probe_table_destroy(tab[0]); pba_probe_table_destroy(tab[1]); }
};

static int correct_check(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, int max_trial, int strands, int weight) {
    if (weight < 1 || weight > 0xFFFF) PBA_FAIL(PBA_E_INVALID, "pba_correct_reads: weight must be in [1, 65535]");
    if (strands < 1 || strands > 3) PBA_FAIL(PBA_E_INVALID, "pba_correct_reads: strands must be 1 (+1), 2 (-1) or 3 (both)");
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        PBA_FAIL(PBA_E_INVALID, "pba_correct_reads: reads_rc differs from reads in count or lengths");
    if (reads->non_acgt || (reads_rc && reads_rc->non_acgt)) PBA_FAIL(PBA_E_ALPHABET, "pba_correct_reads: the read set holds bytes outside ACGT");
    if (max_trial < 1 || max_trial > 63) PBA_FAIL(PBA_E_INVALID, "max_trial must be in [1, 63]");
    return PBA_OK;
}

// the reverse complement and the probe tables once, every chunk of targets against them
static int correct_prepare(CorrectRun &c, uint32_t mask, int max_trial) {
    pba_ctx *ctx = c.ctx;
    const auto timed = c.clk.time(ctx->stream, &c.prof.overlap_ms);
    if (c.strands & 2) PBA_TRY(c.need_rc());
    const pba_seqs *sets[2] = {c.reads, c.reads_rc};
    for (int s = 0; s < 2; ++s) {
        if (!(c.strands & (1 << s))) continue;
        const uint64_t pcap = (uint64_t)c.reads->n * 2u * (uint32_t)max_trial;
        DevBuf d_pent;
        HIPCHK(hipMalloc(&d_pent.p, sizeof(uint64_t) * (pcap + 1)));
        uint64_t n_pent = 0;
        PBA_TRY(pba_overlap_probes(ctx, sets[s], 0, c.reads->n, mask, max_trial, d_pent.p, pcap, &n_pent));
        PBA_TRY(pba_probe_table_create(ctx, d_pent.p, n_pent, mask, max_trial, &c.tab[s]));
    }
    return PBA_OK;
}

// Overlaps of the chunk into c.rows, which grows to what the call reports.  *halve: too many candidates for one call and
// the chunk holds more than one target -- the caller sizes it again at half the budget.
static int correct_overlaps(CorrectRun &c, uint32_t lo, uint32_t hi, bool *halve) {
    pba_ctx *ctx = c.ctx;
    const auto timed = c.clk.time(ctx->stream, &c.prof.overlap_ms);
    pba_overlap_stats cst[2];
    memset(cst, 0, sizeof cst);
    if (c.rows.size() < (size_t)(hi - lo) * 16 + 1024) c.rows.resize((size_t)(hi - lo) * 16 + 1024);
    int st;
    for (;;) {
        st = pba_overlap_strands_table(ctx, c.reads, (c.strands & 2) ? c.reads_rc : nullptr, lo, hi, c.tab[0], c.tab[1], c.R, c.overlap_min,
                                       c.kernel, c.rows.data(), c.rows.size(), &c.n_rows, cst);
        if (st != PBA_OK || c.n_rows <= c.rows.size()) break;
        c.rows.resize(c.n_rows + c.n_rows / 8);
    }
    *halve = (st == PBA_E_TOOLONG || st == PBA_E_NOMEM) && hi - lo > 1;
    if (st != PBA_OK) return st;
    stats_add(c.tot[0], cst[0], c.prof.n_chunks == 0); stats_add(c.tot[1], cst[1], c.prof.n_chunks == 0);
    return PBA_OK;
}

// the chunk's boxes and the votes of its rows
static int correct_vote(CorrectRun &c, uint32_t lo, uint32_t hi) {
    pba_ctx *ctx = c.ctx;
    int st;
    {
        const auto timed = c.clk.time(ctx->stream, &c.prof.vote_ms);
        st = pba_pileup_create(ctx, c.reads, lo, hi, c.weight, &c.pile);
        if (st == PBA_OK) st = pba_pileup_vote(ctx, c.pile, c.reads, c.reads_rc, c.rows.data(), c.n_rows, c.R, nullptr);
    }
    if (st == PBA_E_INVALID && c.pile) {
        char keep[sizeof ctx->err];
        PileView v;
        memcpy(keep, ctx->err, sizeof keep);
        if (pile_view(ctx, "pba_correct_reads", c.pile, &v) != PBA_OK) {   // spent (a live one leaves the message alone): the
            snprintf(ctx->err, sizeof ctx->err, "pba_correct_reads: %.400s", keep);   // engine's own rows did not re-run to themselves
            return PBA_E_HIP;
        }
    }
    return st;
}

// the offsets of every chunk's sequences in one text that runs through the chunks (the sequences of them all, plus one)
static std::vector<uint64_t> chunk_offsets(const std::deque<PileText> &chunks) {
    std::vector<uint64_t> all_off(1, 0);
    for (const PileText &T : chunks) {
        const uint64_t base = all_off.back();
        for (size_t k = 1; k < T.off.size(); ++k) all_off.push_back(base + T.off[k]);
    }
    return all_off;
}

// one array of every chunk (`width` bytes an entry, one entry per character) side by side at dst, in the chunks' order
static int chunks_side_by_side(pba_ctx *ctx, const std::deque<PileText> &chunks, DevBuf PileText::*arr, size_t width, void *dst) {
    uint64_t at = 0;
    for (const PileText &T : chunks) {
        if (T.off.back()) HIPCHK(copy_d2d((uint8_t *)dst + at * width, (T.*arr).p, T.off.back() * width, ctx->stream));
        at += T.off.back();
    }
    return PBA_OK;
}

// The chunks' texts as one packed set of nt sequences.  One chunk: its text and device offsets as they are, no copy.
// Otherwise (none: an empty range) the texts side by side in one buffer under offsets that run through.
static int stitch_text(pba_ctx *ctx, std::deque<PileText> &chunks, uint32_t nt, uint64_t *n_bases_out, pba_seqs **out) {
    if (chunks.size() == 1) {
        const PileText &T = chunks[0];
        *n_bases_out = T.off.back();
        return pba_seqs_from_device_text(ctx, T.text.p, T.d_off.p, nt, T.off.back(), 0, out);
    }
    const std::vector<uint64_t> all_off = chunk_offsets(chunks);
    DevBuf all, d_off;
    HIPCHK(hipMalloc(&all.p, all_off.back() + kSlack));
    PBA_TRY(chunks_side_by_side(ctx, chunks, &PileText::text, 1, all.p));
    if (!chunks.empty()) chunks.back().d_off.reset();
    HIPCHK(hipMalloc(&d_off.p, sizeof(uint64_t) * all_off.size()));
    HIPCHK(hipMemcpyAsync(d_off.p, all_off.data(), sizeof(uint64_t) * all_off.size(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    chunks.clear();
    *n_bases_out = all_off.back();
    return pba_seqs_from_device_text(ctx, all.p, d_off.p, nt, all_off.back(), 0, out);
}

// The chunks' evidence as one pba_qual of nt sequences, under the offsets stitch_text gives the texts.  One chunk: its arrays
// as they are.
static int stitch_qual(pba_ctx *ctx, std::deque<PileText> &chunks, uint32_t nt, pba_qual **qual) {
    if (chunks.size() == 1) return pile_text_qual(ctx, chunks[0], nt, qual);
    const std::vector<uint64_t> all_off = chunk_offsets(chunks);
    static const size_t width[4] = {1, 2, 2, 4};
    static DevBuf PileText::*const from[4] = {&PileText::qv, &PileText::depth, &PileText::agree, &PileText::src};
    DevBuf all[4];
    for (int a = 0; a < 4; ++a) HIPCHK(hipMalloc(&all[a].p, ((size_t)all_off.back() + 16) * width[a]));
    for (int a = 0; a < 4; ++a) PBA_TRY(chunks_side_by_side(ctx, chunks, from[a], width[a], all[a].p));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    void *arr[4] = {all[0].p, all[1].p, all[2].p, all[3].p};
    for (int a = 0; a < 4; ++a) all[a].p = nullptr;
    return qual_adopt(ctx, nt, all_off.data(), arr, qual);
}

// the texts, and where qual is asked for (every chunk evolved with its evidence) the evidence that belongs to them
static int stitch_chunks(pba_ctx *ctx, std::deque<PileText> &chunks, uint32_t nt, uint64_t *n_bases_out, pba_seqs **out,
                         pba_qual **qual = nullptr) {
    if (!qual) return stitch_text(ctx, chunks, nt, n_bases_out, out);
    PBA_TRY(stitch_qual(ctx, chunks, nt, qual));
    const int st = stitch_text(ctx, chunks, nt, n_bases_out, out);
    if (st != PBA_OK) { pba_qual_destroy(*qual); *qual = nullptr; }
    return st;
}

static int correct_stitch(CorrectRun &c, pba_seqs **corrected, pba_qual **qual) {
    const auto timed = c.clk.time(c.ctx->stream, &c.prof.evolve_ms);
    return stitch_chunks(c.ctx, c.chunks, c.t_hi - c.t_lo, &c.prof.n_bases_out, corrected, qual);
}

int pba_correct_reads(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                      uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                      pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2]) {
    return pba_correct_reads_budget(ctx, reads, reads_rc, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, strands, weight, 0,
                                    corrected, rows_out, stats);
}

// pba_correct_reads_budget, and with qual non-null pba_correct_reads_qual: every chunk evolves with its evidence at qmax
static int correct_run(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                       uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                       uint64_t max_boxes, pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2], int qmax,
                       pba_qual **qual) {
    if (!ctx || !reads || !corrected || t_lo > t_hi || t_hi > reads->n) return PBA_E_INVALID;
    *corrected = nullptr;
    PBA_TRY(correct_check(ctx, reads, reads_rc, max_trial, strands, weight));
    HIPCHK(hipSetDevice(ctx->device));
    CorrectRun c{{ctx, reads, reads_rc}, t_lo, t_hi, R, overlap_min, kernel, strands, weight};
    c.qmax = qual ? qmax : -1;
    if (!c.clk.init()) PBA_FAIL(PBA_E_HIP, "pba_correct_reads: events");
    memset(&c.prof, 0, sizeof c.prof);
    memset(c.tot, 0, sizeof c.tot);
    PBA_TRY(correct_prepare(c, mask, max_trial));
    uint32_t lo = t_lo, shrink = 0;                  // shrink: the chunk's box budget is halved this many times
    while (lo < t_hi) {
        uint32_t hi = lo;
        uint64_t boxes = 0;
        bool halve = false;
        PileBudget b;
        PBA_TRY(pile_budget(ctx, max_boxes, shrink, &b));
        pile_take(reads, lo, t_hi, b.budget, &hi, &boxes);   // (a read beyond b.room is left to pba_pileup_create)
        const int st = correct_overlaps(c, lo, hi, &halve);
        if (halve) { ++shrink; continue; }
        if (st != PBA_OK) return st;
        PBA_TRY(correct_vote(c, lo, hi));
        PBA_TRY(c.evolve_chunk(&c.prof.evolve_ms, rows_out ? rows_out + (lo - t_lo) : nullptr));
        c.prof.n_rows += c.n_rows; c.prof.n_bases_in += boxes; ++c.prof.n_chunks;
        lo = hi;
    }
    PBA_TRY(correct_stitch(c, corrected, qual));
    ctx->cprof = c.prof;
    if (stats) { stats[0] = c.tot[0]; stats[1] = c.tot[1]; }
    return PBA_OK;
}

int pba_correct_reads_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                             uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                             uint64_t max_boxes, pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2]) {
    return correct_run(ctx, reads, reads_rc, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, strands, weight, max_boxes, corrected,
                       rows_out, stats, -1, nullptr);
}

// ---- pba_correct_reads_phased: every target voted by the rows of its own copy only ----
struct PhaseGate { int min_depth, min_alt, min_permille; pba_phase_params params; int keep_unphased; pba_phase_stats tot; };

static void phase_stats_add(pba_phase_stats &a, const pba_phase_stats &b) {
    a.n_rows += b.n_rows; a.n_same += b.n_same; a.n_other += b.n_other; a.n_unphased += b.n_unphased; a.n_sites += b.n_sites;
    a.n_records += b.n_records; a.n_flipped_last += b.n_flipped_last; a.alleles_ms += b.alleles_ms; a.phase_ms += b.phase_ms;
}

// The chunk's rows narrowed to those that are not from the other copy: the sites of the pile-up all rows voted into (which is
// destroyed), the rows phased against them, c.rows / c.n_rows replaced by the rows kept.  The rows are the engine's own: one
// that does not re-run to itself is PBA_E_HIP, as in correct_vote.
static int correct_phase(CorrectRun &c, PhaseGate &g) {
    pba_ctx *ctx = c.ctx;
    const auto timed = c.clk.time(ctx->stream, &c.prof.vote_ms);
    pba_sites *sites = nullptr;
    PBA_TRY(pba_pileup_sites(ctx, c.pile, c.reads, g.min_depth, g.min_alt, g.min_permille, &sites));
    struct Guard { pba_sites *s; ~Guard() { pba_sites_destroy(s); } } guard{sites};
    pba_pileup_destroy(c.pile); c.pile = nullptr;
    std::vector<pba_phase_row> ph(std::max<uint64_t>(c.n_rows, 1));
    pba_phase_stats st;
    const int rc = pba_overlap_rows_phase(ctx, c.reads, c.reads_rc, c.rows.data(), c.n_rows, c.R, sites, &g.params, ph.data(), nullptr, &st,
                                          nullptr);
    if (rc == PBA_E_INVALID) {
        char keep[sizeof ctx->err];
        memcpy(keep, ctx->err, sizeof keep);
        snprintf(ctx->err, sizeof ctx->err, "pba_correct_reads_phased: %.400s", keep);
        return PBA_E_HIP;
    }
    PBA_TRY(rc);
    phase_stats_add(g.tot, st);
    const int64_t kept = pba_phase_rows_apply(c.rows.data(), ph.data(), c.n_rows, g.keep_unphased, c.rows.data());
    if (kept < 0) PBA_FAIL(PBA_E_HIP, "pba_correct_reads_phased: rows");
    c.n_rows = (uint64_t)kept;
    return PBA_OK;
}

int pba_correct_reads_phased_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                                    uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                                    uint64_t max_boxes, int min_depth, int min_alt, int min_permille, const pba_phase_params *params,
                                    int keep_unphased, pba_seqs **corrected, pba_correct_row *rows_out, pba_phase_stats *phase_stats,
                                    pba_overlap_stats stats[2]) {
    static const char who[] = "pba_correct_reads_phased";
    if (!ctx || !reads || !corrected || !params || t_lo > t_hi || t_hi > reads->n) return PBA_E_INVALID;
    *corrected = nullptr;
    PBA_TRY(correct_check(ctx, reads, reads_rc, max_trial, strands, weight));
    if (min_depth < 1 || min_alt < 1 || min_permille < 0 || min_permille > 1000)
        return ctx_fail_as(ctx, PBA_E_INVALID, who, "min_depth and min_alt must be at least 1, min_permille in [0, 1000]");
    if (params->n_iter < 0 || params->n_iter > PBA_PHASE_MAX_ITER || params->min_margin < 1 || params->self_weight < 0 || params->self_weight > 0xFFFF)
        return ctx_fail_as(ctx, PBA_E_INVALID, who, "n_iter must be in [0, 64], min_margin at least 1, self_weight in [0, 65535]");
    HIPCHK(hipSetDevice(ctx->device));
    CorrectRun c{{ctx, reads, reads_rc}, t_lo, t_hi, R, overlap_min, kernel, strands, weight};
    PhaseGate g{min_depth, min_alt, min_permille, *params, keep_unphased, {}};
    if (!c.clk.init()) PBA_FAIL(PBA_E_HIP, "pba_correct_reads_phased: events");
    memset(&c.prof, 0, sizeof c.prof);
    memset(c.tot, 0, sizeof c.tot);
    memset(&g.tot, 0, sizeof g.tot);
    PBA_TRY(correct_prepare(c, mask, max_trial));
    uint32_t lo = t_lo, shrink = 0;                  // (the chunk loop of correct_run, with the phase between two votes)
    while (lo < t_hi) {
        uint32_t hi = lo;
        uint64_t boxes = 0;
        bool halve = false;
        PileBudget b;
        PBA_TRY(pile_budget(ctx, max_boxes, shrink, &b));
        pile_take(reads, lo, t_hi, b.budget, &hi, &boxes);
        const int st = correct_overlaps(c, lo, hi, &halve);
        if (halve) { ++shrink; continue; }
        if (st != PBA_OK) return st;
        PBA_TRY(correct_vote(c, lo, hi));
        PBA_TRY(correct_phase(c, g));
        PBA_TRY(correct_vote(c, lo, hi));
        PBA_TRY(c.evolve_chunk(&c.prof.evolve_ms, rows_out ? rows_out + (lo - t_lo) : nullptr));
        c.prof.n_rows += c.n_rows; c.prof.n_bases_in += boxes; ++c.prof.n_chunks;
        lo = hi;
    }
    PBA_TRY(correct_stitch(c, corrected, nullptr));
    ctx->cprof = c.prof;
    if (stats) { stats[0] = c.tot[0]; stats[1] = c.tot[1]; }
    if (phase_stats) *phase_stats = g.tot;
    return PBA_OK;
}

int pba_correct_reads_phased(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                             uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                             int min_depth, int min_alt, int min_permille, const pba_phase_params *params, int keep_unphased,
                             pba_seqs **corrected, pba_correct_row *rows_out, pba_phase_stats *phase_stats,
                             pba_overlap_stats stats[2]) {
    return pba_correct_reads_phased_budget(ctx, reads, reads_rc, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, strands, weight, 0,
                                           min_depth, min_alt, min_permille, params, keep_unphased, corrected, rows_out, phase_stats, stats);
}

// what every *_qual driver checks before anything happens
static int qual_args_ok(pba_ctx *ctx, const char *who, int qmax, pba_qual **qual) {
    if (!ctx || !qual) return PBA_E_INVALID;
    *qual = nullptr;
    if (qmax < 0 || qmax > PBA_QUAL_QMAX) return ctx_fail_as(ctx, PBA_E_INVALID, who, "qmax must be in [0, 60]");
    return PBA_OK;
}

int pba_correct_reads_qual(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                           uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                           uint64_t max_boxes, pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2], int qmax,
                           pba_qual **qual) {
    PBA_TRY(qual_args_ok(ctx, "pba_correct_reads_qual", qmax, qual));
    return correct_run(ctx, reads, reads_rc, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, strands, weight, max_boxes, corrected,
                       rows_out, stats, qmax, qual);
}

// ---------------------------------------------------------------------------------------------
// what the two contig drivers share: found rows by contig, and one round of ranges over a contig set
// ---------------------------------------------------------------------------------------------
// rows <- its found rows ordered by contig (stable: by read inside a contig); those of contig c: rows[first[c] .. first[c + 1])
extern "C++" template <class Row>
static void bucket_by_contig(std::vector<Row> &rows, uint32_t n_contigs, std::vector<uint64_t> &first) {
    first.assign((size_t)n_contigs + 1, 0);
    for (const Row &r : rows)
        if (r.found) ++first[(size_t)r.contig + 1];
    for (uint32_t k = 0; k < n_contigs; ++k) first[k + 1] += first[k];
    std::vector<Row> by(first.back());
    std::vector<uint64_t> at(first.begin(), first.end() - 1);
    for (const Row &r : rows)
        if (r.found) by[at[r.contig]++] = r;
    rows.swap(by);
}

struct RoundResult { uint64_t n_voted, n_bases_in, n_bases_out; uint32_t n_chunks; float vote_ms, evolve_ms; };

// One round over a contig set: pile-ups over consecutive ranges [lo, hi) under the budget (one contig at least, whatever
// max_boxes says -- but a single contig beyond what the card can hold is PBA_E_NOMEM), each created and voted with
// vote(first[lo], first[hi] - first[lo], &voted) -- the bucketed rows of its contigs -- then evolved into c.crows; the texts
// stitched into *out, with the round's evidence in *qual where that is asked for (c.qmax says at which cap).  vote_ms: create + vote; evolve_ms: evolve + stitch.  who: the public function that was called.
extern "C++" template <class Vote>
static int contig_round(PileRun &c, const char *who, const pba_seqs *contigs, int weight, uint64_t max_boxes,
                        const std::vector<uint64_t> &first, Vote vote, RoundResult *r, pba_seqs **out, pba_qual **qual = nullptr) {
    pba_ctx *ctx = c.ctx;
    const uint32_t nt = contigs->n;
    *r = RoundResult{};
    c.crows.assign(std::max<uint32_t>(nt, 1), pba_correct_row{});
    for (uint32_t lo = 0, hi = 0; lo < nt; lo = hi) {
        PileBudget b;
        uint64_t boxes = 0;
        PBA_TRY(pile_budget(ctx, max_boxes, 0, &b));
        pile_take(contigs, lo, nt, b.budget, &hi, &boxes);
        if (boxes > b.room) return ctx_fail_as(ctx, PBA_E_NOMEM, who, "the vote boxes of one contig do not fit the device");
        {
            const auto timed = c.clk.time(ctx->stream, &r->vote_ms);
            uint64_t voted = 0;
            PBA_TRY(pba_pileup_create(ctx, contigs, lo, hi, weight, &c.pile));
            PBA_TRY(vote(first[lo], first[hi] - first[lo], &voted));
            r->n_voted += voted;
        }
        PBA_TRY(c.evolve_chunk(&r->evolve_ms, c.crows.data() + lo));
        ++r->n_chunks;
    }
    for (uint32_t k = 0; k < nt; ++k) r->n_bases_in += contigs->h_len[k];
    {
        const auto timed = c.clk.time(ctx->stream, &r->evolve_ms);
        PBA_TRY(stitch_chunks(ctx, c.chunks, nt, &r->n_bases_out, out, qual));
    }
    c.chunks.clear();
    return PBA_OK;
}

// the per-contig rows of the last round as the contig drivers report them
static void polish_rows_out(const std::vector<pba_correct_row> &crows, uint32_t n, pba_polish_row *rows_out) {
    for (uint32_t k = 0; rows_out && k < n; ++k)
        rows_out[k] = pba_polish_row{crows[k].target, crows[k].n_rows, crows[k].len_in, crows[k].len_out};
}

// ---------------------------------------------------------------------------------------------
// pba_polish_contigs: index -> map -> vote -> evolve over a contig set, round after round
// ---------------------------------------------------------------------------------------------
// what lives across one call of pba_polish_contigs
struct PolishRun : PileRun {
    uint32_t mask;
    double R;
    int trials, min_len, maxn, maxm, kernel, strands, overlap_min, weight;
    uint64_t max_boxes;
    const pba_seqs *cur;                         // the round's contigs: the caller's target, then `own`
    pba_seqs *own = nullptr;                     // owned: the set the last round made, the index
    pba_index *ix = nullptr;
    pba_polish_round_log lg;                     // the round in progress
    std::vector<pba_map_row> rows;               // the round's rows, then its found rows ordered by contig
    std::vector<uint64_t> first;                 // found rows of contig c: rows[first[c] .. first[c + 1])
    ~PolishRun() { pba_index_destroy(ix); if (own) pba_seqs_destroy(own); }
};

static int polish_check(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, int strands, int weight,
                        int rounds) {
    if (rounds < 1) PBA_FAIL(PBA_E_INVALID, "pba_polish_contigs: rounds must be at least 1");
    if (weight < 1 || weight > 0xFFFF) PBA_FAIL(PBA_E_INVALID, "pba_polish_contigs: weight must be in [1, 65535]");
    if (strands < 1 || strands > 3) PBA_FAIL(PBA_E_INVALID, "pba_polish_contigs: strands must be 1 (+1), 2 (-1) or 3 (both)");
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        PBA_FAIL(PBA_E_INVALID, "pba_polish_contigs: reads_rc differs from reads in count or lengths");
    if (target->non_acgt || reads->non_acgt || (reads_rc && reads_rc->non_acgt))
        PBA_FAIL(PBA_E_ALPHABET, "pba_polish_contigs: a set holds bytes outside ACGT");
    return PBA_OK;
}

// the round's index and its rows; the found ones ordered by contig
static int polish_map(PolishRun &c) {
    pba_ctx *ctx = c.ctx;
    {
        const auto timed = c.clk.time(ctx->stream, &c.lg.index_ms);
        PBA_TRY(pba_index_build_set(ctx, c.cur, c.mask, &c.ix));
    }
    {
        const auto timed = c.clk.time(ctx->stream, &c.lg.map_ms);
        c.rows.assign(std::max<size_t>(c.reads->n, 1), pba_map_row{});
        PBA_TRY(pba_map_reads(ctx, c.ix, c.cur, c.reads, c.reads_rc, c.R, c.trials, c.min_len, c.maxn, c.maxm, c.kernel, c.strands,
                              c.rows.data(), nullptr));
    }
    pba_index_destroy(c.ix); c.ix = nullptr;
    bucket_by_contig(c.rows, c.cur->n, c.first);
    c.lg.n_mapped = (uint32_t)c.rows.size();
    return PBA_OK;
}

// one round: c.cur -> c.own (the set of the round before, if it was ours, is dropped)
static int polish_round(PolishRun &c, pba_qual **qual) {
    PBA_TRY(polish_map(c));
    RoundResult r;
    pba_seqs *next = nullptr;
    PBA_TRY(contig_round(c, "pba_polish_contigs", c.cur, c.weight, c.max_boxes, c.first, [&](uint64_t at, uint64_t n, uint64_t *voted) {
        return pba_pileup_vote_mapped(c.ctx, c.pile, c.cur, c.reads, c.reads_rc, c.rows.data() + at, n, c.R, c.overlap_min, nullptr, voted);
    }, &r, &next, qual));
    c.lg.n_voted = (uint32_t)r.n_voted; c.lg.n_chunks = r.n_chunks; c.lg.n_bases_in = r.n_bases_in; c.lg.n_bases_out = r.n_bases_out;
    c.lg.vote_ms = r.vote_ms; c.lg.evolve_ms = r.evolve_ms;
    if (c.own) pba_seqs_destroy(c.own);
    c.own = next; c.cur = next;
    return PBA_OK;
}

int pba_polish_contigs(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t mask, double R,
                       int trials, int min_len, int maxn, int maxm, int kernel, int strands, int overlap_min, int weight, int rounds,
                       pba_seqs **polished, pba_polish_row *rows_out, pba_polish_round_log *log, int log_cap) {
    return pba_polish_contigs_budget(ctx, target, reads, reads_rc, mask, R, trials, min_len, maxn, maxm, kernel, strands, overlap_min,
                                     weight, rounds, 0, polished, rows_out, log, log_cap);
}

// pba_polish_contigs_budget, and with qual non-null pba_polish_contigs_qual: the last round evolves with its evidence at qmax
static int polish_run(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t mask,
                      double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands, int overlap_min, int weight,
                      int rounds, uint64_t max_boxes, pba_seqs **polished, pba_polish_row *rows_out,
                      pba_polish_round_log *log, int log_cap, int qmax, pba_qual **qual) {
    if (!ctx || !target || !reads || !polished || (log_cap > 0 && !log)) return PBA_E_INVALID;
    *polished = nullptr;
    PBA_TRY(polish_check(ctx, target, reads, reads_rc, strands, weight, rounds));
    HIPCHK(hipSetDevice(ctx->device));
    PolishRun c{{ctx, reads, reads_rc}, mask, R, trials, min_len, maxn, maxm, kernel, strands, overlap_min, weight, max_boxes, target};
    if (!c.clk.init()) PBA_FAIL(PBA_E_HIP, "pba_polish_contigs: events");
    if (strands & 2) PBA_TRY(c.need_rc());
    for (int round = 0; round < rounds; ++round) {
        memset(&c.lg, 0, sizeof c.lg);
        c.lg.round = round + 1;
        const bool last = round == rounds - 1;
        c.qmax = qual && last ? qmax : -1;
        PBA_TRY(polish_round(c, last ? qual : nullptr));
        if (round < log_cap) log[round] = c.lg;
    }
    polish_rows_out(c.crows, c.cur->n, rows_out);
    *polished = c.own; c.own = nullptr;
    return PBA_OK;
}

int pba_polish_contigs_budget(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t mask,
                              double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands, int overlap_min, int weight,
                              int rounds, uint64_t max_boxes, pba_seqs **polished, pba_polish_row *rows_out,
                              pba_polish_round_log *log, int log_cap) {
    return polish_run(ctx, target, reads, reads_rc, mask, R, trials, min_len, maxn, maxm, kernel, strands, overlap_min, weight, rounds,
                      max_boxes, polished, rows_out, log, log_cap, -1, nullptr);
}

int pba_polish_contigs_qual(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t mask,
                            double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands, int overlap_min, int weight,
                            int rounds, uint64_t max_boxes, pba_seqs **polished, pba_polish_row *rows_out,
                            pba_polish_round_log *log, int log_cap, int qmax, pba_qual **qual) {
    PBA_TRY(qual_args_ok(ctx, "pba_polish_contigs_qual", qmax, qual));
    return polish_run(ctx, target, reads, reads_rc, mask, R, trials, min_len, maxn, maxm, kernel, strands, overlap_min, weight, rounds,
                      max_boxes, polished, rows_out, log, log_cap, qmax, qual);
}

// ---------------------------------------------------------------------------------------------
// pba_layout_consensus: stitch -> place -> vote -> evolve over a layout's contigs, one round
// ---------------------------------------------------------------------------------------------
// what lives across one call of pba_layout_consensus
struct LayConsRun : PileRun {
    pba_seqs *contigs = nullptr;                 // owned: the stitched set
    pba_layout_cons_stats st;
    std::vector<pba_place_row> places;           // one per read, then the found ones ordered by contig
    std::vector<uint64_t> first;                 // found placements of contig c: places[first[c] .. first[c + 1])
    ~LayConsRun() { if (contigs) pba_seqs_destroy(contigs); }
};

// the placements, the found ones ordered by contig; the reverse complement if one of them needs it
static int laycons_place(LayConsRun &c, const pba_layout *lay, const pba_strand_overlap *rows, uint64_t n_rows) {
    c.places.assign(std::max<size_t>(c.reads->n, 1), pba_place_row{});
    PBA_TRY(pba_layout_place(c.ctx, lay, c.reads, rows, n_rows, c.places.data(), c.reads->n, &c.st.place));
    bucket_by_contig(c.places, c.contigs->n, c.first);
    for (const pba_place_row &r : c.places)
        if (r.strand == -1) return c.need_rc();
    return PBA_OK;
}

// pba_layout_consensus, and with qual non-null pba_layout_consensus_qual: the round evolves with its evidence at qmax
static int laycons_run(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, const pba_seqs *reads_rc,
                       const pba_strand_overlap *rows, uint64_t n_rows, double R, int overlap_min, int weight, uint64_t max_boxes,
                       pba_seqs **consensus, pba_polish_row *rows_out, pba_layout_cons_stats *stats, int qmax, pba_qual **qual) {
    if (!ctx || !lay || !reads || !consensus || (!rows && n_rows)) return PBA_E_INVALID;
    *consensus = nullptr;
    if (weight < 1 || weight > 0xFFFF) PBA_FAIL(PBA_E_INVALID, "pba_layout_consensus: weight must be in [1, 65535]");
    if (!(R > 0.0) || !(R < 1.0)) PBA_FAIL(PBA_E_INVALID, "R must be in (0,1)");
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        PBA_FAIL(PBA_E_INVALID, "pba_layout_consensus: reads_rc differs from reads in count or lengths");
    if (reads->non_acgt || (reads_rc && reads_rc->non_acgt)) PBA_FAIL(PBA_E_ALPHABET, "pba_layout_consensus: a set holds bytes outside ACGT");
    HIPCHK(hipSetDevice(ctx->device));
    LayConsRun c{{ctx, reads, reads_rc}};
    c.qmax = qual ? qmax : -1;
    if (!c.clk.init()) PBA_FAIL(PBA_E_HIP, "pba_layout_consensus: events");
    memset(&c.st, 0, sizeof c.st);
    {
        const auto timed = c.clk.time(ctx->stream, &c.st.stitch_ms);
        PBA_TRY(pba_layout_stitch(ctx, lay, reads, &c.contigs));
    }
    PBA_TRY(laycons_place(c, lay, rows, n_rows));
    RoundResult r;
    PBA_TRY(contig_round(c, "pba_layout_consensus", c.contigs, weight, max_boxes, c.first, [&](uint64_t at, uint64_t n, uint64_t *voted) {
        return pba_pileup_vote_placed(ctx, c.pile, c.contigs, reads, c.reads_rc, c.places.data() + at, n, R, overlap_min, nullptr, voted);
    }, &r, consensus, qual));
    c.st.n_contigs = c.contigs->n;
    c.st.n_voted = r.n_voted; c.st.n_chunks = r.n_chunks; c.st.n_bases_in = r.n_bases_in; c.st.n_bases_out = r.n_bases_out;
    c.st.vote_ms = r.vote_ms; c.st.evolve_ms = r.evolve_ms;
    polish_rows_out(c.crows, c.contigs->n, rows_out);
    if (stats) *stats = c.st;
    return PBA_OK;
}

int pba_layout_consensus(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, const pba_seqs *reads_rc,
                         const pba_strand_overlap *rows, uint64_t n_rows, double R, int overlap_min, int weight, uint64_t max_boxes,
                         pba_seqs **consensus, pba_polish_row *rows_out, pba_layout_cons_stats *stats) {
    return laycons_run(ctx, lay, reads, reads_rc, rows, n_rows, R, overlap_min, weight, max_boxes, consensus, rows_out, stats, -1, nullptr);
}

int pba_layout_consensus_qual(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, const pba_seqs *reads_rc,
                              const pba_strand_overlap *rows, uint64_t n_rows, double R, int overlap_min, int weight, uint64_t max_boxes,
                              pba_seqs **consensus, pba_polish_row *rows_out, pba_layout_cons_stats *stats, int qmax, pba_qual **qual) {
    PBA_TRY(qual_args_ok(ctx, "pba_layout_consensus_qual", qmax, qual));
    return laycons_run(ctx, lay, reads, reads_rc, rows, n_rows, R, overlap_min, weight, max_boxes, consensus, rows_out, stats, qmax, qual);
}

}  // extern "C"
