// pba_pileup.hip -- the pile-ups: the vote boxes of MANY references at once (every read of a target range is one,
// csrc/consensus.h has the single-reference form), the segmented vote and evolve.  Host side and kernels.  The same boxes
// serve reads and contigs: mapped rows and placements vote through one gated vote (pile_vote_gated) and one anchor -> pair
// function.  The drivers that chain overlap -> vote -> evolve over a read set, polish a contig set from its mapped reads
// and vote a layout's reads onto its contigs are csrc/pba_pile_drivers.hip; they reach the boxes through the public calls
// and pile_evolve_text (pba_host.h).
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
//
// Box arena: sel[], sup[] (4 x u16 in a u64 each, A in bits 15:0, as ConsDev) and tot[] over all bases of the range, the
// segment of target t at box_off[t - t_lo] (u64 on the device; the host keeps the arena below 2^31 boxes so that the vote
// kernel's box indices stay ints).  20 bytes per base.  No 3*max_len margins and no second ping-pong set: nothing grows,
// and evolve writes only text.  No text byte per box either: the box of base i is filled straight from the packed read,
// the votes never read the text, and the winner of an evolved box comes from its counters.
// Votes: k_vote_pairs<NB, true, SEG = true> (pba_align.hip) through trace_batch with the arena as its VoteInto, strand +1 rows against `reads`, strand -1
// rows against `reads_rc`, both into the same arena.  Counters are u16 bumped with 32-bit atomics on their dword: a
// selection counter holds weight + votes <= 65 535 (beyond that it would carry into its neighbour, not wrap).
// Evolve: every box yields 0..2 characters -- winner(sel) if its selection holds a majority of tot, then winner(sup) if
// its suppliment does (cons_yield, the one rule k_cons_evolve applies too).  The reference also folds a deleted box's
// selection into the suppliment of the last box kept before it, which changes only the NEXT round's sup counters; only the
// text leaves a pile-up, so those counts are not materialised.
//
// Three kernels, each one workgroup of 256 threads per BLOCK of boxes: k_pile_fill makes the boxes from the packed
// sequence, k_pile_count (the count pass) counts the characters a block evolves to, the host scans the counts, and
// k_pile_write (the write pass) puts every block's text at its final offset of one contiguous text, which
// pba_seqs_from_device_text packs.  What a block is comes from one of two SOURCES, fixed at compile time:
//   SrcTargets  block b is all of segment b.  Right for reads: thousands of short segments.
//   SrcTiles    block b is tiles[b] = (segment, first box inside it), PBA_PILE_TILE boxes or what is left of the segment.
//               A contig of megabases would keep ONE workgroup busy for tens of thousands of serial steps.  The table is
//               made by the host (the precedent: the (contig, first chunk) table of k_seed_emit_set).
// Both index their counts and their text offsets by the block number.  A block's text goes to the offset the scan of the
// counts gives it -- a count, not a position, so a box's two characters stay side by side wherever a tile ends.  One long
// segment switches the whole pile-up to tiles (pile_with_src: the one place that picks).
// The write pass has one body, pile_block_write, which finds where every box's characters go and hands them to one of
// two EMITTERS: EmitText stores the one or two characters; EmitQual stores them and, for each, the record of the box it
// came from (pba_pileup_evolve_qual; qual.h), in the one pass that reads the boxes.
#include "pba_host.h"
#include "qual.h"

#include <memory>

// ---- the blocks: boxes [first, first + len) of segment seg, first counted inside the segment
struct PileSpan { uint32_t seg, first; unsigned long long len; };
#define PBA_PILE_TILE 4096u
struct PileTile { uint32_t seg, first; };

struct SrcTargets {
    static constexpr bool tiled = false;
    __device__ __forceinline__ PileSpan span(const VoteInto &P, uint32_t b) const { return PileSpan{b, 0u, P.box_off[b + 1] - P.box_off[b]}; }
};
struct SrcTiles {
    static constexpr bool tiled = true;
    const PileTile *tiles;
    __device__ __forceinline__ PileSpan span(const VoteInto &P, uint32_t b) const {
        const PileTile t = tiles[b];
        const unsigned long long rest = P.box_off[t.seg + 1] - (P.box_off[t.seg] + t.first);
        return PileSpan{t.seg, t.first, rest < PBA_PILE_TILE ? rest : PBA_PILE_TILE};
    }
};

// boxes of block b0 + blockIdx.x <- vote_box(base, weight), from the packed sequence
template <class Src>
static __global__ void __launch_bounds__(256)
k_pile_fill(SeqSetDev S, Src src, uint32_t b0, VoteInto P, int weight) {
    const PileSpan s = src.span(P, b0 + blockIdx.x);
    const uint8_t *seq = S.packed + S.off[P.t_lo + s.seg];
    const unsigned long long first = P.box_off[s.seg];
    const uint32_t end = s.first + (uint32_t)s.len;
    for (uint32_t i = s.first + threadIdx.x; i < end; i += 256) {
        const int code = (seq[i >> 2] >> (6 - 2 * (i & 3))) & 3;            // 2-bit code == C2I of the base
        P.C.sel[first + i] = cons_vote_box(code, weight);
        P.C.sup[first + i] = 0ull;
        P.C.tot[first + i] = 1;
    }
}

// characters boxes [first, first + len) evolve to, by one workgroup of 256 threads (the sum is returned to every thread)
static __device__ __forceinline__ int pile_block_count(const ConsDev &C, unsigned long long first, unsigned long long len) {
    __shared__ int part[4];
    int mine = 0;
    for (unsigned long long i = threadIdx.x; i < len; i += 256) {
        const int y = cons_yield(C.sel[first + i], C.sup[first + i], C.tot[first + i]);
        mine += (y & 1) + (y >> 1);
    }
    const int w = wave_sum_i32(mine);                          // every lane is here: the loop has ended for all of them
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0) part[threadIdx.x / PBA_WAVE] = w;
    __syncthreads();
    return part[0] + part[1] + part[2] + part[3];
}

// The characters of boxes [first, first + len) from text position at0 onwards, by one workgroup, 256 boxes per step.  A
// box yields at most two characters, so the offsets inside a step are two ballots and two popcounts per lane plus the
// totals of the wavefronts before it in LDS.  i0: the position inside its segment of box `first`.  Each character goes out
// through emit(at, counters, tot, pos): the character elected from `counters` of a box with `tot`, box pos of its segment,
// at text position `at` -- the selection's first, the split box's (pos | PBA_QUAL_SUP) right behind it (ref_seq.h:328-334).
template <class Emit>
static __device__ __forceinline__ void pile_block_write(const ConsDev &C, unsigned long long first, unsigned long long len, uint32_t i0,
                                                        unsigned long long at0, const Emit &emit) {
    __shared__ int part[4];
    const int lane = threadIdx.x & (PBA_WAVE - 1), wave = threadIdx.x / PBA_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long next = at0;                             // where the step's first character goes
    for (unsigned long long base = 0; base < len; base += 256) {
        const unsigned long long i = base + threadIdx.x;
        unsigned long long sel = 0, sup = 0;
        int y = 0, tot = 0;
        if (i < len) { sel = C.sel[first + i]; sup = C.sup[first + i]; tot = C.tot[first + i]; y = cons_yield(sel, sup, tot); }
        const unsigned long long mv = __builtin_amdgcn_ballot_w64((y & 1) != 0), ms = __builtin_amdgcn_ballot_w64((y & 2) != 0);
        if (lane == 0) part[wave] = __builtin_popcountll(mv) + __builtin_popcountll(ms);
        __syncthreads();
        int before = __builtin_popcountll(mv & below) + __builtin_popcountll(ms & below);
        for (int w = 0; w < wave; ++w) before += part[w];
        const int step = part[0] + part[1] + part[2] + part[3];
        unsigned long long at = next + (unsigned long long)before;
        const uint32_t pos = i0 + (uint32_t)i;
        if (y & 1) emit(at++, sel, tot, pos);
        if (y & 2) emit(at, sup, tot, pos | PBA_QUAL_SUP);
        next += (unsigned long long)step;
        __syncthreads();                                       // part[] is rewritten by the next step
    }
}

// a character alone
struct EmitText {
    char *text;
    __device__ __forceinline__ void operator()(unsigned long long at, unsigned long long counters, int, uint32_t) const { text[at] = cons_winner(counters); }
};

// a character and, in the four arrays of Q at the same index, the record of the box it came from
struct EmitQual {
    char *text;
    QualInto Q;
    __device__ __forceinline__ void operator()(unsigned long long at, unsigned long long counters, int tot, uint32_t src) const {
        const int a = cons_max4(counters);
        text[at] = cons_winner(counters);
        Q.qv[at] = (uint8_t)qual_phred((uint32_t)a, (uint64_t)(tot - 1) + (uint64_t)Q.weight, Q.qmax);
        Q.depth[at] = (uint16_t)min(tot - 1, 65535); Q.agree[at] = (uint16_t)a; Q.src[at] = src;
    }
};

// count pass: cnt[b] = characters block b evolves to
template <class Src>
static __global__ void __launch_bounds__(256)
k_pile_count(VoteInto P, Src src, uint32_t b0, int *cnt) {
    const uint32_t b = b0 + blockIdx.x;
    const PileSpan s = src.span(P, b);
    const int n = pile_block_count(P.C, P.box_off[s.seg] + s.first, s.len);
    if (threadIdx.x == 0) cnt[b] = n;
}

// write pass: the characters of block b from text position off[b] onwards
template <class Src, class Emit>
static __global__ void __launch_bounds__(256)
k_pile_write(VoteInto P, Src src, uint32_t b0, const unsigned long long *off, Emit emit) {
    const uint32_t b = b0 + blockIdx.x;
    const PileSpan s = src.span(P, b);
    pile_block_write(P.C, P.box_off[s.seg] + s.first, s.len, s.first, off[b], emit);
}

extern "C" {

struct pba_pileup {
    int device;
    uint32_t t_lo, t_hi, n_reads;
    int weight;
    bool spent;
    uint64_t n_boxes;
    VoteBoxes boxes;                    // the arena (no txt)
    unsigned long long *d_box_off;
    std::vector<uint64_t> box_off;      // nt + 1
    PileTile *d_tiles;                  // non-null: a segment is longer than kPileLongSeg and the tiled kernels serve (n_tiles of them)
    uint32_t n_tiles;
    std::vector<int32_t> n_rows;        // rows voted per target
    VoteInto view() const { return VoteInto{boxes.dev, 0, 0, 0, d_box_off, t_lo}; }
};

static void pile_free_boxes(pba_pileup *p) {
    p->boxes.release();
    if (p->d_box_off) (void)hipFree(p->d_box_off);
    if (p->d_tiles) (void)hipFree(p->d_tiles);
    p->d_box_off = nullptr; p->d_tiles = nullptr;
}

// a launch's global size is a 32-bit number: one workgroup of 256 threads per block, at most 2^22 blocks per launch
static const uint32_t kPileSlice = 1u << 22;
// n blocks in slices of kPileSlice: launch(grid, b0) for each, b0 the slice's first block
extern "C++" template <class Launch>
static void pile_slices(uint32_t n, Launch launch) {
    for (uint32_t b0 = 0; b0 < n; b0 += kPileSlice) launch(dim3(std::min(kPileSlice, n - b0)), b0);
}
// A pile-up whose longest segment has more boxes than this runs the tiled kernels.  Above every read the engine accepts
// (kMaxSeqLen), so read pile-ups keep the per-target kernels.  (-DPBA_PILE_LONG_SEG=n: a tuning build, tools/build_variant.py,
// that keeps the per-target kernels up to n boxes, to compare the two forms on one input.)
#ifndef PBA_PILE_LONG_SEG
#define PBA_PILE_LONG_SEG 65536
#endif
static const uint64_t kPileLongSeg = PBA_PILE_LONG_SEG;
static const uint32_t kPileTile = PBA_PILE_TILE;
static_assert(PBA_PILE_LONG_SEG >= kMaxSeqLen, "read pile-ups keep the per-target kernels");

// run(src) with the block source the kernels of p run over, and what it returns: the one place that picks the form.  Its
// blocks: p->n_tiles tiles where src.tiled, the targets of p otherwise.
extern "C++" template <class Run>
static auto pile_with_src(const pba_pileup *p, Run run) {
    if (p->d_tiles) return run(SrcTiles{p->d_tiles});
    return run(SrcTargets{});
}

// The tiles of p in the order of d_tiles and of everything indexed by tile: for every segment in order, every kPileTile
// boxes of it.  tile(segment, first box inside it) for each, until one returns false (then false).
extern "C++" template <class Tile>
static bool pile_each_tile(const pba_pileup *p, Tile tile) {
    for (uint32_t k = 0; k < p->t_hi - p->t_lo; ++k)
        for (uint64_t at = 0, len = p->box_off[k + 1] - p->box_off[k]; at < len; at += kPileTile)
            if (!tile(k, (uint32_t)at)) return false;
    return true;
}

// the (segment, first box) table of a pile-up with a long segment, on the device; none (d_tiles stays null) otherwise
static int pile_make_tiles(pba_ctx *ctx, pba_pileup *p) {
    const uint32_t nt = p->t_hi - p->t_lo;
    uint64_t longest = 0;
    for (uint32_t k = 0; k < nt; ++k) longest = std::max<uint64_t>(longest, p->box_off[k + 1] - p->box_off[k]);
    if (longest <= kPileLongSeg) return PBA_OK;
    std::vector<PileTile> tiles;
    tiles.reserve((size_t)(p->n_boxes / kPileTile) + nt);     // (full tiles, and at most one short one per segment)
    pile_each_tile(p, [&](uint32_t k, uint32_t at) { tiles.push_back(PileTile{k, at}); return true; });
    if (hipMalloc((void **)&p->d_tiles, sizeof(PileTile) * tiles.size()) != hipSuccess) {
        (void)hipGetLastError(); p->d_tiles = nullptr;
        PBA_FAIL(PBA_E_NOMEM, "pba_pileup_create: tile table");
    }
    p->n_tiles = (uint32_t)tiles.size();
    HIPCHK(hipMemcpy(p->d_tiles, tiles.data(), sizeof(PileTile) * tiles.size(), hipMemcpyHostToDevice));   // (tiles dies with this scope)
    return PBA_OK;
}

int pba_overlap_row_pair(const pba_strand_overlap *row, uint32_t target_len, uint32_t query_len, pba_pair *out) {
    if (!row || !out) return PBA_E_INVALID;
    if ((row->dir != 1 && row->dir != -1) || (row->strand != 1 && row->strand != -1)) return PBA_E_INVALID;
    if (row->target < 0 || row->query < 0 || row->j < 0 || row->ref_pos < 0) return PBA_E_INVALID;
    if (target_len > 0x7FFFFFFFu || query_len > 0x7FFFFFFFu) return PBA_E_INVALID;
    const int64_t tl = target_len, slen = query_len;
    if (row->j >= slen) return PBA_E_INVALID;                                  // b_len = slen - j >= 1
    if (row->dir == 1 ? row->ref_pos >= tl : (int64_t)row->ref_pos + 16 > tl) return PBA_E_INVALID;
    memset(out, 0, sizeof *out);
    out->a_seq = (uint32_t)row->target; out->b_seq = (uint32_t)row->query;
    row_accessors(row->dir, row->j, row->ref_pos, 0, (int)tl, 0, (int)slen, out);   // the whole target is the window
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
    p->d_box_off = nullptr; p->d_tiles = nullptr; p->n_tiles = 0;
    p->box_off.assign((size_t)nt + 1, 0);
    p->n_rows.assign(nt, 0);
    for (uint32_t k = 0; k < nt; ++k) p->box_off[k + 1] = p->box_off[k] + reads->h_len[t_lo + k];
    p->n_boxes = p->box_off[nt];
    if (p->n_boxes >= kPileMaxBoxes) PBA_FAIL(PBA_E_TOOLONG, "pba_pileup_create: 2^31 boxes or more in one pile-up: use a smaller target range");
    const size_t cap = (size_t)p->n_boxes + 64;
    const bool ok = p->boxes.alloc(cap, false) && hipMalloc((void **)&p->d_box_off, sizeof(uint64_t) * ((size_t)nt + 1)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); pile_free_boxes(p.get()); PBA_FAIL(PBA_E_NOMEM, "pba_pileup_create: vote boxes"); }
    hipError_t e = hipMemcpyAsync(p->d_box_off, p->box_off.data(), sizeof(uint64_t) * ((size_t)nt + 1), hipMemcpyHostToDevice, ctx->stream);
    const VoteInto P = p->view();
    const int tst = pile_make_tiles(ctx, p.get());
    if (tst != PBA_OK) { pile_free_boxes(p.get()); return tst; }
    pile_with_src(p.get(), [&](auto src) {
        pile_slices(src.tiled ? p->n_tiles : nt, [&](dim3 grid, uint32_t b0) {
            if (e != hipSuccess) return;
            hipLaunchKernelGGL(k_pile_fill<decltype(src)>, grid, dim3(256), 0, ctx->stream, reads->dev(), src, b0, P, weight);
            e = hipGetLastError();
        });
    });
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { pile_free_boxes(p.get()); return ctx_fail(ctx, PBA_E_HIP, "pba_pileup_create", e); }
    *out = p.release();
    return PBA_OK;
}

int pile_view(pba_ctx *ctx, const char *who, const pba_pileup *p, PileView *v) {
    if (p->spent) return ctx_fail_as(ctx, PBA_E_INVALID, who, "the pile-up is spent");
    *v = PileView{p->boxes.dev, p->d_box_off, p->box_off.data(), p->t_lo, p->t_hi, p->n_reads, p->weight, p->n_boxes};
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

// What every vote call checks before it looks at a row, in the order include/pba.h gives.  who: the public function that
// was called; target: the set the boxes were filled from (under pba_pileup_vote the reads themselves).
static int pile_vote_check(pba_ctx *ctx, const pba_pileup *p, const char *who, const pba_seqs *target, const pba_seqs *reads,
                           const pba_seqs *reads_rc, uint64_t n, double R) {
    if (p->spent) return ctx_fail_as(ctx, PBA_E_INVALID, who, "the pile-up is spent");
    if (!(R > 0.0) || !(R < 1.0)) PBA_FAIL(PBA_E_INVALID, "R must be in (0,1)");
    if (!pile_same_reads(p, target)) return ctx_fail_as(ctx, PBA_E_INVALID, who, "the target set is not the set of this pile-up");
    if (reads_rc && (reads_rc->n != reads->n || reads_rc->h_len != reads->h_len))
        return ctx_fail_as(ctx, PBA_E_INVALID, who, "reads_rc differs from reads in count or lengths");
    if (target->non_acgt || reads->non_acgt || (reads_rc && reads_rc->non_acgt))
        return ctx_fail_as(ctx, PBA_E_ALPHABET, who, "a set holds bytes outside ACGT");
    if (n > 0x7FFFFFFFull) return ctx_fail_as(ctx, PBA_E_INVALID, who, "too many rows in one call");
    return PBA_OK;
}

// The votes of a call: pairs[0] against B = fwd, pairs[1] against B = rc, two batches into the boxes of p (A: the set they
// were filled from), gated by overlap_min; after(s, results of batch s) once a batch has voted.
extern "C++" template <class After>
static int pile_vote_batches(pba_ctx *ctx, pba_pileup *p, const pba_seqs *A, const pba_seqs *fwd, const pba_seqs *rc,
                             const std::vector<pba_pair> pairs[2], double R, int overlap_min, After after) {
    HIPCHK(hipSetDevice(ctx->device));
    const VoteInto into = p->view();
    std::vector<pba_result> out;
    bool voted = false;                   // a batch of this call has gone through
    for (int s = 0; s < 2; ++s) {
        if (pairs[s].empty()) continue;
        out.resize(pairs[s].size());
        const int st = trace_batch(ctx, A, s ? rc : fwd, pairs[s].data(), pairs[s].size(), R, 0, 0, PBA_KERNEL_BITVEC, out.data(),
                                   TraceInto::votes(into, overlap_min));
        if (st != PBA_OK) {
            // PBA_E_TOOLONG / PBA_E_INVALID come from the plan and the pair checks, before any launch.  Anything else may have
            // left votes behind, and so has an earlier batch of this call: the boxes no longer say which rows they hold.
            if (voted || (st != PBA_E_TOOLONG && st != PBA_E_INVALID)) p->spent = true;
            return st;
        }
        voted = true;
        PBA_TRY(after(s, out));
    }
    return PBA_OK;
}

int pba_pileup_vote(pba_ctx *ctx, pba_pileup *p, const pba_seqs *reads, const pba_seqs *reads_rc,
                    const pba_strand_overlap *rows, uint64_t n, double R, pba_result *res) {
    if (!ctx || !p || !reads || (!rows && n)) return PBA_E_INVALID;
    PBA_TRY(pile_vote_check(ctx, p, "pba_pileup_vote", reads, reads, reads_rc, n, R));
    if (n == 0) return PBA_OK;
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
    // (the rows passed their OVERLAP_MIN gate when they were found: the walk votes whatever re-runs to success)
    return pile_vote_batches(ctx, p, reads, reads, reads_rc, pairs, R, 0, [&](int s, const std::vector<pba_result> &out) {
        for (size_t q = 0; q < out.size(); ++q) {
            const pba_strand_overlap &r = rows[which[s][q]];
            if (res) res[which[s][q]] = out[q];
            if (!walk_agrees(out[q], r.cost, r.matlen_a, r.matlen_b)) {
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
        return PBA_OK;
    });
}

// The pair of a read that votes from an anchor: base `pos` of the contig against base `j` of the read's text, from there
// onwards (dir +1) or backwards (dir -1, both accessors) to the end of the read.  The callers have checked the anchor
// against the lengths.
static int anchored_pair(int32_t contig, int32_t pos, int32_t read, int32_t j, int dir, uint32_t contig_len, uint32_t read_len,
                         double R, pba_pair *out) {
    const bool fwd = dir == 1;
    const int rem_a = fwd ? (int)(contig_len - (uint32_t)pos) : pos + 1;
    const int b_len = fwd ? (int)(read_len - (uint32_t)j) : j + 1;
    // align cuts a to b + max_dst itself whenever a is the longer side (seq_aligner.h:94-102): the same cut, made here
    const TextClip c = text_clip(rem_a, b_len, R);
    if (c.len_a > kMaxSeqLen || b_len > kMaxSeqLen) return PBA_E_TOOLONG;
    memset(out, 0, sizeof *out);
    out->a_seq = (uint32_t)contig; out->a_pos = pos; out->a_len = c.len_a;
    out->b_seq = (uint32_t)read; out->b_pos = j; out->b_len = b_len;
    out->flags = fwd ? 0u : (PBA_A_BACKWARD | PBA_B_BACKWARD);
    return PBA_OK;
}

int pba_map_row_pair(const pba_map_row *row, uint32_t contig_len, uint32_t read_len, double R, pba_pair *out) {
    if (!row || !out || !row->found || (row->strand != 1 && row->strand != -1)) return PBA_E_INVALID;
    if (!(R > 0.0) || !(R < 1.0) || row->contig < 0 || row->read < 0 || row->j < 0 || row->pos < 0) return PBA_E_INVALID;
    if (contig_len > 0x7FFFFFFFu || read_len > 0x7FFFFFFFu) return PBA_E_INVALID;
    if ((uint32_t)row->j >= read_len || (uint32_t)row->pos >= contig_len) return PBA_E_INVALID;
    return anchored_pair(row->contig, row->pos, row->read, row->j, 1, contig_len, read_len, R, out);
}

int pba_place_row_pair(const pba_place_row *row, uint32_t contig_len, uint32_t read_len, double R, pba_pair *out) {
    if (!row || !out || !row->found || (row->strand != 1 && row->strand != -1) || (row->dir != 1 && row->dir != -1)) return PBA_E_INVALID;
    if (!(R > 0.0) || !(R < 1.0) || row->contig < 0 || row->read < 0 || row->j < 0 || row->pos < 0) return PBA_E_INVALID;
    if (contig_len > 0x7FFFFFFFu || read_len > 0x7FFFFFFFu) return PBA_E_INVALID;
    if ((uint32_t)row->j >= read_len || (uint32_t)row->pos >= contig_len) return PBA_E_INVALID;
    return anchored_pair(row->contig, row->pos, row->read, row->j, row->dir, contig_len, read_len, R, out);
}

// Rows of reads anchored on the targets of p (pba_map_row, pba_place_row: the fields read here have one name in both), each
// through the pair make_pair gives it, under try_align's gate.  who: the public function that was called.
extern "C++" template <class Row>
static int pile_vote_gated(pba_ctx *ctx, pba_pileup *p, const char *who, const pba_seqs *target, const pba_seqs *reads,
                           const pba_seqs *reads_rc, const Row *rows, uint64_t n, double R, int overlap_min, pba_result *res,
                           uint64_t *n_voted, int (*make_pair)(const Row *, uint32_t, uint32_t, double, pba_pair *)) {
    if (!ctx || !p || !target || !reads || (!rows && n)) return PBA_E_INVALID;
    if (n_voted) *n_voted = 0;
    PBA_TRY(pile_vote_check(ctx, p, who, target, reads, reads_rc, n, R));
    std::vector<pba_pair> pairs[2];       // strand +1 (B = reads), strand -1 (B = reads_rc)
    std::vector<uint32_t> which[2];
    for (uint64_t k = 0; k < n; ++k) {
        const Row &r = rows[k];
        if (!r.found) continue;
        if (r.contig < 0 || (uint32_t)r.contig < p->t_lo || (uint32_t)r.contig >= p->t_hi)
            return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's contig is outside the pile-up's range");
        if (r.read < 0 || (uint32_t)r.read >= reads->n) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's read is not a read of the set");
        if (r.strand == -1 && !reads_rc) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a strand -1 row needs reads_rc");
        pba_pair pr;
        const int st = make_pair(&r, target->h_len[r.contig], reads->h_len[r.read], R, &pr);
        if (st == PBA_E_TOOLONG) return ctx_fail_as(ctx, PBA_E_TOOLONG, who, "a row's accessor is longer than the engine limit");
        if (st != PBA_OK) return ctx_fail_as(ctx, PBA_E_INVALID, who, "a row's strand or anchor is not valid for its sequences");
        const int s = r.strand == 1 ? 0 : 1;
        pairs[s].push_back(pr); which[s].push_back((uint32_t)k);
    }
    for (uint64_t k = 0; res && k < n; ++k)
        if (!rows[k].found) { memset(&res[k], 0, sizeof res[k]); res[k].rc = -1; }
    // try_align's gate (ref_seq.h:264-265).  No re-run check: this alignment has the contig as a, where the walk that
    // found the row had the read (a mapped row) or the target read (a placement), and runs to the end of the read.
    return pile_vote_batches(ctx, p, target, reads, reads_rc, pairs, R, overlap_min, [&](int s, const std::vector<pba_result> &out) {
        for (size_t q = 0; q < out.size(); ++q) {
            if (res) res[which[s][q]] = out[q];
            if (out[q].rc < 0 || out[q].matlen_a < overlap_min) continue;
            ++p->n_rows[(uint32_t)rows[which[s][q]].contig - p->t_lo];
            if (n_voted) ++*n_voted;
        }
        return PBA_OK;
    });
}

int pba_pileup_vote_mapped(pba_ctx *ctx, pba_pileup *p, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                           const pba_map_row *rows, uint64_t n, double R, int overlap_min, pba_result *res, uint64_t *n_voted) {
    return pile_vote_gated(ctx, p, "pba_pileup_vote_mapped", target, reads, reads_rc, rows, n, R, overlap_min, res, n_voted, pba_map_row_pair);
}

int pba_pileup_vote_placed(pba_ctx *ctx, pba_pileup *p, const pba_seqs *contigs, const pba_seqs *reads, const pba_seqs *reads_rc,
                           const pba_place_row *rows, uint64_t n, double R, int overlap_min, pba_result *res, uint64_t *n_voted) {
    return pile_vote_gated(ctx, p, "pba_pileup_vote_placed", contigs, reads, reads_rc, rows, n, R, overlap_min, res, n_voted, pba_place_row_pair);
}

int pba_pileup_dump(pba_ctx *ctx, const pba_pileup *p, uint32_t target, uint16_t *sel, uint16_t *sup, int32_t *tot, int cap,
                    int32_t *n) {
    if (!ctx || !p || !n || cap < 0 || (cap && (!sel || !sup || !tot)) || target < p->t_lo || target >= p->t_hi) return PBA_E_INVALID;
    if (p->spent) PBA_FAIL(PBA_E_INVALID, "pba_pileup_dump: the pile-up is spent");
    HIPCHK(hipSetDevice(ctx->device));
    const uint64_t first = p->box_off[target - p->t_lo];
    *n = (int32_t)(p->box_off[target - p->t_lo + 1] - first);
    return p->boxes.to_host(ctx, (size_t)first, std::min(*n, cap), sel, sup, tot);
}

// count pass: len_out[k] of every target; tiled form: also tile_off[i], where tile i's text starts inside the one text
// (the scan runs on the host, which needs the lengths anyway: 2^31 boxes are 524 288 tiles)
static int pile_count(pba_ctx *ctx, const pba_pileup *p, std::vector<int32_t> *len_out, std::vector<uint64_t> *tile_off) {
    return pile_with_src(p, [&](auto src) -> int {
        const uint32_t nt = p->t_hi - p->t_lo, n = src.tiled ? p->n_tiles : nt;
        const VoteInto P = p->view();
        DevBuf d_cnt;
        std::vector<int32_t> cnt(n, 0);
        HIPCHK(hipMalloc(&d_cnt.p, sizeof(int32_t) * ((size_t)n + 1)));
        pile_slices(n, [&](dim3 grid, uint32_t b0) {
            hipLaunchKernelGGL(k_pile_count<decltype(src)>, grid, dim3(256), 0, ctx->stream, P, src, b0, d_cnt.as<int>());
        });
        HIPCHK(hipGetLastError());
        if (n) HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (!src.tiled) { len_out->swap(cnt); return PBA_OK; }
        len_out->assign(nt, 0);
        tile_off->assign((size_t)n + 1, 0);
        uint32_t i = 0;
        const bool fits = pile_each_tile(p, [&](uint32_t k, uint32_t) {
            if ((uint64_t)(*len_out)[k] + (uint64_t)cnt[i] > 0x7FFFFFFFull) return false;
            (*len_out)[k] += cnt[i];
            (*tile_off)[i + 1] = (*tile_off)[i] + (uint64_t)cnt[i];
            ++i;
            return true;
        });
        if (!fits) PBA_FAIL(PBA_E_TOOLONG, "pba_pileup_evolve: a segment evolves to 2^31 characters or more");
        return PBA_OK;
    });
}

// write pass: every block's text at its offset of T->text -- a target's at T->off (already on the device as T->d_off), a
// tile's at tile_off -- and with it, where T asks for it, the evidence
static int pile_write(pba_ctx *ctx, const pba_pileup *p, const PileText *T, const std::vector<uint64_t> &tile_off) {
    return pile_with_src(p, [&](auto src) -> int {
        typedef decltype(src) Src;
        const uint32_t n = src.tiled ? p->n_tiles : p->t_hi - p->t_lo;
        const VoteInto P = p->view();
        DevBuf d_toff;
        if (src.tiled) {
            HIPCHK(hipMalloc(&d_toff.p, sizeof(uint64_t) * tile_off.size()));
            HIPCHK(hipMemcpyAsync(d_toff.p, tile_off.data(), sizeof(uint64_t) * tile_off.size(), hipMemcpyHostToDevice, ctx->stream));
        }
        const unsigned long long *off = (const unsigned long long *)(src.tiled ? d_toff.p : T->d_off.p);
        const QualInto Q{T->qv.as<uint8_t>(), T->depth.as<uint16_t>(), T->agree.as<uint16_t>(), T->src.as<uint32_t>(), p->weight, T->qmax};
        pile_slices(n, [&](dim3 grid, uint32_t b0) {
            if (T->qmax >= 0)
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pile_write<Src, EmitQual>), grid, dim3(256), 0, ctx->stream, P, src, b0, off,
                                   EmitQual{T->text.as<char>(), Q});
            else
                hipLaunchKernelGGL(HIP_KERNEL_NAME(k_pile_write<Src, EmitText>), grid, dim3(256), 0, ctx->stream, P, src, b0, off,
                                   EmitText{T->text.as<char>()});
        });
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return PBA_OK;
    });
}

// evolve to *T; the boxes are released
int pile_evolve_text(pba_ctx *ctx, pba_pileup *p, PileText *T, pba_correct_row *rows_out) {
    if (p->spent) PBA_FAIL(PBA_E_INVALID, "pba_pileup_evolve: the pile-up is spent");
    HIPCHK(hipSetDevice(ctx->device));
    const uint32_t nt = p->t_hi - p->t_lo;
    std::vector<int32_t> len_out;
    std::vector<uint64_t> tile_off;
    PBA_TRY(pile_count(ctx, p, &len_out, &tile_off));
    T->off.assign((size_t)nt + 1, 0);
    for (uint32_t k = 0; k < nt; ++k) T->off[k + 1] = T->off[k] + (uint64_t)len_out[k];
    HIPCHK(hipMalloc(&T->text.p, T->off[nt] + kSlack));
    if (T->qmax >= 0) {
        const size_t nc = (size_t)T->off[nt] + 16;
        HIPCHK(hipMalloc(&T->qv.p, nc));
        HIPCHK(hipMalloc(&T->depth.p, nc * 2));
        HIPCHK(hipMalloc(&T->agree.p, nc * 2));
        HIPCHK(hipMalloc(&T->src.p, nc * 4));
    }
    HIPCHK(hipMalloc(&T->d_off.p, sizeof(uint64_t) * ((size_t)nt + 1)));
    HIPCHK(hipMemcpyAsync(T->d_off.p, T->off.data(), sizeof(uint64_t) * ((size_t)nt + 1), hipMemcpyHostToDevice, ctx->stream));
    PBA_TRY(pile_write(ctx, p, T, tile_off));
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
    PileText T;
    PBA_TRY(pile_evolve_text(ctx, p, &T, rows_out));
    return pba_seqs_from_device_text(ctx, T.text.p, T.d_off.p, p->t_hi - p->t_lo, T.off.back(), 0, corrected);
}

// the evidence arrays of T into a pba_qual of its nt sequences (they leave T)
int pile_text_qual(pba_ctx *ctx, PileText &T, uint32_t nt, pba_qual **qual) {
    void *arr[4] = {T.qv.p, T.depth.p, T.agree.p, T.src.p};
    T.qv.p = T.depth.p = T.agree.p = T.src.p = nullptr;
    return qual_adopt(ctx, nt, T.off.data(), arr, qual);
}

int pba_pileup_evolve_qual(pba_ctx *ctx, pba_pileup *p, int qmax, pba_seqs **corrected, pba_correct_row *rows_out, pba_qual **qual) {
    if (!ctx || !p || !corrected || !qual) return PBA_E_INVALID;
    *corrected = nullptr; *qual = nullptr;
    if (qmax < 0 || qmax > PBA_QUAL_QMAX) PBA_FAIL(PBA_E_INVALID, "pba_pileup_evolve_qual: qmax must be in [0, 60]");
    PileText T;
    T.qmax = qmax;
    const uint32_t nt = p->t_hi - p->t_lo;
    PBA_TRY(pile_evolve_text(ctx, p, &T, rows_out));
    PBA_TRY(pba_seqs_from_device_text(ctx, T.text.p, T.d_off.p, nt, T.off.back(), 0, corrected));
    const int st = pile_text_qual(ctx, T, nt, qual);
    if (st != PBA_OK) { pba_seqs_destroy(*corrected); *corrected = nullptr; }
    return st;
}

int pba_ctx_last_correct_profile(const pba_ctx *ctx, pba_correct_profile *out) {
    if (!ctx || !out) return PBA_E_INVALID;
    *out = ctx->cprof;
    return PBA_OK;
}

}  // extern "C"
