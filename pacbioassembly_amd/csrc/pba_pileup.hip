// pba_pileup.hip -- read correction from overlap pile-ups: the vote boxes of MANY references at once (every read of a
// target range is one, csrc/consensus.h has the single-reference form), the segmented vote and evolve, and the driver
// that chains overlap -> vote -> evolve over a read set.  Host side and kernels.  The same boxes serve contigs: the
// drivers that polish a contig set from its mapped reads and that vote a layout's reads onto its contigs from their
// placements (pba_layout_consensus) are here too.  Mapped rows and placements vote through one gated vote
// (pile_vote_gated) and one anchor -> pair function; the three drivers share their run state (PileRun), the budget of a
// range and its greedy take, and the two contig drivers one round over the ranges of a contig set (contig_round).
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
// text leaves a pile-up, so those counts are not materialised.  A count pass (one workgroup per target) gives the new
// lengths, the host scans them, and a write pass puts every target's text at its final offset of one contiguous text,
// which pba_seqs_from_device_text packs.
#include "pba_host.h"
#include "qual.h"

#include <deque>
#include <memory>

// boxes of target t0 + blockIdx.x <- vote_box(base, weight), from the packed read
static __global__ void __launch_bounds__(256)
k_pile_fill(SeqSetDev S, uint32_t k0, VoteInto P, int weight) {
    const uint32_t k = k0 + blockIdx.x, t = P.t_lo + k;
    const uint8_t *seq = S.packed + S.off[t];
    const uint32_t len = S.len[t];
    const unsigned long long first = P.box_off[k];
    for (uint32_t i = threadIdx.x; i < len; i += 256) {
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

// The text of boxes [first, first + len) at out[0 ..), by one workgroup, 256 boxes per step.  A box yields at most two
// characters, so the offsets inside a step are two ballots and two popcounts per lane plus the totals of the wavefronts
// before it in LDS.
static __device__ __forceinline__ void pile_block_write(const ConsDev &C, unsigned long long first, unsigned long long len, char *out) {
    __shared__ int part[4];
    const int lane = threadIdx.x & (PBA_WAVE - 1), wave = threadIdx.x / PBA_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long done = 0;                               // characters written by the steps before this one
    for (unsigned long long base = 0; base < len; base += 256) {
        const unsigned long long i = base + threadIdx.x;
        unsigned long long sel = 0, sup = 0;
        int y = 0;
        if (i < len) { sel = C.sel[first + i]; sup = C.sup[first + i]; y = cons_yield(sel, sup, C.tot[first + i]); }
        const unsigned long long mv = __builtin_amdgcn_ballot_w64((y & 1) != 0), ms = __builtin_amdgcn_ballot_w64((y & 2) != 0);
        if (lane == 0) part[wave] = __builtin_popcountll(mv) + __builtin_popcountll(ms);
        __syncthreads();
        int before = __builtin_popcountll(mv & below) + __builtin_popcountll(ms & below);
        for (int w = 0; w < wave; ++w) before += part[w];
        const int step = part[0] + part[1] + part[2] + part[3];
        unsigned long long at = done + (unsigned long long)before;
        if (y & 1) out[at++] = cons_winner(sel);
        if (y & 2) out[at] = cons_winner(sup);                 // the split box sits right behind (ref_seq.h:328-334)
        done += (unsigned long long)step;
        __syncthreads();                                       // part[] is rewritten by the next step
    }
}

// count pass: len_out[k] = characters target k evolves to
static __global__ void __launch_bounds__(256)
k_pile_count(VoteInto P, uint32_t k0, int *len_out) {
    const uint32_t k = k0 + blockIdx.x;
    const unsigned long long first = P.box_off[k];
    const int n = pile_block_count(P.C, first, P.box_off[k + 1] - first);
    if (threadIdx.x == 0) len_out[k] = n;
}

// write pass: the text of target k at text[text_off[k] ..)
static __global__ void __launch_bounds__(256)
k_pile_write(VoteInto P, uint32_t k0, const unsigned long long *text_off, char *text) {
    const uint32_t k = k0 + blockIdx.x;
    const unsigned long long first = P.box_off[k];
    pile_block_write(P.C, first, P.box_off[k + 1] - first, text + text_off[k]);
}

// ---- long segments (a contig of megabases would keep ONE workgroup busy for tens of thousands of serial steps): the same
// three passes with one workgroup per TILE of kPileTile boxes.  tiles[]: (segment, first box inside it), made by the host
// (the precedent: the (contig, first chunk) table of k_seed_emit_set).  A tile's text goes to the offset the scan of the tile
// counts gives it -- a count, not a position, so a box's two characters stay side by side wherever the tile ends.
#define PBA_PILE_TILE 4096u
struct PileTile { uint32_t seg, first; };
static __device__ __forceinline__ unsigned long long pile_tile_len(const VoteInto &P, const PileTile &t) {
    const unsigned long long rest = P.box_off[t.seg + 1] - P.box_off[t.seg] - t.first;
    return rest < PBA_PILE_TILE ? rest : PBA_PILE_TILE;
}

static __global__ void __launch_bounds__(256)
k_pile_fill_tiles(SeqSetDev S, const PileTile *tiles, uint32_t tile0, VoteInto P, int weight) {
    const PileTile t = tiles[tile0 + blockIdx.x];
    const uint8_t *seq = S.packed + S.off[P.t_lo + t.seg];
    const unsigned long long first = P.box_off[t.seg];
    const uint32_t end = t.first + (uint32_t)pile_tile_len(P, t);
    for (uint32_t i = t.first + threadIdx.x; i < end; i += 256) {
        const int code = (seq[i >> 2] >> (6 - 2 * (i & 3))) & 3;
        P.C.sel[first + i] = cons_vote_box(code, weight);
        P.C.sup[first + i] = 0ull;
        P.C.tot[first + i] = 1;
    }
}

static __global__ void __launch_bounds__(256)
k_pile_count_tiles(VoteInto P, const PileTile *tiles, uint32_t tile0, int *tile_cnt) {
    const PileTile t = tiles[tile0 + blockIdx.x];
    const int n = pile_block_count(P.C, P.box_off[t.seg] + t.first, pile_tile_len(P, t));
    if (threadIdx.x == 0) tile_cnt[tile0 + blockIdx.x] = n;
}

static __global__ void __launch_bounds__(256)
k_pile_write_tiles(VoteInto P, const PileTile *tiles, uint32_t tile0, const unsigned long long *tile_off, char *text) {
    const PileTile t = tiles[tile0 + blockIdx.x];
    pile_block_write(P.C, P.box_off[t.seg] + t.first, pile_tile_len(P, t), text + tile_off[tile0 + blockIdx.x]);
}

// ---- the write pass with evidence (pba_pileup_evolve_qual; qual.h): pile_block_write's offsets, and for every
// character the record of the box it came from, in the one pass that reads the boxes.  i0: the position inside its segment of
// box `first`; at: where the block's first character goes in the text and in the four arrays of Q.
static __device__ __forceinline__ void pile_block_write_qual(const ConsDev &C, unsigned long long first, unsigned long long len, uint32_t i0,
                                                             char *text, const QualInto &Q, unsigned long long at0) {
    __shared__ int part[4];
    const int lane = threadIdx.x & (PBA_WAVE - 1), wave = threadIdx.x / PBA_WAVE;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long done = 0;
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
        unsigned long long at = at0 + done + (unsigned long long)before;
        if (y) {
            const uint64_t n = (uint64_t)(tot - 1) + (uint64_t)Q.weight;
            const uint16_t depth = (uint16_t)min(tot - 1, 65535);
            const uint32_t pos = i0 + (uint32_t)i;
            if (y & 1) {
                const int a = cons_max4(sel);
                text[at] = cons_winner(sel);
                Q.qv[at] = (uint8_t)qual_phred((uint32_t)a, n, Q.qmax); Q.depth[at] = depth; Q.agree[at] = (uint16_t)a; Q.src[at] = pos;
                ++at;
            }
            if (y & 2) {                                       // the split box sits right behind, as in pile_block_write
                const int a = cons_max4(sup);
                text[at] = cons_winner(sup);
                Q.qv[at] = (uint8_t)qual_phred((uint32_t)a, n, Q.qmax); Q.depth[at] = depth; Q.agree[at] = (uint16_t)a; Q.src[at] = pos | PBA_QUAL_SUP;
            }
        }
        done += (unsigned long long)step;
        __syncthreads();                                       // part[] is rewritten by the next step
    }
}

static __global__ void __launch_bounds__(256)
k_pile_write_qual(VoteInto P, uint32_t k0, const unsigned long long *text_off, char *text, QualInto Q) {
    const uint32_t k = k0 + blockIdx.x;
    const unsigned long long first = P.box_off[k];
    pile_block_write_qual(P.C, first, P.box_off[k + 1] - first, 0u, text, Q, text_off[k]);
}

static __global__ void __launch_bounds__(256)
k_pile_write_tiles_qual(VoteInto P, const PileTile *tiles, uint32_t tile0, const unsigned long long *tile_off, char *text, QualInto Q) {
    const PileTile t = tiles[tile0 + blockIdx.x];
    pile_block_write_qual(P.C, P.box_off[t.seg] + t.first, pile_tile_len(P, t), t.first, text, Q, tile_off[tile0 + blockIdx.x]);
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

// a launch's global size is a 32-bit number: one workgroup of 256 threads per target, at most 2^22 targets per launch
static const uint32_t kPileSlice = 1u << 22;
static const uint64_t kPileMaxBoxes = (1ull << 31) - 65536;
// A pile-up whose longest segment has more boxes than this runs the tiled kernels.  Above every read the engine accepts
// (kMaxSeqLen), so read pile-ups keep the per-target kernels.  (-DPBA_PILE_LONG_SEG=n: a tuning build, tools/build_variant.py,
// that keeps the per-target kernels up to n boxes, to compare the two forms on one input.)
#ifndef PBA_PILE_LONG_SEG
#define PBA_PILE_LONG_SEG 65536
#endif
static const uint64_t kPileLongSeg = PBA_PILE_LONG_SEG;
static const uint32_t kPileTile = PBA_PILE_TILE;
static_assert(PBA_PILE_LONG_SEG >= kMaxSeqLen, "read pile-ups keep the per-target kernels");

// the (segment, first box) table of a pile-up with a long segment, on the device; none (d_tiles stays null) otherwise
static int pile_make_tiles(pba_ctx *ctx, pba_pileup *p) {
    const uint32_t nt = p->t_hi - p->t_lo;
    uint64_t longest = 0, n_tiles = 0;
    for (uint32_t k = 0; k < nt; ++k) {
        const uint64_t len = p->box_off[k + 1] - p->box_off[k];
        longest = std::max(longest, len); n_tiles += (len + kPileTile - 1) / kPileTile;
    }
    if (longest <= kPileLongSeg) return PBA_OK;
    std::vector<PileTile> tiles;
    tiles.reserve((size_t)n_tiles);
    for (uint32_t k = 0; k < nt; ++k)
        for (uint64_t at = 0, len = p->box_off[k + 1] - p->box_off[k]; at < len; at += kPileTile) tiles.push_back(PileTile{k, (uint32_t)at});
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
    for (uint32_t k0 = 0; !p->d_tiles && k0 < nt && e == hipSuccess; k0 += kPileSlice) {
        hipLaunchKernelGGL(k_pile_fill, dim3(std::min(kPileSlice, nt - k0)), dim3(256), 0, ctx->stream, reads->dev(), k0, P, weight);
        e = hipGetLastError();
    }
    for (uint32_t k0 = 0; p->d_tiles && k0 < p->n_tiles && e == hipSuccess; k0 += kPileSlice) {
        hipLaunchKernelGGL(k_pile_fill_tiles, dim3(std::min(kPileSlice, p->n_tiles - k0)), dim3(256), 0, ctx->stream, reads->dev(),
                           p->d_tiles, k0, P, weight);
        e = hipGetLastError();
    }
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

// a pile-up evolved to one contiguous device text: target k at text[off[k] .. off[k+1]); d_off: off on the device (nt + 1 u64)
// qmax >= 0: evolve also writes the evidence of every character (qual.h), one entry per text byte
struct PileText {
    DevBuf text, d_off;
    std::vector<uint64_t> off;
    int qmax = -1;
    DevBuf qv, depth, agree, src;
};

// count pass: len_out[k] of every target; tiled form: also tile_off[i], where tile i's text starts inside the one text
// (the scan runs on the host, which needs the lengths anyway: 2^31 boxes are 524 288 tiles)
static int pile_count(pba_ctx *ctx, const pba_pileup *p, std::vector<int32_t> *len_out, std::vector<uint64_t> *tile_off) {
    const uint32_t nt = p->t_hi - p->t_lo, n = p->d_tiles ? p->n_tiles : nt;
    const VoteInto P = p->view();
    DevBuf d_cnt;
    std::vector<int32_t> cnt(n, 0);
    HIPCHK(hipMalloc(&d_cnt.p, sizeof(int32_t) * ((size_t)n + 1)));
    for (uint32_t k0 = 0; k0 < n; k0 += kPileSlice) {
        const dim3 grid(std::min(kPileSlice, n - k0));
        if (p->d_tiles) hipLaunchKernelGGL(k_pile_count_tiles, grid, dim3(256), 0, ctx->stream, P, p->d_tiles, k0, d_cnt.as<int>());
        else hipLaunchKernelGGL(k_pile_count, grid, dim3(256), 0, ctx->stream, P, k0, d_cnt.as<int>());
    }
    HIPCHK(hipGetLastError());
    if (n) HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (!p->d_tiles) { len_out->swap(cnt); return PBA_OK; }
    len_out->assign(nt, 0);
    tile_off->assign((size_t)n + 1, 0);
    uint32_t i = 0;                                            // the tiles lie in segment order, a segment's in box order
    for (uint32_t k = 0; k < nt; ++k)
        for (uint64_t at = 0, len = p->box_off[k + 1] - p->box_off[k]; at < len; at += kPileTile, ++i) {
            if ((uint64_t)(*len_out)[k] + (uint64_t)cnt[i] > 0x7FFFFFFFull) PBA_FAIL(PBA_E_TOOLONG, "pba_pileup_evolve: a segment evolves to 2^31 characters or more");
            (*len_out)[k] += cnt[i];
            (*tile_off)[i + 1] = (*tile_off)[i] + (uint64_t)cnt[i];
        }
    return PBA_OK;
}

// write pass: every target's text at T->off (already on the device as T->d_off), tile by tile at tile_off in the tiled form
static int pile_write(pba_ctx *ctx, const pba_pileup *p, const PileText *T, const std::vector<uint64_t> &tile_off) {
    const uint32_t nt = p->t_hi - p->t_lo, n = p->d_tiles ? p->n_tiles : nt;
    const VoteInto P = p->view();
    DevBuf d_toff;
    if (p->d_tiles) {
        HIPCHK(hipMalloc(&d_toff.p, sizeof(uint64_t) * tile_off.size()));
        HIPCHK(hipMemcpyAsync(d_toff.p, tile_off.data(), sizeof(uint64_t) * tile_off.size(), hipMemcpyHostToDevice, ctx->stream));
    }
    const QualInto Q{T->qv.as<uint8_t>(), T->depth.as<uint16_t>(), T->agree.as<uint16_t>(), T->src.as<uint32_t>(), p->weight, T->qmax};
    for (uint32_t k0 = 0; T->qmax >= 0 && k0 < n; k0 += kPileSlice) {
        const dim3 grid(std::min(kPileSlice, n - k0));
        if (p->d_tiles)
            hipLaunchKernelGGL(k_pile_write_tiles_qual, grid, dim3(256), 0, ctx->stream, P, p->d_tiles, k0, d_toff.as<unsigned long long>(),
                               T->text.as<char>(), Q);
        else
            hipLaunchKernelGGL(k_pile_write_qual, grid, dim3(256), 0, ctx->stream, P, k0, T->d_off.as<unsigned long long>(), T->text.as<char>(), Q);
    }
    for (uint32_t k0 = 0; T->qmax < 0 && k0 < n; k0 += kPileSlice) {
        const dim3 grid(std::min(kPileSlice, n - k0));
        if (p->d_tiles)
            hipLaunchKernelGGL(k_pile_write_tiles, grid, dim3(256), 0, ctx->stream, P, p->d_tiles, k0, d_toff.as<unsigned long long>(),
                               T->text.as<char>());
        else
            hipLaunchKernelGGL(k_pile_write, grid, dim3(256), 0, ctx->stream, P, k0, T->d_off.as<unsigned long long>(), T->text.as<char>());
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

// evolve to *T; the boxes are released
static int pile_evolve_text(pba_ctx *ctx, pba_pileup *p, PileText *T, pba_correct_row *rows_out) {
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
static int pile_text_qual(pba_ctx *ctx, PileText &T, uint32_t nt, pba_qual **qual) {
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
    if (st == PBA_E_INVALID && c.pile && c.pile->spent) {    // the engine's own rows did not re-run to themselves
        char keep[sizeof ctx->err];
        memcpy(keep, ctx->err, sizeof keep);
        snprintf(ctx->err, sizeof ctx->err, "pba_correct_reads: %.400s", keep);
        return PBA_E_HIP;
    }
    return st;
}

// The chunks' texts as one packed set of nt sequences.  One chunk: its text and device offsets as they are, no copy.
// Otherwise (none: an empty range) the texts side by side in one buffer under offsets that run through.
static int stitch_text(pba_ctx *ctx, std::deque<PileText> &chunks, uint32_t nt, uint64_t *n_bases_out, pba_seqs **out) {
    if (chunks.size() == 1) {
        const PileText &T = chunks[0];
        *n_bases_out = T.off.back();
        return pba_seqs_from_device_text(ctx, T.text.p, T.d_off.p, nt, T.off.back(), 0, out);
    }
    std::vector<uint64_t> all_off(1, 0);
    for (const PileText &T : chunks) {
        const uint64_t base = all_off.back();
        for (size_t k = 1; k < T.off.size(); ++k) all_off.push_back(base + T.off[k]);
    }
    DevBuf all, d_off;
    HIPCHK(hipMalloc(&all.p, all_off.back() + kSlack));
    uint64_t at = 0;
    for (const PileText &T : chunks) {
        if (T.off.back()) HIPCHK(copy_d2d((uint8_t *)all.p + at, T.text.p, T.off.back(), ctx->stream));
        at += T.off.back();
    }
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
    std::vector<uint64_t> all_off(1, 0);
    for (const PileText &T : chunks) {
        const uint64_t base = all_off.back();
        for (size_t k = 1; k < T.off.size(); ++k) all_off.push_back(base + T.off[k]);
    }
    static const size_t width[4] = {1, 2, 2, 4};
    DevBuf all[4];
    for (int a = 0; a < 4; ++a) HIPCHK(hipMalloc(&all[a].p, ((size_t)all_off.back() + 16) * width[a]));
    uint64_t at = 0;
    for (const PileText &T : chunks) {
        const void *from[4] = {T.qv.p, T.depth.p, T.agree.p, T.src.p};
        for (int a = 0; a < 4 && T.off.back(); ++a)
            HIPCHK(copy_d2d((uint8_t *)all[a].p + at * width[a], from[a], T.off.back() * width[a], ctx->stream));
        at += T.off.back();
    }
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
