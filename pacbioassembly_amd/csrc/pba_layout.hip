// pba_layout.hip -- layout: reads into contigs from their overlap rows (pba_layout_*).  Host side and kernels.
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
//
// A best-overlap graph over pba_strand_overlap rows.  A read has two ENDS, e = 2 * read + side (side 0 its first base, side 1
// its last), and two STATES, s = 2 * read + orient (orient 0 walks the read as given: in at side 0, out at side 1; orient 1
// walks its reverse complement).  Numbered this way the entry end of state s is end s and its exit end is end s ^ 1, and
//   succ(s) = mate[s ^ 1]      (the mate's index IS the state that enters there)
//   pred(s) = mate[s] ^ 1
// so the chain structure is the mate array and nothing else.  Stages (one launch each unless said):
//   k_lay_classify   a lane per row: internal / containment / dovetail; container by u64 atomicMin of (row << 32 | outer)
//   k_lay_best       a lane per row: u64 atomicMax of (length, 0xFFFF - cost, ~row) at both ends of a surviving dovetail
//   k_lay_mate       a lane per end: mutual winners
//   k_lay_succ       a lane per state: skip / adv from the winning row at the predecessor's exit end, and the first hop
//   k_lay_jump       a lane per state, ceil(log2(2n)) launches, ping-pong: pointer, hops, bases before, smallest read seen
//   k_lay_cut        a lane per state: the state (m, 0) of a cycle's smallest read m cuts mate[2m] from both sides
//                    (k_lay_succ and the jumps then run again, only if some cycle was cut)
//   k_lay_chain      a lane per state: a tail tells its head the chain's reads and bases, and whether this direction is canonical
//   k_lay_place      a lane per read: its canonical state; head flags, reads and bases per head, for the host's scan
//   k_lay_table      a lane per read: its pba_layout_row, and its slot in the (contig, rank) order (a counting sort whose
//                    counts are the chains' read counts: slot = first slot of the contig + rank)
//   k_lay_stitch     a lane per 16 output bases: the supplying read by bisection over the slots' text offsets
// Placement (pba_layout_place), over any rows against a finished layout:
//   k_lay_pick       a lane per row: the anchor's contig coordinate (lay_anchor); u64 atomicMax of the best-edge key at the query
//   k_lay_emit       a lane per read: the winning row back out of the key, its anchor again, one pba_place_row
// Plain loads, vector stores and global atomics only; no LDS (nothing is shared inside a workgroup but the counters' sums).
#include "pba_host.h"

#include <memory>

#define PBA_LAY_NONE 0xFFFFFFFFFFFFFFFFull

enum { LAY_INTERNAL = 0, LAY_CONTAIN = 1, LAY_REFUSED = 2, LAY_DOVETAIL = 3 };
struct LayClass { int kind, a, b; };                          // CONTAIN: inner, outer read; DOVETAIL: t's end, q's end
enum { LC_INTERNAL = 0, LC_CONTAIN, LC_REFUSED, LC_DOVETAIL, LC_DROPPED, LC_MATED, LC_CYCLES, LC_CONTAINED, LC_COUNT };

static __device__ __forceinline__ LayClass lay_classify(const pba_strand_overlap &r, const uint32_t *len, int hang) {
    const int t = r.target, q = r.query, lt = (int)len[t], lq = (int)len[q];
    const int tb = r.t_beg, te = r.t_end;
    const int qb = r.strand == 1 ? r.q_beg : lq - r.q_end, qe = r.strand == 1 ? r.q_end : lq - r.q_beg;   // of the walked text
    const int tl = tb, tr = lt - te, ql = qb, qr = lq - qe;
    if (min(tl, ql) > hang || min(tr, qr) > hang) return LayClass{LAY_INTERNAL, 0, 0};
    const bool t_in_q = tl <= ql && tr <= qr, q_in_t = ql <= tl && qr <= tr;
    if (t_in_q || q_in_t) {
        const bool t_below = lt < lq || (lt == lq && t > q);  // rank(x) = (len[x], -x)
        int inner, outer;
        if (t_in_q && q_in_t) { inner = t_below ? t : q; outer = t_below ? q : t; }
        else if (t_in_q) { inner = t; outer = q; }
        else { inner = q; outer = t; }
        const bool ok = inner == t ? t_below : !t_below;
        return LayClass{ok ? LAY_CONTAIN : LAY_REFUSED, inner, outer};
    }
    if (tl > ql) return LayClass{LAY_DOVETAIL, 2 * t + 1, 2 * q + (r.strand == 1 ? 0 : 1)};
    return LayClass{LAY_DOVETAIL, 2 * t, 2 * q + (r.strand == 1 ? 1 : 0)};
}

// the sum of a per-lane count over the wavefront, added once to counters[which] (every lane of the wavefront is here)
static __device__ __forceinline__ void lay_count(unsigned long long *counters, int which, int mine) {
    const int w = wave_sum_i32(mine);
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0 && w) atomicAdd(&counters[which], (unsigned long long)w);
}

static __global__ void __launch_bounds__(256)
k_lay_classify(const pba_strand_overlap *rows, uint64_t n_rows, const uint32_t *len, int hang, unsigned long long *cont,
               unsigned long long *counters) {
    int c[4] = {0, 0, 0, 0};
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_rows; k += (uint64_t)gridDim.x * blockDim.x) {
        const LayClass cl = lay_classify(rows[k], len, hang);
        ++c[cl.kind];
        if (cl.kind == LAY_CONTAIN) atomicMin(&cont[cl.a], ((unsigned long long)k << 32) | (uint32_t)cl.b);
    }
    lay_count(counters, LC_INTERNAL, c[LAY_INTERNAL]); lay_count(counters, LC_CONTAIN, c[LAY_CONTAIN]);
    lay_count(counters, LC_REFUSED, c[LAY_REFUSED]); lay_count(counters, LC_DOVETAIL, c[LAY_DOVETAIL]);
}

static __device__ __forceinline__ unsigned long long lay_key(int span, int cost, uint64_t row) {
    const uint32_t c = (uint32_t)min(max(cost, 0), 0xFFFF);
    return ((unsigned long long)(uint32_t)span << 48) | ((unsigned long long)(0xFFFFu - c) << 32) | (unsigned long long)(~(uint32_t)row);
}
static __device__ __forceinline__ uint32_t lay_key_row(unsigned long long key) { return ~(uint32_t)key; }

static __global__ void __launch_bounds__(256)
k_lay_best(const pba_strand_overlap *rows, uint64_t n_rows, const uint32_t *len, int hang, const unsigned long long *cont,
           unsigned long long *best, unsigned long long *counters) {
    int dropped = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_rows; k += (uint64_t)gridDim.x * blockDim.x) {
        const pba_strand_overlap r = rows[k];
        const LayClass cl = lay_classify(r, len, hang);
        if (cl.kind != LAY_DOVETAIL) continue;
        if (cont[r.target] != PBA_LAY_NONE || cont[r.query] != PBA_LAY_NONE) { ++dropped; continue; }
        atomicMax(&best[cl.a], lay_key(r.t_end - r.t_beg, r.cost, k));
        atomicMax(&best[cl.b], lay_key(r.q_end - r.q_beg, r.cost, k));
    }
    lay_count(counters, LC_DROPPED, dropped);
}

// the end the winning row at end e leads to, or -1
static __device__ __forceinline__ int lay_lead(const pba_strand_overlap *rows, const uint32_t *len, int hang,
                                               const unsigned long long *best, int e) {
    const unsigned long long key = best[e];
    if (key == 0ull) return -1;                               // (a key holds a length >= 1: never 0)
    const LayClass cl = lay_classify(rows[lay_key_row(key)], len, hang);
    return cl.a == e ? cl.b : cl.a;
}

static __global__ void __launch_bounds__(256)
k_lay_mate(const pba_strand_overlap *rows, const uint32_t *len, int hang, const unsigned long long *best, int *mate, uint32_t n_ends,
           unsigned long long *counters) {
    int mated = 0;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < n_ends; e += gridDim.x * blockDim.x) {
        const int f = lay_lead(rows, len, hang, best, (int)e);
        const int m = f >= 0 && lay_lead(rows, len, hang, best, f) == (int)e ? f : -1;
        mate[e] = m;
        mated += m >= 0;
    }
    lay_count(counters, LC_MATED, mated);
}

struct LayGeom { int skip, adv; };
// state s supplies bases [skip, skip + adv) of its walked read: from the winning row at the exit end of its predecessor
static __device__ __forceinline__ LayGeom lay_geom(const pba_strand_overlap *rows, const uint32_t *len, const unsigned long long *best,
                                                  const int *mate, int s) {
    const int r = s >> 1, L = (int)len[r], x = mate[s];
    if (x < 0) return LayGeom{0, L};
    const pba_strand_overlap row = rows[lay_key_row(best[x])];
    const int b = row.target == r ? row.t_beg : row.q_beg, e = row.target == r ? row.t_end : row.q_end;
    const int skip = (s & 1) ? L - b : e;
    return LayGeom{skip, max(L - skip, 0)};
}

// what pointer jumping carries per state: ptr, the hops to it, the bases supplied by the states from ptr up to (not
// including) this one, and the smallest read id among the states after ptr up to this one
struct LayJump { int *ptr, *hops, *mn; unsigned long long *before; };

static __global__ void __launch_bounds__(256)
k_lay_succ(const pba_strand_overlap *rows, const uint32_t *len, const unsigned long long *best, const int *mate, int *skip, int *adv,
           LayJump J, int *canon, uint32_t n_states) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_states; s += gridDim.x * blockDim.x) {
        const LayGeom g = lay_geom(rows, len, best, mate, (int)s);
        skip[s] = g.skip; adv[s] = g.adv; canon[s] = 0;
        const int x = mate[s];
        J.mn[s] = (int)(s >> 1);
        if (x < 0) { J.ptr[s] = (int)s; J.hops[s] = 0; J.before[s] = 0ull; }
        else { J.ptr[s] = x ^ 1; J.hops[s] = 1; J.before[s] = (unsigned long long)lay_geom(rows, len, best, mate, x ^ 1).adv; }
    }
}

static __global__ void __launch_bounds__(256)
k_lay_jump(LayJump in, LayJump out, uint32_t n_states) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_states; s += gridDim.x * blockDim.x) {
        const int p = in.ptr[s];
        out.ptr[s] = in.ptr[p];
        out.hops[s] = in.hops[s] + in.hops[p];                // (a head points at itself with 0 hops and 0 bases: a fixed point)
        out.before[s] = in.before[s] + in.before[p];
        out.mn[s] = min(in.mn[s], in.mn[p]);
    }
}

// After the jumps a state whose pointer is not a head lies on a cycle, and its mn is the cycle's smallest read m.  The two
// directions of a cycle are disjoint sets of states; (m, 0) lies on one of them, and its lane alone cuts: mate[2m] and the
// end it was mated to.  No other lane's decision reads those two entries (they belong to this cycle and its reverse).
static __global__ void __launch_bounds__(256)
k_lay_cut(LayJump J, int *mate, uint32_t n_states, unsigned long long *counters) {
    for (uint32_t s = blockIdx.x * blockDim.x + threadIdx.x; s < n_states; s += gridDim.x * blockDim.x) {
        if ((s & 1) || J.mn[s] != (int)(s >> 1)) continue;
        const int f = mate[s];
        if (f < 0 || mate[J.ptr[s]] < 0) continue;            // a head, or a state a head reaches
        mate[s] = -1;
        mate[f] = -1;
        atomicAdd(&counters[LC_CYCLES], 1ull);
    }
}

// a tail t (no successor) tells its head what the chain holds; the other direction of the path starts at t ^ 1
static __global__ void __launch_bounds__(256)
k_lay_chain(LayJump J, const int *adv, const int *mate, int *canon, int *chain_reads, unsigned long long *chain_bases, uint32_t n_states) {
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_states; t += gridDim.x * blockDim.x) {
        if (mate[t ^ 1] >= 0) continue;
        const int h = J.ptr[t];
        canon[h] = (h >> 1) < (int)(t >> 1) || (h == (int)t && !(t & 1));
        chain_reads[h] = J.hops[t] + 1;
        chain_bases[h] = J.before[t] + (unsigned long long)adv[t];
    }
}

static __global__ void __launch_bounds__(256)
k_lay_place(LayJump J, const unsigned long long *cont, const int *canon, const int *chain_reads, const unsigned long long *chain_bases,
            int min_reads, int *pstate, int *head_reads, unsigned long long *head_bases, uint32_t n, unsigned long long *counters) {
    int contained = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        int s = -1, hr = 0;
        unsigned long long hb = 0ull;
        if (cont[r] != PBA_LAY_NONE) ++contained;
        else {
            s = canon[J.ptr[2 * r]] ? (int)(2 * r) : (int)(2 * r + 1);      // exactly one direction of a path is canonical
            if (J.ptr[s] == s && chain_reads[s] >= min_reads) { hr = chain_reads[s]; hb = chain_bases[s]; }
        }
        pstate[r] = s; head_reads[r] = hr; head_bases[r] = hb;             // head_reads > 0: r starts a contig
    }
    lay_count(counters, LC_CONTAINED, contained);
}

static __global__ void __launch_bounds__(256)
k_lay_table(LayJump J, const unsigned long long *cont, const int *pstate, const int *skip, const int *adv, const int *contig_of_head,
            const uint32_t *contig_slot, const unsigned long long *contig_text, pba_layout_row *table, int *slot_read,
            unsigned long long *slot_text, uint32_t n_slots, uint32_t n) {
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        pba_layout_row o;
        o.read = (int32_t)r; o.state = PBA_LAY_UNPLACED; o.contig = -1; o.rank = o.orient = o.offset = o.skip = o.adv = 0; o.container = -1;
        const int s = pstate[r];
        if (s < 0) { o.state = PBA_LAY_CONTAINED; o.container = (int32_t)(uint32_t)cont[r]; }
        else {
            const int c = contig_of_head[J.ptr[s] >> 1];
            if (c >= 0) {
                o.state = PBA_LAY_PLACED; o.contig = c; o.rank = J.hops[s]; o.orient = s & 1;
                o.offset = (int32_t)J.before[s]; o.skip = skip[s]; o.adv = adv[s];
                const uint32_t slot = contig_slot[c] + (uint32_t)o.rank;
                if (slot < n_slots) {                         // (always: a rank is below its chain's read count)
                    slot_read[slot] = (int)r;
                    slot_text[slot] = contig_text[c] + J.before[s];
                }
            }
        }
        table[r] = o;
    }
}

// 16 output bases per lane.  slot_text[0 .. n_slots] is non-decreasing and ends with `total`: the slot that supplies base g
// is the last one with slot_text <= g (slots that supply nothing share their offset with the slot after them).
static __global__ void __launch_bounds__(256)
k_lay_stitch(SeqSetDev S, const pba_layout_row *table, const int *slot_read, const unsigned long long *slot_text, uint32_t n_slots,
             unsigned long long total, char *text) {
    const unsigned long long groups = (total + 15) / 16;
    for (unsigned long long grp = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; grp < groups; grp += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long g0 = grp * 16;
        const int nb = (int)min(16ull, total - g0);
        uint32_t lo = 0, hi = n_slots;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (slot_text[mid] <= g0) lo = mid; else hi = mid;
        }
        uint32_t slot = lo;
        unsigned long long s_beg = slot_text[slot], s_end = slot_text[slot + 1];
        pba_layout_row row = table[slot_read[slot]];
        const uint8_t *seq = S.packed + S.off[row.read];
        int L = (int)S.len[row.read];
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        for (int k = 0; k < nb; ++k) {
            const unsigned long long g = g0 + (unsigned long long)k;
            while (g >= s_end && slot + 1 < n_slots) {        // (ends before the bound: slot_text[n_slots] = total > g)
                ++slot; s_beg = s_end; s_end = slot_text[slot + 1];
                row = table[slot_read[slot]];
                seq = S.packed + S.off[row.read];
                L = (int)S.len[row.read];
            }
            const int at = row.skip + (int)(g - s_beg);       // < skip + adv <= L
            const int i = row.orient ? L - 1 - at : at;
            int code = (seq[i >> 2] >> (6 - 2 * (i & 3))) & 3;
            if (row.orient) code ^= 3;
            w[k >> 2] |= (uint32_t)(uint8_t)"ACGT"[code] << (8 * (k & 3));
        }
        if (nb == 16) *reinterpret_cast<uint4 *>(text + g0) = make_uint4(w[0], w[1], w[2], w[3]);
        else for (int k = 0; k < nb; ++k) text[g0 + k] = (char)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// ---- placement: where a row's anchor -- the first pair of elements its alignment compared -- lies on the target's contig
enum { PC_NOT_PLACED = 0, PC_OUTSIDE, PC_ELIGIBLE, PC_FOUND_PLACED, PC_FOUND_CONTAINED, PC_FOUND_UNPLACED, PC_COUNT };
struct LayAnchor { int kind, contig, pos, dir, strand, j; };  // kind: PC_NOT_PLACED / PC_OUTSIDE / PC_ELIGIBLE (then the rest)

// The one geometry of both placement kernels.  The anchor base must be one the target SUPPLIES: only there is
// contig[offset + p] == walked(t)[skip + p] an identity; the bases before skip were supplied by the predecessor's text.
static __device__ __forceinline__ LayAnchor lay_anchor(const pba_strand_overlap &r, const uint32_t *len, const pba_layout_row *table) {
    const pba_layout_row T = table[r.target];
    LayAnchor a{PC_NOT_PLACED, -1, 0, 0, 0, 0};
    if (T.state != PBA_LAY_PLACED) return a;
    const int lt = (int)len[r.target], lq = (int)len[r.query];
    const int qb = r.strand == 1 ? r.q_beg : lq - r.q_end, qe = r.strand == 1 ? r.q_end : lq - r.q_beg;   // of the walked text
    const int xa = r.dir == 1 ? r.t_beg : r.t_end - 1, yb = r.dir == 1 ? qb : qe - 1;
    const int at = T.orient ? lt - 1 - xa : xa;               // the anchor in the text the contig holds of t
    a.kind = PC_OUTSIDE;
    if (at < T.skip || at >= T.skip + T.adv) return a;
    a.kind = PC_ELIGIBLE; a.contig = T.contig; a.pos = T.offset + at - T.skip;
    a.dir = T.orient ? -r.dir : r.dir; a.strand = T.orient ? -r.strand : r.strand;   // the contig holds rc(t): all turns round
    a.j = T.orient ? lq - 1 - yb : yb;
    return a;
}

static __global__ void __launch_bounds__(256)
k_lay_pick(const pba_strand_overlap *rows, uint64_t n_rows, const uint32_t *len, const pba_layout_row *table, unsigned long long *pick,
           unsigned long long *counters) {
    int c[3] = {0, 0, 0};
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_rows; k += (uint64_t)gridDim.x * blockDim.x) {
        const pba_strand_overlap r = rows[k];
        const LayAnchor a = lay_anchor(r, len, table);
        ++c[a.kind];
        if (a.kind == PC_ELIGIBLE) atomicMax(&pick[r.query], lay_key(r.q_end - r.q_beg, r.cost, k));
    }
    lay_count(counters, PC_NOT_PLACED, c[PC_NOT_PLACED]); lay_count(counters, PC_OUTSIDE, c[PC_OUTSIDE]);
    lay_count(counters, PC_ELIGIBLE, c[PC_ELIGIBLE]);
}

static __global__ void __launch_bounds__(256)
k_lay_emit(const pba_strand_overlap *rows, const uint32_t *len, const pba_layout_row *table, const unsigned long long *pick,
           pba_place_row *out, uint32_t n, unsigned long long *counters) {
    int c[3] = {0, 0, 0};                                     // found reads by layout state: UNPLACED, PLACED, CONTAINED
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
        pba_place_row o;
        o.read = (int32_t)r; o.found = 0; o.row = 0u; o.contig = -1; o.pos = o.dir = o.strand = o.j = 0;
        const unsigned long long key = pick[r];
        if (key != 0ull) {                                    // (a key holds a length >= 1: never 0)
            const uint32_t k = lay_key_row(key);
            const LayAnchor a = lay_anchor(rows[k], len, table);   // eligible: it was picked
            o.found = 1; o.row = k; o.contig = a.contig; o.pos = a.pos; o.dir = a.dir; o.strand = a.strand; o.j = a.j;
            ++c[table[r].state];
        }
        out[r] = o;
    }
    lay_count(counters, PC_FOUND_PLACED, c[PBA_LAY_PLACED]); lay_count(counters, PC_FOUND_CONTAINED, c[PBA_LAY_CONTAINED]);
    lay_count(counters, PC_FOUND_UNPLACED, c[PBA_LAY_UNPLACED]);
}

extern "C" {

struct pba_layout {
    int device;
    uint32_t n, n_slots;
    std::vector<uint32_t> h_len;
    std::vector<int32_t> c_head, c_reads, c_len;
    std::vector<uint64_t> c_text;                // text offset of every contig, and the total
    DevBuf keep;                                 // one allocation behind the three arrays stitch and pba_layout_rows read:
    pba_layout_row *table;                       //   a row per read
    int *slot_read;                              //   the read of every slot of the (contig, rank) order
    unsigned long long *slot_text;               //   the text offset of every slot, and the total
    mutable pba_layout_stats stats;
};

static const uint64_t kLayMaxContig = 0x7FFFFFF0ull;

static int lay_check(pba_ctx *ctx, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows, int hang, int min_reads) {
    if (hang < 0) PBA_FAIL(PBA_E_INVALID, "pba_layout_create: hang must be >= 0");
    if (min_reads < 1) PBA_FAIL(PBA_E_INVALID, "pba_layout_create: min_reads must be >= 1");
    return check_overlap_rows(ctx, "pba_layout_create", reads, rows, n_rows, false, true);
}

static inline dim3 lay_grid(uint64_t n) { return dim3(elem_grid(n, 256)); }

int pba_layout_create(pba_ctx *ctx, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows, int hang, int min_reads,
                      pba_layout **out, pba_layout_stats *stats) {
    if (!ctx || !reads || !out || (!rows && n_rows)) return PBA_E_INVALID;
    *out = nullptr;
    PBA_TRY(lay_check(ctx, reads, rows, n_rows, hang, min_reads));
    HIPCHK(hipSetDevice(ctx->device));
    StageClock clk;
    if (!clk.init()) PBA_FAIL(PBA_E_HIP, "pba_layout_create: hipEventCreate");
    std::unique_ptr<pba_layout, void (*)(pba_layout *)> lay(new (std::nothrow) pba_layout(), pba_layout_destroy);
    if (!lay) PBA_FAIL(PBA_E_NOMEM, "pba_layout");
    const uint32_t n = reads->n, ns = 2 * n;
    lay->device = ctx->device; lay->n = n; lay->n_slots = 0;
    lay->h_len.assign(reads->h_len.begin(), reads->h_len.begin() + n);
    lay->c_text.assign(1, 0);
    memset(&lay->stats, 0, sizeof lay->stats);
    lay->stats.n_rows = n_rows;
    hipStream_t st = ctx->stream;

    // Device work arrays: carved out of ONE pooled buffer of the ctx (and the rows out of another), as the other drivers keep
    // theirs -- a hipMalloc / hipFree pair per array would synchronise the device fifteen times inside the timed stages.  What
    // stitch and pba_layout_rows need is one allocation kept in *lay, sized by its upper bound (no more slots than reads).
    const size_t S = std::max<size_t>(ns, 1), N = std::max<size_t>(n, 1);
    size_t carve = 0;
    auto take = [&carve](size_t bytes) { const size_t at = carve; carve += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_cont = take(8 * N), o_best = take(8 * S), o_mate = take(4 * S), o_skip = take(4 * S), o_adv = take(4 * S),
                 o_jump0 = take(20 * S), o_jump1 = take(20 * S),            // before (u64), then ptr, hops, mn
                 o_canon = take(4 * S), o_creads = take(4 * S), o_cbases = take(8 * S), o_pstate = take(4 * N), o_hreads = take(4 * N),
                 o_hbases = take(8 * N), o_cnt = take(8 * LC_COUNT), o_coh = take(4 * N), o_cslot = take(4 * N), o_ctext = take(8 * (N + 1));
    uint8_t *work = nullptr, *d_rows = nullptr;
    POOL(POOL_LAY_WORK, carve, work);
    POOL(POOL_LAY_ROWS, std::max<size_t>(1, sizeof(pba_strand_overlap) * n_rows), d_rows);
    carve = 0;
    const size_t k_table = take(sizeof(pba_layout_row) * N), k_sread = take(4 * N), k_stext = take(8 * (N + 1));
    HIPCHK(hipMalloc(&lay->keep.p, carve));
    lay->table = (pba_layout_row *)(lay->keep.as<uint8_t>() + k_table);
    lay->slot_read = (int *)(lay->keep.as<uint8_t>() + k_sread);
    lay->slot_text = (unsigned long long *)(lay->keep.as<uint8_t>() + k_stext);
    LayJump J[2];
    for (int k = 0; k < 2; ++k) {
        J[k].before = (unsigned long long *)(work + (k ? o_jump1 : o_jump0));
        J[k].ptr = (int *)(J[k].before + S); J[k].hops = J[k].ptr + S; J[k].mn = J[k].hops + S;
    }
    const pba_strand_overlap *R = (const pba_strand_overlap *)d_rows;
    unsigned long long *cont = (unsigned long long *)(work + o_cont), *best = (unsigned long long *)(work + o_best),
                       *cnt = (unsigned long long *)(work + o_cnt), *cbases = (unsigned long long *)(work + o_cbases),
                       *hbases = (unsigned long long *)(work + o_hbases), *d_ctext = (unsigned long long *)(work + o_ctext);
    int *mate = (int *)(work + o_mate), *skip = (int *)(work + o_skip), *adv = (int *)(work + o_adv), *canon = (int *)(work + o_canon),
        *creads = (int *)(work + o_creads), *pstate = (int *)(work + o_pstate), *hreads = (int *)(work + o_hreads), *d_coh = (int *)(work + o_coh);
    uint32_t *d_cslot = (uint32_t *)(work + o_cslot);
    unsigned long long h_cnt[LC_COUNT];
    memset(h_cnt, 0, sizeof h_cnt);

    {   // rows up once; classification, best edges, mates
        const auto timed = clk.time(st, &lay->stats.classify_ms);
        if (n_rows) HIPCHK(hipMemcpyAsync(d_rows, rows, sizeof(pba_strand_overlap) * n_rows, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(cont, 0xFF, 8 * N, st));
        HIPCHK(hipMemsetAsync(best, 0, 8 * S, st));
        HIPCHK(hipMemsetAsync(cnt, 0, 8 * LC_COUNT, st));
        if (n_rows) {
            hipLaunchKernelGGL(k_lay_classify, lay_grid(n_rows), dim3(256), 0, st, R, n_rows, reads->d_len, hang, cont, cnt);
            hipLaunchKernelGGL(k_lay_best, lay_grid(n_rows), dim3(256), 0, st, R, n_rows, reads->d_len, hang, cont, best, cnt);
        }
        if (ns) hipLaunchKernelGGL(k_lay_mate, lay_grid(ns), dim3(256), 0, st, R, reads->d_len, hang, best, mate, ns, cnt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    int rounds = 0;
    while ((1ull << rounds) < ns) ++rounds;                   // ceil(log2(2n)): a path holds at most n states
    std::vector<int32_t> h_hreads(n);
    std::vector<uint64_t> h_hbases(n);
    int cur = 0;
    {   // chains
        const auto timed = clk.time(st, &lay->stats.chain_ms);
        for (int pass = 0; pass < 2 && ns; ++pass) {
            cur = 0;
            hipLaunchKernelGGL(k_lay_succ, lay_grid(ns), dim3(256), 0, st, R, reads->d_len, best, mate, skip, adv, J[0], canon, ns);
            for (int k = 0; k < rounds; ++k, cur ^= 1)
                hipLaunchKernelGGL(k_lay_jump, lay_grid(ns), dim3(256), 0, st, J[cur], J[cur ^ 1], ns);
            if (pass) break;
            hipLaunchKernelGGL(k_lay_cut, lay_grid(ns), dim3(256), 0, st, J[cur], mate, ns, cnt);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if (!h_cnt[LC_CYCLES]) break;                     // no cycle was cut: the ranks stand
        }
        if (ns) {
            hipLaunchKernelGGL(k_lay_chain, lay_grid(ns), dim3(256), 0, st, J[cur], adv, mate, canon, creads, cbases, ns);
            hipLaunchKernelGGL(k_lay_place, lay_grid(n), dim3(256), 0, st, J[cur], cont, canon, creads, cbases, min_reads, pstate, hreads,
                               hbases, n, cnt);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h_hreads.data(), hreads, 4 * (size_t)n, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(h_hbases.data(), hbases, 8 * (size_t)n, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        // the scan over the head flags: contig ids by ascending head read, first slot and first text byte of every contig
        std::vector<int32_t> contig_of_head(N, -1);
        std::vector<uint32_t> c_slot;
        for (uint32_t r = 0; r < n; ++r) {
            if (h_hreads[r] <= 0) continue;
            if (h_hbases[r] >= kLayMaxContig) PBA_FAIL(PBA_E_TOOLONG, "pba_layout_create: a contig of 0x7FFFFFF0 bases or more");
            contig_of_head[r] = (int32_t)lay->c_head.size();
            c_slot.push_back(lay->n_slots);
            lay->c_head.push_back((int32_t)r); lay->c_reads.push_back(h_hreads[r]); lay->c_len.push_back((int32_t)h_hbases[r]);
            lay->n_slots += (uint32_t)h_hreads[r];
            lay->c_text.push_back(lay->c_text.back() + h_hbases[r]);
        }
        const size_t nc = lay->c_head.size();
        HIPCHK(hipMemsetAsync(lay->slot_read, 0, 4 * N, st));
        HIPCHK(hipMemsetAsync(lay->slot_text, 0, 8 * (N + 1), st));
        HIPCHK(hipMemcpyAsync(d_coh, contig_of_head.data(), 4 * N, hipMemcpyHostToDevice, st));
        if (nc) HIPCHK(hipMemcpyAsync(d_cslot, c_slot.data(), 4 * nc, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_ctext, lay->c_text.data(), 8 * (nc + 1), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(lay->slot_text + lay->n_slots, &lay->c_text.back(), 8, hipMemcpyHostToDevice, st));
        if (n) hipLaunchKernelGGL(k_lay_table, lay_grid(n), dim3(256), 0, st, J[cur], cont, pstate, skip, adv, d_coh, d_cslot, d_ctext,
                                  lay->table, lay->slot_read, lay->slot_text, lay->n_slots, n);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));                     // (the host vectors must outlive their copies)
    }
    pba_layout_stats &s = lay->stats;
    s.n_internal = h_cnt[LC_INTERNAL]; s.n_contain = h_cnt[LC_CONTAIN]; s.n_contain_refused = h_cnt[LC_REFUSED];
    s.n_dovetail = h_cnt[LC_DOVETAIL]; s.n_dovetail_dropped = h_cnt[LC_DROPPED];
    s.n_contained = (uint32_t)h_cnt[LC_CONTAINED]; s.n_mated_ends = (uint32_t)h_cnt[LC_MATED]; s.n_cycles = (uint32_t)h_cnt[LC_CYCLES];
    s.n_contigs = (uint32_t)lay->c_head.size(); s.n_placed = lay->n_slots; s.n_unplaced = n - s.n_placed - s.n_contained;
    s.n_bases = lay->c_text.back();
    if (stats) *stats = s;
    *out = lay.release();
    return PBA_OK;
}

int pba_layout_rows(pba_ctx *ctx, const pba_layout *lay, pba_layout_row *out, uint32_t cap) {
    if (!ctx || !lay) return PBA_E_INVALID;
    if (cap < lay->n || (!out && lay->n)) PBA_FAIL(PBA_E_INVALID, "pba_layout_rows: room for fewer rows than the layout has reads");
    HIPCHK(hipSetDevice(ctx->device));
    if (lay->n) HIPCHK(hipMemcpyAsync(out, lay->table, sizeof(pba_layout_row) * (size_t)lay->n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PBA_OK;
}

uint32_t pba_layout_contigs(const pba_layout *lay) { return lay ? (uint32_t)lay->c_head.size() : 0; }

int pba_layout_contig_info(const pba_layout *lay, int32_t *head_read, int32_t *n_reads, int32_t *length, uint32_t cap) {
    if (!lay || cap < lay->c_head.size()) return PBA_E_INVALID;
    for (size_t c = 0; c < lay->c_head.size(); ++c) {
        if (head_read) head_read[c] = lay->c_head[c];
        if (n_reads) n_reads[c] = lay->c_reads[c];
        if (length) length[c] = lay->c_len[c];
    }
    return PBA_OK;
}

int pba_layout_stitch(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, pba_seqs **contigs) {
    if (!ctx || !lay || !reads || !contigs) return PBA_E_INVALID;
    *contigs = nullptr;
    if (reads->n != lay->n || !std::equal(lay->h_len.begin(), lay->h_len.end(), reads->h_len.begin()))
        PBA_FAIL(PBA_E_INVALID, "pba_layout_stitch: the set differs from the layout's in count or lengths");
    if (reads->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_layout_stitch: the read set holds bytes outside ACGT (code 3 has no complement)");
    HIPCHK(hipSetDevice(ctx->device));
    StageClock clk;
    if (!clk.init()) PBA_FAIL(PBA_E_HIP, "pba_layout_stitch: hipEventCreate");
    const uint64_t total = lay->c_text.back();
    const uint32_t nc = (uint32_t)lay->c_head.size();
    DevBuf text, d_off;
    lay->stats.stitch_ms = 0.f;
    const auto timed = clk.time(ctx->stream, &lay->stats.stitch_ms);
    HIPCHK(hipMalloc(&text.p, total + kSlack));
    HIPCHK(hipMalloc(&d_off.p, 8 * ((size_t)nc + 1)));
    HIPCHK(hipMemcpyAsync(d_off.p, lay->c_text.data(), 8 * ((size_t)nc + 1), hipMemcpyHostToDevice, ctx->stream));
    if (total) {
        hipLaunchKernelGGL(k_lay_stitch, lay_grid((total + 15) / 16), dim3(256), 0, ctx->stream, reads->dev(), lay->table,
                           lay->slot_read, lay->slot_text, lay->n_slots, (unsigned long long)total,
                           text.as<char>());
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return pba_seqs_from_device_text(ctx, text.p, d_off.p, nc, total, 0, contigs);
}

int pba_layout_place(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows,
                     pba_place_row *out, uint32_t cap, pba_place_stats *stats) {
    if (!ctx || !lay || !reads || (!rows && n_rows)) return PBA_E_INVALID;
    if (reads->n != lay->n || !std::equal(lay->h_len.begin(), lay->h_len.end(), reads->h_len.begin()))
        PBA_FAIL(PBA_E_INVALID, "pba_layout_place: the set differs from the layout's in count or lengths");
    if (cap < lay->n || (!out && lay->n)) PBA_FAIL(PBA_E_INVALID, "pba_layout_place: room for fewer rows than the layout has reads");
    PBA_TRY(check_overlap_rows(ctx, "pba_layout_place", reads, rows, n_rows, true, true));
    HIPCHK(hipSetDevice(ctx->device));
    StageClock clk;
    if (!clk.init()) PBA_FAIL(PBA_E_HIP, "pba_layout_place: hipEventCreate");
    const uint32_t n = lay->n;
    const size_t N = std::max<size_t>(n, 1);
    size_t carve = 0;
    auto take = [&carve](size_t bytes) { const size_t at = carve; carve += (bytes + 255) & ~(size_t)255; return at; };
    const size_t o_pick = take(8 * N), o_cnt = take(8 * PC_COUNT), o_out = take(sizeof(pba_place_row) * N);
    uint8_t *work = nullptr, *d_rows = nullptr;
    POOL(POOL_LAY_WORK, carve, work);
    POOL(POOL_LAY_ROWS, std::max<size_t>(1, sizeof(pba_strand_overlap) * n_rows), d_rows);
    const pba_strand_overlap *R = (const pba_strand_overlap *)d_rows;
    unsigned long long *pick = (unsigned long long *)(work + o_pick), *cnt = (unsigned long long *)(work + o_cnt);
    pba_place_row *d_out = (pba_place_row *)(work + o_out);
    unsigned long long h_cnt[PC_COUNT];
    memset(h_cnt, 0, sizeof h_cnt);
    pba_place_stats s;
    memset(&s, 0, sizeof s);
    s.n_rows = n_rows;
    hipStream_t st = ctx->stream;
    {   // rows up once; the pick and the emit
        const auto timed = clk.time(st, &s.place_ms);
        if (n_rows) HIPCHK(hipMemcpyAsync(d_rows, rows, sizeof(pba_strand_overlap) * n_rows, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(pick, 0, 8 * N, st));
        HIPCHK(hipMemsetAsync(cnt, 0, 8 * PC_COUNT, st));
        if (n_rows) hipLaunchKernelGGL(k_lay_pick, lay_grid(n_rows), dim3(256), 0, st, R, n_rows, reads->d_len, lay->table, pick, cnt);
        if (n) {
            hipLaunchKernelGGL(k_lay_emit, lay_grid(n), dim3(256), 0, st, R, reads->d_len, lay->table, pick, d_out, n, cnt);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(out, d_out, sizeof(pba_place_row) * (size_t)n, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(h_cnt, cnt, sizeof h_cnt, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    s.n_target_not_placed = h_cnt[PC_NOT_PLACED]; s.n_outside = h_cnt[PC_OUTSIDE]; s.n_eligible = h_cnt[PC_ELIGIBLE];
    s.n_found_placed = (uint32_t)h_cnt[PC_FOUND_PLACED]; s.n_found_contained = (uint32_t)h_cnt[PC_FOUND_CONTAINED];
    s.n_found_unplaced = (uint32_t)h_cnt[PC_FOUND_UNPLACED];
    s.n_found = s.n_found_placed + s.n_found_contained + s.n_found_unplaced;
    if (stats) *stats = s;
    return PBA_OK;
}

int pba_layout_last_stats(const pba_layout *lay, pba_layout_stats *out) {
    if (!lay || !out) return PBA_E_INVALID;
    *out = lay->stats;
    return PBA_OK;
}

void pba_layout_destroy(pba_layout *lay) {
    if (!lay) return;
    (void)hipSetDevice(lay->device);
    delete lay;
}

}  // extern "C"
