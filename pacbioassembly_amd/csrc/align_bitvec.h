// align_bitvec.h -- bit-parallel kernel body for 2-bit packed sequences: one candidate pair per
// wavefront, the DP band swept as a 64-lane systolic array.
//
// What is computed.  seq_aligner<>::align (/root/reference/src/seq_aligner.h:92-213, canonical
// reading SURVEY.md A.4) exposes only: whether some diagonal cell fails cost(i,i) > i*R for
// i > 10 (:185), and the first strict minimum of the last row (or column) past the diagonal
// (:191-213).  Both are functions of the plain unit-cost edit-distance matrix U with
// U(i,0)=i, U(0,j)=j, because (DESIGN.md "exactness of the bit-vector kernel"):
//   * banded D >= U, and a path that leaves the band |i-j| <= max_dst and comes back to
//     diagonal offset d costs at least 2*(max_dst+1) - |d|;
//   * a passing diagonal cell has cost <= floor(i*R) <= max_dst-1, so banded and unbanded
//     values agree wherever the comparison could go either way, and every goal cell (last row or
//     column past the diagonal) that could be a strict minimum costs less than D(m,m) <= max_dst-1.
// U is evaluated in Myers/Hyyro vertical-delta encoding: a 32-row block holds +1/-1 bit masks
// (Pv, Mv); one text column updates the block with ~20 integer ops, i.e. 32 DP cells per
// ~20 lane-ops instead of ~8 ops per cell.
//
// Mapping to the wavefront.  Rows are the LONGER sequence (as far down as the window reaches: m + w
// of them), columns the shorter one (m): the free end of the alignment then runs down the last
// column, whose cells are produced by the last ~w/RB superblocks while the lanes above still work --
// with the shorter sequence as rows the same cells cost w extra steps at the end with most of the
// array idle.  Rows are cut into superblocks of NB*32 rows; superblock s lives in lane s mod 64 and
// processes column j at step t = j + s, so a column flows down the lanes one lane per step.  The
// horizontal deltas leaving the bottom row of a superblock are carry-outs of v_addc_co_u32, i.e. lane
// masks in SGPR pairs, and reach the next lane through a scalar 64-bit rotate of those masks (no DPP,
// no VALU).  (The score-only sweeps at one and two blocks per lane keep the lanes in the order of their superblocks
// instead -- lane k holds the k-th superblock not yet closed, lane_shift.h -- and the rotate is a shift.)  Only the columns of a superblock's window are processed (lo..hi); cells left of the
// window are taken as "+1 per row" and the row above the window as "+1 per column", which are real
// (if expensive) paths, so everything computed is an upper bound W >= U that equals U whenever U's
// optimal path stays inside the windows.
// The window is asymmetric: row i sees the columns [i - w, i + wl]: w on the side of the free end
// (below the diagonal, where the goal cells (i, m), i >= m, lie), wl on the other.  A path that leaves
// on the wl side must come back across the diagonal: it costs >= 2*wl+2; one that leaves on the w
// side costs >= w+1.  Hence:
//   * a PASSING diagonal verdict is always exact (W >= U);  a FAILING one at row i is exact when
//     floor(i*R) < 2*wl+2 (no unseen path back to the diagonal is cheap enough to change it);
//   * the goal column is exact when its minimum is <= min(w, 2*wl+1).
// Anything else answers "uncertified" and the pair is re-run with w = max_dst, the reference's own
// band, and wl = max_dst/2 + 1: every row's threshold floor(i*R) <= max_dst - 1 < 2*wl + 2 and every
// goal minimum of a pair that passed its checks is <= max_dst - 1, so that sweep certifies
// everything.  Results are bit-identical to the reference in all cases.  First pass: w = 9/16
// max_dst, wl = w/2: 25 % fewer cells than a symmetric window and, more to the point, narrow enough
// for one block less per lane at BASELINE sizes.
#ifndef PBA_ALIGN_BITVEC_H
#define PBA_ALIGN_BITVEC_H

#include <limits.h>

#include <type_traits>

#include "align_rowsweep.h"
#include "dev_common.h"
#include "eq_table.h"
#include "lane_shift.h"
#include "text_ring.h"

// The score-only sweeps of the aligning kernels at one and two blocks per lane read their match masks from a per-lane table
// in LDS (eq_table.h) instead of computing them every step.  -DPBA_BV_EQTAB=0 builds those forms with the register planes
// and the mask-pair ring of every other ring form (tools/build_variant.py).
#ifndef PBA_BV_EQTAB
#define PBA_BV_EQTAB 1
#endif
#ifndef PBA_BV_RING                                    // (align_bitvec below: 0 builds every form with the register planes)
#define PBA_BV_RING 1
#endif
#define PBA_BV_EQTAB_NB(nb) (PBA_BV_EQTAB && PBA_BV_RING && (nb) <= 2)
// The table forms keep the lanes in the order of their superblocks, lane 0 the top of the band (lane_shift.h): the hand-off
// is two scalar shifts and an or.  -DPBA_BV_SHIFT=0 builds them with the ring of lanes and the `live` mask of every other form.
#ifndef PBA_BV_SHIFT
#define PBA_BV_SHIFT 1
#endif
// The one step behind a close of those forms runs inside the close's own iteration of the handler, in front of the stretch
// that follows it.  -DPBA_BV_CLOSE_INLINE=0: it ends that iteration and runs alone in one of its own.
#ifndef PBA_BV_CLOSE_INLINE
#define PBA_BV_CLOSE_INLINE 1
#endif

#define PBA_BV_MAX_NB 8
#define PBA_BV_FIN_WORDS(nb) ((2 * (nb) + 1) * 64)     // u32 of LDS per wavefront for the last column's deltas (bitvec_pass: fin)
// per wavefront of a score-only launch: the fin words, then the text ring (text_ring.h); in the table forms the table with the
// fin Pv / Mv words on it, the ring of 4-byte cells and the fin superblock word (eq_table.h)
#define PBA_BV_LDS_BYTES(nb) (PBA_BV_EQTAB_NB(nb) ? eqt_lds_words(nb) * 4 : PBA_BV_FIN_WORDS(nb) * 4 + PBA_TXR_BYTES)
#define PBA_BV_BAND_NUM 9      // first-pass half width = max(max_dst/2, 9/16 * max_dst) + 1
#define PBA_BV_BAND_DEN 16

// widest window (wl + w) a superblock of NB blocks supports: lane s must be done with superblock s
// before superblock s+64 starts (wl + w <= 63*32*NB + 64)
__device__ __host__ inline int bv_max_span(int nb) { return 2016 * nb + 64; }
__device__ __host__ inline int bv_nb_for_span(int span) {
    const int need = (span - 64 + 2015) / 2016;
    const int nb = need < 1 ? 1 : need;
    return nb <= 4 ? nb : (nb <= 6 ? 6 : (nb <= 8 ? 8 : 0));   // instantiated: 1,2,3,4,6,8; 0 = too wide
}
__device__ __host__ inline int bv_nb_for(int w) { return bv_nb_for_span(2 * w); }   // symmetric window

// 64 bits of an accessor's 2-bit stream starting at base index `idx` (may be unaligned / slightly out of
// range: sequence sets carry 1 KB of readable slack on both sides): bit 63:62 = base idx, ..., bit 1:0 = base idx+31
__device__ __forceinline__ uint64_t load_bases32(const uint8_t *seq, int idx) {
    const uint8_t *p = seq + (idx >> 2);
    const uint64_t hi = __builtin_bswap64(ld_u64(p)), nx = __builtin_bswap64(ld_u64(p + 8));
    const int sh = 2 * (idx & 3);
    return sh ? (hi << sh) | (nx >> (64 - sh)) : hi;
}

// bit q of the result = bit 2q of x (q = 0..31)
__device__ __forceinline__ uint32_t compress_even64(uint64_t x) {
    uint32_t lo = (uint32_t)x & 0x55555555u, hi = (uint32_t)(x >> 32) & 0x55555555u;
    lo = (lo | (lo >> 1)) & 0x33333333u; hi = (hi | (hi >> 1)) & 0x33333333u;
    lo = (lo | (lo >> 2)) & 0x0F0F0F0Fu; hi = (hi | (hi >> 2)) & 0x0F0F0F0Fu;
    lo = (lo | (lo >> 4)) & 0x00FF00FFu; hi = (hi | (hi >> 4)) & 0x00FF00FFu;
    lo = (lo | (lo >> 8)) & 0x0000FFFFu; hi = (hi | (hi >> 8)) & 0x0000FFFFu;
    return lo | (hi << 16);
}

// bit planes of 32 consecutive accessor elements starting at element e: bit r of plo/phi = low/high bit of
// element e+r.  From the set's precomputed planes, stored word by word side by side (low word w, high word w, low word
// w+1, ...): four consecutive dwords -- one 16-byte fetch, one cache line for both planes -- and one funnel shift per
// plane (the index may run a few hundred bases before / past the sequence: neighbours or zero slack, never used).
__device__ __forceinline__ void load_planes32(const PackedFetch &f, int e, uint32_t &plo, uint32_t &phi) {
    const int idx = f.dir > 0 ? f.org + e : f.org - e - 31;          // lowest base index of the 32, in memory order
    const uint32_t *p = f.pl + 2 * (ptrdiff_t)(idx >> 5);             // (arithmetic shift: negative indices reach the slack)
    const uint32_t sh = (uint32_t)idx & 31u;
    const uint32_t lo = __builtin_amdgcn_alignbit(p[2], p[0], sh);    // ({low[w+1], low[w]} >> sh)[31:0]
    const uint32_t hi = __builtin_amdgcn_alignbit(p[3], p[1], sh);
    plo = f.dir > 0 ? lo : __builtin_bitreverse32(lo);                // backward: element r is base idx + 31 - r
    phi = f.dir > 0 ? hi : __builtin_bitreverse32(hi);
}

// the planes of 32 bases from the packed bytes (k_make_planes builds a set's planes with this, once)
__device__ __forceinline__ void planes_from_packed(const uint8_t *seq, int idx, uint32_t &plo, uint32_t &phi) {
    const uint64_t x = load_bases32(seq, idx);                        // base idx + r at bits 63-2r : 62-2r
    plo = __builtin_bitreverse32(compress_even64(x));
    phi = __builtin_bitreverse32(compress_even64(x >> 1));
}

// d = a + b + carry-in, carry-out to a lane mask: v_addc_co_u32 with SGPR-pair carries.  One instruction does
// "shift left by one, OR in the delta entering at the top row, hand out the delta leaving at the bottom row".
__device__ __forceinline__ uint32_t addc_mask(uint32_t a, uint32_t b, uint64_t cin, uint64_t &cout) {
    uint32_t d;
    asm("v_addc_co_u32 %0, %1, %2, %3, %4" : "=v"(d), "=s"(cout) : "v"(a), "v"(b), "s"(cin));
    return d;
}

// a | (b & c) in one full-rate v_bitop3_b32 (the compiler would pick the half-rate v_and_or_b32)
__device__ __forceinline__ uint32_t or_of_and(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t d;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xf8" : "=v"(d) : "v"(a), "v"(b), "v"(c));   // 0xF0 | (0xCC & 0xAA)
    return d;
}
// the same with c wave-uniform, from a scalar register (a VOP3 instruction takes one)
__device__ __forceinline__ uint32_t or_of_and_s(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t d;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xf8" : "=v"(d) : "v"(a), "v"(b), "s"(c));
    return d;
}
// ~a & ~(b ^ c): the match mask of a block from one xor and one bitop3 (left to itself the compiler rebuilds
// Eq & Pv from the two xors separately, one instruction more per block)
__device__ __forceinline__ uint32_t eq_mask(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t d;
    asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x09" : "=v"(d) : "v"(a), "v"(b), "v"(c));   // ~0xF0 & ~(0xCC ^ 0xAA)
    return d;
}
// a wave-uniform 64-bit value the compiler does not know to be one, back in a scalar register pair
__device__ __forceinline__ uint64_t bv_uniform64(uint64_t x) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x) |
           (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32;
}
// a | ~b and a & b of two lane masks, on the scalar unit whatever the compiler thinks of their uniformity: as plain C++ the
// masked carries of the streamed trace form's step loop (a divergent store inside it) are kept in vector register pairs,
// rotated there, and handed to v_addc_co_u32 as its carry-in, which takes none.  Every place that forms hpm / hnm uses these.
__device__ __forceinline__ uint64_t bv_orn2(uint64_t a, uint64_t b) {
    uint64_t d;
    asm("s_orn2_b64 %0, %1, %2" : "=s"(d) : "s"(a), "s"(b) : "scc");
    return d;
}
__device__ __forceinline__ uint64_t bv_and2(uint64_t a, uint64_t b) {
    uint64_t d;
    asm("s_and_b64 %0, %1, %2" : "=s"(d) : "s"(a), "s"(b) : "scc");
    return d;
}
// the shifted form's hand-off (lane_shift.h: lsh_hin_plus, lsh_hin_minus), on the scalar unit for the same reason
__device__ __forceinline__ uint64_t bv_shl1(uint64_t a) {
    uint64_t d;
    asm("s_lshl_b64 %0, %1, 1" : "=s"(d) : "s"(a) : "scc");
    return d;
}
__device__ __forceinline__ uint64_t bv_shl1_or1(uint64_t a) {
    uint64_t d;
    asm("s_lshl_b64 %0, %1, 1\n\ts_or_b64 %0, %0, 1" : "=&s"(d) : "s"(a) : "scc");
    return d;
}
// lane k's copy of lane k + 1's x (lane_shift.h: lsh_src_lane); the last lane keeps its own.  A whole-wave DPP shift: one
// instruction, no address register and no LDS trip (ds_bpermute_b32 does the same through the LDS crossbar, and its
// address cost k_locate<2> and k_spaced_round<1> a spilled word each)
__device__ __forceinline__ uint32_t bv_lane_below(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}
// sign-extended bit k of x (k wave-uniform): 0 or ~0
__device__ __forceinline__ uint32_t bit_mask(uint32_t x, int k) {
    uint32_t d;
    asm("v_bfe_i32 %0, %1, %2, 1" : "=v"(d) : "v"(x), "s"(k));
    return d;
}

// One sweep over the window [i - wleft, i + w].  Returns 0 when all diagonal checks pass (then best / besti hold the
// minimum of the last column at or below the diagonal and its row), else the first failing row.
//
// Instruction budget (measured on MI355X, tools/ubench_ops: and/or/xor/add/sub/not/bitop3/ashr issue every
// ~2.5 cycles per SIMD, shifts, bfe, alignbit, lshl_or, add3, addc and DPP moves every ~4.3): a Myers block is
// 9 full-rate ops + 3 v_addc_co (the carries are the horizontal deltas entering / leaving the block, kept as lane
// masks in SGPR pairs), and the lane-to-lane hand-off of those deltas is a SCALAR rotate of the two masks -- no
// DPP, no VALU.  The diagonal's D0 bits are collected with one bitop3 (in the diagonal's block only, at one or two
// blocks per lane) under a wave-uniform one-hot that a scalar shift advances; text
// elements come from two 32-step bit-plane registers, or (RING: the score-only forms of the aligning kernels) as ready mask
// pairs from the wavefront's text ring in LDS (text_ring.h), two steps' with one read; in rings 1 and 2 of those forms the
// match masks themselves come from the lane's table in LDS (eq_table.h: the ring's cell is the letter's row offset, one address
// add and one ds_read2st64_b32 per step replace the xor and the bitop3 of every block).  Everything rare is scheduled: the events of the sweep fall at
// steps known in advance, kept as wave-uniform timers, and the step loop runs from one to the next without a test.
//
// TRACE: also store, for every step and block, the two words the traceback needs (bv_trace_walk below):
//   word 0 = Eq | ~D0   bit r set: the cell's parent is the diagonal one (seq_aligner.h:164-166: MATCH wins ties)
//   word 1 = Ph (horizontal +1 entering the cell from the left), or the new Pv (vertical +1) when the rows are
//            the reference's b (`swap_roles`): set = the reference's INSERT, clear = its DELETE, for cells whose
//            parent is not diagonal (INSERT is tried first and wins the tie, seq_aligner.h:167-173)
// at tr[((t-1) * NB + nb) * 128 + 2 * lane + word]: one 8-byte store per lane, 512 contiguous bytes per instruction.
// TRACE == 2: instead, checkpoints -- at the start of every 32-step chunk the lane's Pv / Mv words, its superblock and window
// state and the two hand-off masks go to tr (bv_ck_words per chunk, 1/25 of the streamed words); the walk re-runs one
// chunk at a time from its checkpoint into LDS (align_bvtrace.h: bitvec_rerun).
#define PBA_BV_CK_WORDS(nb) ((nb) * 128 + 128)
#define PBA_BV_BAIL 0x40000000                         // bitvec_pass: "not worth finishing in this window" (above any row number)
template <int NB>
__device__ __forceinline__ void bv_ckpt_store(uint32_t *tr, int tb, int lane, const uint32_t *Pv, const uint32_t *Mv, int s_cur,
                                              uint32_t opened, uint64_t hp_last, uint64_t hn_last) {
    uint32_t *ck = tr + (size_t)((tb - 1) >> 5) * PBA_BV_CK_WORDS(NB);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { ck[nb * 128 + lane] = Pv[nb]; ck[nb * 128 + 64 + lane] = Mv[nb]; }
    ck[NB * 128 + lane] = (uint32_t)s_cur | (opened << 31);
    if (lane < 4)
        ck[NB * 128 + 64 + lane] = lane == 0 ? (uint32_t)hp_last : lane == 1 ? (uint32_t)(hp_last >> 32) : lane == 2 ? (uint32_t)hn_last : (uint32_t)(hn_last >> 32);
}

template <int NB, int TRACE = 0, bool BAIL = false, bool RING = false>
__device__ __forceinline__ int bitvec_pass(const PackedFetch &rowsF, int nr, const PackedFetch &colsF, int m, int wleft, int w,
                                           double R, int &best_out, int &besti_out, int &diag_out, uint32_t *fin,
                                           uint32_t *tr = nullptr, bool swap_roles = false, int bail_w = 0) {
    // BAIL and bail_w > 0: give the sweep up (return PBA_BV_BAIL) once the diagonal says where the pair is heading -- at row i >= 1024,
    // (D(i,i) - 4 sqrt(D(i,i))) * m / i > bail_w (four standard deviations of a count of D(i,i) errors below the projection:
    // a pair that will come in under bail_w is not given up by accident; the check runs at every 32nd row): a cost the
    // window could not certify anyway (align_bitvec: the caller re-runs the pair with the
    // reference's band either way; this only decides how many rows the narrow sweep spends finding out).  Never changes a result.
    // rowsF / nr: the longer sequence and how many of its rows are swept (m <= nr <= m + wleft); colsF / m: the shorter
    // one.  Row i sees the columns [i - wleft, i + w] (wleft: the wide side, towards the free end; w: the narrow one).
    constexpr int RB = 32 * NB;                 // rows per superblock
    const int lane = threadIdx.x & (PBA_WAVE - 1);
    m = __builtin_amdgcn_readfirstlane(m); nr = __builtin_amdgcn_readfirstlane(nr);   // wave-uniform by construction
    w = __builtin_amdgcn_readfirstlane(w); wleft = __builtin_amdgcn_readfirstlane(wleft);
    const int S = (nr + RB - 1) / RB;           // superblocks
    const int s_m = (m - 1) / RB;               // superblock, block and bit of row m (the end of the diagonal)
    const int nb_m = ((m - 1) - s_m * RB) >> 5, r_m = (m - 1) & 31;
    const int t1 = m + s_m;                     // step at which cell (m,m) is produced
    const int t_end = m + S - 1;                // step at which the last superblock takes the last column
    (void)nb_m; (void)r_m;

    // EQT: the match masks come from the lane's table in LDS (eq_table.h) -- `fin` is then the wavefront's whole region: the
    // table (with the fin Pv / Mv words on the lane's own rows), the ring, the fin superblock word.  The row planes are
    // live only while a lane fills its rows, not in the step loop.
    constexpr bool EQT = RING && PBA_BV_EQTAB_NB(NB);
    constexpr int FIN_SB = EQT ? PBA_EQT_LETTERS * NB * PBA_EQT_LANES + PBA_TXR_SLOTS : 2 * NB * PBA_WAVE;   // eqt_sb_word(NB); else behind the fin words
    typedef __attribute__((address_space(3))) uint32_t lds_u32;
    // SHIFT: lane k holds superblock s_cl + k and works in column (lane + s_cl) & 63 of the table (lane_shift.h); the close
    // event moves the lanes' state one lane up.  Else superblock s stays in lane s & 63, which is its column.
    constexpr bool SHIFT = EQT && PBA_BV_SHIFT;
    // The lane's column of the table is formed from `lane` and the schedule's scalar where it is used (a stretch forms it once,
    // in front of its loop): kept in a register of its own and moved on by the close it cost k_locate a spilled word more.
#define tab_lane ((lds_u32 *)fin + (SHIFT ? lsh_col(lane, s_cl) : lane))
    // a lane's four match masks per block, from the row planes of superblock sb: row (l, nb) = ~(Plo ^ mask(l0)) & ~(Phi ^ mask(l1))
#define PBA_BV_FILL_ROWS(sb)                                                          \
    _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) {                               \
        uint32_t plo_, phi_;                                                          \
        load_planes32(rowsF, (sb) * RB + 32 * nb, plo_, phi_);                        \
        tab_lane[(0 * NB + nb) * PBA_EQT_LANES] = ~(plo_ | phi_);                     \
        tab_lane[(1 * NB + nb) * PBA_EQT_LANES] = plo_ & ~phi_;                       \
        tab_lane[(2 * NB + nb) * PBA_EQT_LANES] = ~plo_ & phi_;                       \
        tab_lane[(3 * NB + nb) * PBA_EQT_LANES] = plo_ & phi_;                        \
    }

    uint32_t Pv[NB], Mv[NB], Plo[NB], Phi[NB], acc[NB];
    int s_cur = lane;      // (the forms without the text ring: LANE_SB below)
    uint32_t opened = 0;   // 0 / 1 in a VGPR (a bool would live in an SGPR pair and be re-merged with exec every step)
    (void)opened; (void)Plo; (void)Phi;
    if (s_cur < S) {
        constexpr int s_cl = 0;   // (tab_lane: the sweep starts with superblock s in lane s, column s)
        (void)s_cl;
        if constexpr (EQT) { PBA_BV_FILL_ROWS(s_cur) } else {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) load_planes32(rowsF, s_cur * RB + 32 * nb, Plo[nb], Phi[nb]);
        }
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) { Pv[nb] = ~0u; Mv[nb] = 0u; acc[nb] = 0u; }

    // The event schedule.  Nothing in it depends on the data: superblock s lives in lane s & 63 (SHIFT: in lane s - s_cl, and
    // the close moves every lane's state one lane up -- the schedule is the same, PBA_BV_LANE_OF), and each kind of event
    // falls at a step that is a function of (s, m, nr, w, wleft) alone, strictly increasing in s -- at most one event of
    // a kind per step.  So the schedule is three wave-uniform timers, each with the superblock it fires for, advanced
    // with scalar arithmetic in the handler; no lane carries a timer and the step loop tests nothing.
    //   open  (s): max(1, s*RB + 1 - wleft) + s             the window of superblock s opens: Pv = ~0, Mv = 0
    //   close (s): min(m, s*RB + RB + w) + s + 1            first step after the window: the lane moves on to s + 64,
    //                                                       and from this step on its hout is no window cell (`live`)
    //   seg      : i + s + 1 for rows i = 32, 64, .., m     the 32-row diagonal segment ending at row i (of superblock
    //                                                       s = (i-1)/RB) was completed by the step before.  Where it
    //                                                       ends its superblock it also lets the diagonal into the next
    //                                                       one, which it reaches two steps later (`one`)
    //   diag  (s): s*(RB+1) + 1, while s*RB < m             the forms without DIAG_FOLD only (below): the diagonal enters
    //                                                       the superblock's first row
    int T_open = 1, s_op = 0;
    int T_close = min(m, RB + w) + 1, s_cl = 0;
    int T_diag = 1, s_dg = 0;                    // (the forms without DIAG_FOLD, below)
    int T_seg = min(32, m) + 1, s_sg = 0;
    int s_next = 1;                              // the earliest of them
    (void)T_diag; (void)s_dg;
    // Which superblock a lane holds, and whether its window is open, belong to the schedule too: a lane moves on to s + 64
    // when superblock s closes, closes fire in the order of s, so the lanes hold s_cl .. s_cl + 63; the open windows are those
    // of s_cl .. s_op - 1.  The RING forms keep neither in a vector register: the few places that ask (a chunk's start, the
    // end) derive them, which is what lets the ring's two-step stretch into 64 registers without a spilled word more.  The
    // other forms (LANE_SB) keep both in the lane, updated by the events, as they always did.  (Macros, not lambdas: two
    // more closures over the schedule's scalars cost k_cigar_pairs<4> and k_vote_pairs<4, true, false> a wave per SIMD.)
    constexpr bool LANE_SB = !RING;
#define PBA_BV_LANE_SB() (LANE_SB ? s_cur : SHIFT ? lsh_sb(lane, s_cl) : s_cl + ((lane - s_cl) & (PBA_WAVE - 1)))
#define PBA_BV_LANE_OF(s) (SHIFT ? lsh_lane(s, s_cl) : (s) & (PBA_WAVE - 1))   /* the lane of superblock s, s_cl as it is now */
#define PBA_BV_LANE_OPEN() (LANE_SB ? opened != 0 : PBA_BV_LANE_SB() < s_op)
    // Where the diagonal is: at any step it is in one block of one lane, or in none (the one-step gap between two
    // superblocks, and past row m).  Both are wave-uniform and belong to the schedule: `one` is the one-hot of the diagonal
    // cell's bit in its block's word, qd that block.  `one` is 64 bits wide and the block's word is its HIGH half: bit 32 + r
    // is row r of the block, and the step's one scalar shift moves it a row down.  segment_done sets both: a segment that
    // ends inside its superblock re-arms bit 32; one that ends its superblock (rows left) arms bit 31 -- the gap step between
    // the two superblocks, in which the high half is 0 and nothing collects, shifts it to bit 32, and the first row of the
    // next superblock collects at bit 0 of its word; the segment holding row m leaves 0.  Superblock 0 is entered in front of
    // the loop.  There is no diagonal-entry event.
    // DIAG_FOLD: not with six blocks per lane -- the pair of registers `one` travels in between stretches takes k_locate<6>
    // from 80 to 84 vector registers, a wave per SIMD.  That ring keeps the 32-bit one-hot and
    // the diagonal-entry event of the LANE_HOT form (T_diag).
    constexpr bool DIAG_FOLD = !BAIL && NB != 6;
    constexpr int OH_SH = DIAG_FOLD ? 32 : 0;    // where the block's word sits in `one`
    typedef typename std::conditional<DIAG_FOLD, uint64_t, uint32_t>::type onehot_t;
    onehot_t one = DIAG_FOLD ? (onehot_t)1 << OH_SH : 0;
    int qd = 0;
    // Not in the BAIL form (the all-vs-all walk): its candidates are mostly false ones that die within their first segments,
    // on the ramp, where a window opens at every step and a stretch is one step long -- there the scalar one-hot's two
    // instructions per stretch (read in front, written back behind) cost more than the step saves (measured: walk + 4 to 6 %,
    // DESIGN.md 4.3 round 8).  That form keeps the one-hot in the diagonal's lane, advanced by a vector add: dmw.
    constexpr bool LANE_HOT = BAIL;
    // There the lane below cannot be armed a step early: the add doubles dmw, and no 32-bit value doubles to 1.  That form
    // keeps its diagonal-entry event (T_diag).
    uint32_t dmw = 0;                            // LANE_HOT: bit of the diagonal cell in its block's word (0: not in this lane)
    (void)dmw; (void)one; (void)qd;

    uint32_t wl = 0, wh = 0;                     // text bit planes: bit k = low / high bit of the element of step tb+k
    // RING: no planes -- the text comes from the wavefront's ring in LDS (text_ring.h), PBA_TXR_BYTES behind the fin words:
    // ta is this lane's cell for the step at hand, one cell further every step
    // EQT: the ring's cell is the byte offset of the letter's rows in the lane's table (eq_table.h: eqt_cell), behind the table.
    // Every cell gets a letter in front of the sweep: a lane steps before its window opens and after it has closed, through
    // cells no chunk of this sweep has written, and what it finds there is an address.
    typedef __attribute__((address_space(3))) typename std::conditional<EQT, uint32_t, uint64_t>::type txr_cell;
    txr_cell *const ring = (txr_cell *)(fin + (EQT ? PBA_EQT_LETTERS * NB * PBA_EQT_LANES : PBA_BV_FIN_WORDS(NB)));
    const txr_cell *ta = ring;
    (void)wl; (void)wh; (void)ring; (void)ta;
    if constexpr (EQT) {
        static_assert(PBA_TXR_SLOTS <= 3 * PBA_WAVE && PBA_TXR_SLOTS > 2 * PBA_WAVE, "three cells per lane cover the ring");
        ring[lane] = 0; ring[PBA_WAVE + lane] = 0;
        if (lane < PBA_TXR_SLOTS - 2 * PBA_WAVE) ring[2 * PBA_WAVE + lane] = 0;
    }
    // wave-uniform, in scalar registers: the running D(i,i) at the end of the last segment judged (segments end in row
    // order, so it simply carries on from lane to lane) and the first failing row (0: none so far)
    int score = 0, fail_row = 0;
    // the vertical deltas of the LAST column as this lane's last superblock at or below row m left them (a lane keeps
    // stepping on garbage after its window has closed, so they are put aside at the close); fin_s: that superblock, or -1
    // They live in LDS (fin: PBA_BV_FIN_WORDS(NB) u32 of this wavefront's own: [2*nb][lane] Pv, [2*nb+1][lane] Mv, [2*NB][lane]
    // the superblock): written once per superblock that reaches the last column, read once at the end -- as registers
    // they were live through the whole step loop, and at 64 registers per lane the compiler spilled them to scratch memory.
    fin[FIN_SB + lane] = 0xFFFFFFFFu;
    uint64_t hp_last = ~0ull, hn_last = 0ull;    // lane masks: delta +1 / -1 leaving each lane's last block in the previous step
    // What a lane hands out is masked, not what a lane takes in.  live: the lanes whose hout of the step just run is a window
    // cell that the lane below takes; hpm / hnm: that step's carries under it -- "+1 per column", the row above a window,
    // where the bit is clear -- which the next step rotates one lane up.
    // Derivation, from the taking side: let valid(t) bit k say that lane k's first block takes lane k - 1's hout of step
    // t - 1 at step t.  It holds for lane s & 63 from the step it takes superblock s (0 < s < S) through step close(s - 1),
    // whose column is the last of the window above.  live after step t is valid(t + 1) rotated one lane down:
    //   * at the start valid is lanes 1 .. min(S, 64) - 1 (lane 0's superblock 0 has the top border above it, and the lanes
    //     >= S hold nothing), so live is lanes 0 .. min(S, 64) - 2;
    //   * lane s & 63 hands out its last window cell in step close(s) - 1, taken at step close(s): its bit is cleared by
    //     the close event itself, which runs in front of step close(s) and so first masks that step's carries;
    //   * lane (s - 1) & 63, which holds superblock s + 63 by then, hands out to superblock s + 64 from the step lane s & 63
    //     takes that superblock, close(s): its bit is set there when s + 64 < S, and this one must already hold for the
    //     carries of step close(s) - 1 -- the window of s + 64 may open at close(s) itself (bv_max_span) and take them.
    //     They are still at hand unmasked (hp_last / hn_last), so the event forms hpm / hnm again under the new bit, then
    //     clears its own.  (When s + 64 >= S the bit stays as close(s - 1) left it: clear.)
    // hp_last / hn_last stay the raw carries of the step: what a checkpoint holds (bv_ckpt_store, bitvec_rerun).
    // SHIFT has neither `live` nor the raw carries: lane 0 is the one lane that takes the border, in every step but the one
    // right behind a close (lane_shift.h reads the derivation above for that mapping).
    uint64_t live = (S >= PBA_WAVE ? ~0ull : (1ull << S) - 1ull) >> 1;
    uint64_t hpm = ~0ull, hnm = 0ull;

    // text planes for the 32 steps starting at the wave-uniform step tb (element of step t is t - 1 - the lane's superblock)
    // RING: the wavefront fetches the chunk's 32 new elements once and every lane writes one cell -- lanes 0..31
    // element first + lane at its slot, lanes 32..63 the same elements' second copies where a slot has one (else the
    // first copy once more) -- then takes its own address.  A wavefront's LDS operations complete in order: no wait.
    auto load_text = [&](int tb) {
        if constexpr (RING) {
            const int first = txr_fetch_first(tb, s_cl);
            uint32_t plo, phi;
            load_planes32(colsF, first, plo, phi);
            const int c = lane & (PBA_TXR_CHUNK - 1), slot = txr_slot(first + c), mir = txr_mirror(slot);
            const int dst = (lane >= PBA_TXR_CHUNK && mir >= 0) ? mir : slot;
            if constexpr (EQT) ring[dst] = (((plo >> c) & 1u) | (((phi >> c) & 1u) << 1)) * (uint32_t)(NB * PBA_EQT_LANES * 4);   // eqt_cell(letter)
            else ring[dst] = (uint64_t)(0u - ((plo >> c) & 1u)) | ((uint64_t)(0u - ((phi >> c) & 1u)) << 32);
            ta = ring + txr_addr(tb, PBA_BV_LANE_SB());
        } else {
            load_planes32(colsF, tb - PBA_BV_LANE_SB() - 1, wl, wh);
        }
    };

    // The 32-row diagonal segment of superblock s ending at row i (a multiple of 32, or m) is complete: check its rows
    // against seq_aligner.h:185 and carry the diagonal score on.  Judged on the scalar side: s, i, the running score and
    // the verdict are wave-uniform, and the one datum a lane holds -- the segment's word, acc[q] of lane s & 63 -- comes
    // over with one v_readlane.  The FP64 comparisons run on uniform operands (the scalar unit has no FP64) and their
    // result is a scalar condition.  What is left for the lane: its acc[] cleared.  The one-hot is re-armed on the scalar side.
    // Every lane ORs D0 bits into its acc[qd] under the wave's one-hot, whether the diagonal is in it or not; only acc[q] of
    // lane s & 63 is ever read, here.  That is harmless only because a lane's acc[] is cleared when the diagonal enters the
    // lane (below, at the segment end in front of it; without DIAG_FOLD: the diagonal-entry event) and at every segment
    // end: both clears must stay.
    // Returns 0, or the first failing row (PBA_BV_BAIL: the sweep is given up); a sweep ends at its first failure, so
    // no segment is judged after one.
    auto segment_done = [&](int s, int i) -> int {
        const int rr = i - 1 - s * RB, cnt = (rr & 31) + 1, i0 = i - cnt, q = rr >> 5;
        const int L = PBA_BV_LANE_OF(s);
        uint32_t dw = 0;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) if (q == nb) dw = __builtin_amdgcn_readlane(acc[nb], L);
        dw &= 0xFFFFFFFFu >> (32 - cnt);
        // D(i0+k, i0+k) = score + k - popcount(low k bits of dw); non-decreasing in k
        const int end = score + cnt - __builtin_popcount(dw);
        const int ifirst = max(i0 + 1, 11);                                   // rows <= 10 are never checked
        int fr = 0;
        if (i >= ifirst && (double)end > (double)ifirst * R) {
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)     // (rare, and it ends within a few rows)
            for (int k = ifirst - i0; k <= cnt; ++k) {                        // row by row
                const int d = score + k - __builtin_popcount(dw & (0xFFFFFFFFu >> (32 - k)));
                if ((double)d > (double)(i0 + k) * R) { fr = i0 + k; break; }
            }
        }
        if constexpr (BAIL) {
            if (bail_w > 0 && i >= 1024 && fr == 0 &&
                ((float)end - 4.0f * __builtin_sqrtf((float)end)) * (float)m > (float)i * (float)bail_w) fr = PBA_BV_BAIL;
        }
        score = end;                                     // D(i,i): the next segment starts from it, in whichever lane
        // the diagonal leaves this lane's rows for the lane below (its word is cleared here, one step early: nothing
        // collects in the gap step), or enters this lane's next block at bit 0
        const bool leaves = rr == RB - 1 && i != m;
        if (lane == L || (DIAG_FOLD && leaves && lane == PBA_BV_LANE_OF(s + 1))) {
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb] = 0; // the next block's word starts clean
            if constexpr (LANE_HOT) dmw = (i == m || rr == RB - 1) ? 0u : 1u;
        }
        if constexpr (DIAG_FOLD) one = i == m ? 0 : (onehot_t)1 << (leaves ? OH_SH - 1 : OH_SH);
        else one = (i == m || rr == RB - 1) ? 0u : 1u;
        qd = (q + 1) % NB;                               // (0 where the diagonal leaves the superblock)
        return fr;
    };

    // The events due at step t (== s_next), before the step runs: segment end, close / move on, open (without DIAG_FOLD: diagonal entry).
    // DIAG: phase 1 (the diagonal is still being swept).  Sets seg_fail when a segment's check failed.
#define PBA_BV_EVENTS(DIAG)                                                           \
    {                                                                                 \
        if (DIAG && t == T_seg) {                                                     \
            const int s = s_sg, i = t - 1 - s;                                        \
            seg_fail = segment_done(s, i);                                            \
            if (i == m) T_seg = INT_MAX;                                              \
            else { s_sg = s + (i == s * RB + RB ? 1 : 0); T_seg = min(i + 32, m) + s_sg + 1; } \
        }                                                                             \
        if (t == T_close) {                                                           \
            const int s = s_cl;                                                       \
            if constexpr (SHIFT) {                                                    \
                /* lane_shift.h: lane 0 keeps its last column, every lane takes the state of the lane below it, the last \
                   lane its next superblock's rows in the column lane 0 leaves */ \
                if (lane == 0 && s >= s_m) {                                        \
                    tab_lane[FIN_SB] = (uint32_t)s;                                   \
                    _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) { tab_lane[2 * nb * PBA_WAVE] = Pv[nb]; tab_lane[(2 * nb + 1) * PBA_WAVE] = Mv[nb]; } \
                }                                                                     \
                _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) {                   \
                    Pv[nb] = bv_lane_below(Pv[nb]); \
                    Mv[nb] = bv_lane_below(Mv[nb]); \
                    acc[nb] = bv_lane_below(acc[nb]); \
                }                                                                     \
                s_cl = s + 1;                /* from here on the lanes' columns are those of s + 1 .. s + 64 */ \
                if (lane == PBA_WAVE - 1 && s + PBA_WAVE < S) { PBA_BV_FILL_ROWS(s + PBA_WAVE) } \
                ta = ring + lsh_ring_addr(t, lane, s_cl);                             \
                closed = true;               /* this step takes the carries unshifted: the lanes moved (PBA_BV_HIN) */ \
            } else {                                                                \
            if (lane == (s & (PBA_WAVE - 1))) {                                       \
                if (s >= s_m) {              /* its window ended with the last column: keep that column */ \
                    fin[FIN_SB + lane] = (uint32_t)(LANE_SB ? s_cur : s);  \
                    _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) { fin[2 * nb * PBA_WAVE + lane] = Pv[nb]; fin[(2 * nb + 1) * PBA_WAVE + lane] = Mv[nb]; } \
                }                                                                     \
                /* the lane's next superblock: its rows, and its slice of the text (a lane that opens its first window \
                   already got its planes at the start of the chunk: no load, no wait -- during the ramp one lane opens \
                   per step, and false candidates are all ramp) */                    \
                if constexpr (LANE_SB) { s_cur += PBA_WAVE; opened = 0; }             \
                const int sn = LANE_SB ? s_cur : s + PBA_WAVE;                        \
                /* EQT: its match masks.  Never after the fin words went onto the lane's rows above: s >= s_m and \
                   S - s_m < 64 (the windows span at most bv_max_span rows) give s + 64 >= S (eq_table.h) */ \
                if (s + PBA_WAVE < S) {                                               \
                    if constexpr (EQT) { PBA_BV_FILL_ROWS(sn) } else {                \
                    _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) load_planes32(rowsF, sn * RB + 32 * nb, Plo[nb], Phi[nb]); \
                    }                                                                 \
                }                                                                     \
                if constexpr (RING) ta = ring + txr_addr(t, sn);      /* 64 elements back; they are in the ring */ \
                else load_text(t - ((t - 1) & 31));                                   \
            }                                                                         \
            /* the lane above hands out to this lane's next superblock, the carries of the step before included; this \
               lane's own hout is no window cell from this step on (`live` above) */  \
            if (s + PBA_WAVE < S) {                                                   \
                live |= 1ull << ((s - 1) & (PBA_WAVE - 1));                           \
                hpm = bv_orn2(hp_last, live); hnm = bv_and2(hn_last, live);           \
            }                                                                         \
            live &= ~(1ull << (s & (PBA_WAVE - 1)));                                  \
            }                                                                         \
            s_cl = s + 1;                                                             \
            T_close = s_cl < S ? min(m, s_cl * RB + RB + w) + s_cl + 1 : INT_MAX;     \
        }                                                                             \
        if (t == T_open) {                                                            \
            if (lane == PBA_BV_LANE_OF(s_op)) {                                       \
                _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) { Pv[nb] = ~0u; Mv[nb] = 0u; } \
                if constexpr (LANE_SB) opened = 1;                                    \
            }                                                                         \
            s_op += 1;                                                                \
            T_open = s_op < S ? max(1, s_op * RB + 1 - wleft) + s_op : INT_MAX;       \
        }                                                                             \
        if constexpr (!DIAG_FOLD) {                                                   \
            if (DIAG && t == T_diag) {                                                \
                if (lane == (s_dg & (PBA_WAVE - 1))) {                                \
                    _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) acc[nb] = 0;    \
                    if constexpr (LANE_HOT) dmw = 1u;                                 \
                }                                                                     \
                one = 1u; qd = 0;                                                     \
                s_dg += 1;                                                            \
                T_diag = s_dg * RB < m ? s_dg * (RB + 1) + 1 : INT_MAX;               \
            }                                                                         \
        }                                                                             \
        s_next = min(T_open, T_close);                                                \
        if (DIAG) s_next = min(s_next, DIAG_FOLD ? T_seg : min(T_seg, T_diag));       \
        if constexpr (TRACE == 1) st_on = ((__builtin_amdgcn_ballot_w64(PBA_BV_LANE_OPEN()) >> (lane & 48)) & 0xFFFFull) != 0; \
    }

    // hin of each lane's first block: the lane above's hout of the previous step, rotated one lane up, where that
    // hout was a window cell this lane takes; elsewhere the row above the window counts "+1 per column" (`live` above:
    // masked where it is handed out, PBA_BV_HOUT)
    // SHIFT: lane 0 is the top of the band and takes the border, every other lane its neighbour's hout as it is; CLOSED: the
    // one step behind a close, where the lanes have moved one up instead and the carries are taken where they are (lane_shift.h)
#define PBA_BV_HIN(CLOSED)                                                            \
    uint64_t hp = SHIFT ? ((CLOSED) ? hpm : bv_shl1_or1(hpm)) : (hpm << 1) | (hpm >> 63); \
    uint64_t hn = SHIFT ? ((CLOSED) ? hnm : bv_shl1(hnm)) : (hnm << 1) | (hnm >> 63);
#define PBA_BV_HOUT()                                                                 \
    if constexpr (SHIFT) { hpm = hp; hnm = hn; } else {                               \
    hp_last = hp; hn_last = hn;                                                       \
    hpm = bv_orn2(hp, live); hnm = bv_and2(hn, live);                                 \
    }

    // one block update (hp / hn: lane masks of the delta entering at the block's top row, replaced by the one leaving)
    // D0 (bit r set iff D(i,j) == D(i-1,j-1)) doubles as Myers' Xv in the two vertical updates (Hyyro's form of
    // the recurrences: wherever D0 and Eq | Mv differ a carry came in from the row above, whose horizontal delta is
    // then -1, and both forms give Pv' = 1, Mv' = 0)
#define PBA_BV_BLOCK(nb, PH_PRE, MH_PRE, D0, EQ)                                     \
    {                                                                                \
        const uint32_t Eq = EQT ? eqr[nb] : eq_mask(Plo[nb] ^ clo, Phi[nb], chi);    \
        EQ = Eq;                                                                     \
        const uint32_t pv = Pv[nb], mv = Mv[nb];                                     \
        uint64_t unused;                                                             \
        const uint32_t sum = addc_mask(Eq & pv, pv, hn, unused);   /* hn as carry-in == Eq |= 1 at the top row */ \
        const uint32_t Xh = (sum ^ pv) | Eq;                                         \
        const uint32_t Ph = mv | ~(Xh | pv);                                         \
        const uint32_t Mh = pv & Xh;                                                 \
        D0 = Xh | mv;                                                                \
        PH_PRE = Ph; MH_PRE = Mh;                                                    \
        const uint32_t Ph2 = addc_mask(Ph, Ph, hp, hp);                              \
        const uint32_t Mh2 = addc_mask(Mh, Mh, hn, hn);                              \
        Pv[nb] = Mh2 | ~(D0 | Ph2);                                                  \
        Mv[nb] = Ph2 & D0;                                                           \
    }

    // TRACE: this lane's slot of step t, block 0, word 0.  Recomputed from t every step: a pointer carried through
    // the loop loses its increment on the text-refill path of the step loop (ROCm 7.2 clang, seen in the ISA)
    uint2 *const tr_lane = (uint2 *)tr + lane;
    (void)tr_lane;
    bool st_on = false;          // TRACE: some lane of this lane's 16-lane group is inside its window (updated at events)
    (void)st_on;
#define PBA_BV_TRP() (tr_lane + (size_t)(t - 1) * (NB * 64))
    // One stretch of phase 1: plain steps from k up to kstop.  QD: the block the diagonal is in, as a constant (its word
    // alone collects), or -1: every block's word collects (garbage in all but the diagonal's, cleared at the segment's end).
    // LANE_HOT: every block's word collects under the lane's own one-hot.
    // EQT: the step's match masks were read ahead (eqn[OFS][], PBA_BV_ROWS)
#define PBA_BV_TEXT(OFS)                                                             \
        uint32_t clo = 0, chi = 0, eqr[NB];                                          \
        _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) eqr[nb] = eqn[OFS][nb];    \
        (void)clo; (void)chi; (void)eqr;                                             \
        if constexpr (EQT) { }                                                       \
        else if constexpr (RING) { const uint64_t cell = ta[OFS]; clo = (uint32_t)cell; chi = (uint32_t)(cell >> 32); } \
        else { clo = bit_mask(wl, k + (OFS)); chi = bit_mask(wh, k + (OFS)); }
    // EQT: the match masks of the step whose cell is cq[OFS] -- the lane's own address plus the cell, both blocks with one read
#define PBA_BV_ROWS(OFS)                                                             \
        {                                                                            \
        const lds_u32 *const row = (const lds_u32 *)((const __attribute__((address_space(3))) uint8_t *)tab_lane + cq[OFS]); \
        _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) eqn[OFS][nb] = row[nb * PBA_EQT_LANES]; \
        }
#define PBA_BV_STEP1(QD, OFS) PBA_BV_STEP1X(QD, OFS, false)
#define PBA_BV_STEP1X(QD, OFS, CLOSED)                                               \
        {                                                                            \
        const int t = tb + k + (OFS);                                                \
        (void)t;                                                                     \
        PBA_BV_TEXT(OFS)                                                             \
        PBA_BV_HIN(CLOSED);                                                              \
        _Pragma("unroll")                                                            \
        for (int nb = 0; nb < NB; ++nb) {                                            \
            uint32_t d0, php, mhp, eq;                                               \
            PBA_BV_BLOCK(nb, php, mhp, d0, eq);                                      \
            (void)php; (void)mhp; (void)eq;                                          \
            if constexpr (TRACE == 1) {      /* whole 128-byte lines only: a 16-lane group stores when any of its lanes is */ \
                if (st_on)                   /* inside its window (masking lane by lane was measured 1.5x SLOWER: partial lines) */ \
                    PBA_BV_TRP()[nb * 64] = make_uint2(eq | ~d0, swap_roles ? Pv[nb] : php); \
            }                                                                        \
            /* keep the diagonal cell's D0 bit: in every lane, under the wave's one-hot (what a lane without the diagonal \
               collects is cleared when the diagonal enters it) */                   \
            if constexpr (LANE_HOT) acc[nb] = or_of_and(acc[nb], d0, dmw); else       \
            if ((QD) < 0 || nb == (QD)) acc[nb] = or_of_and_s(acc[nb], d0, (uint32_t)(oh >> OH_SH)); \
        }                                                                            \
        PBA_BV_HOUT()                                                                \
        /* next row of the block, on the scalar side; re-armed every 32 rows.  (LANE_HOT: a full-rate add the compiler cannot \
           turn back into the slower shift) */                                       \
        if constexpr (LANE_HOT) asm("v_add_u32 %0, %1, %1" : "=v"(dmw) : "v"(dmw)); else oh <<= 1; \
        }
    // RING: the stretch runs two steps per turn -- both steps' cells come with one LDS instruction, and the address add, the
    // counter, the compare and the branch are paid once per two steps; an odd stretch (every stretch of a ramp is one step) takes
    // its odd step first.
    // EQT: two LDS trips stand between a step and its masks, the cell and then the rows.  A turn takes both steps' cells with
    // one read and both steps' rows in front of its first step, so the second step never waits.  (Reading the next turn's
    // cells a turn ahead was written too: the compiler moves that read back to the top of the turn that uses it, and at
    // eight waves per SIMD the other waves cover the trip.  DESIGN.md 4.3, round 12.)
#define PBA_BV_STRETCH1(QD)                                                          \
        uint32_t cq[2] = {0u, 0u}, eqn[2][NB] = {};                                  \
        (void)cq; (void)eqn;                                                         \
        if constexpr (EQT) {                                                         \
            if ((kstop - k) & 1) { cq[0] = ta[0]; PBA_BV_ROWS(0) PBA_BV_STEP1(QD, 0) ta += 1; k += 1; } \
            while (k < kstop) {                                                      \
                cq[0] = ta[0]; cq[1] = ta[1];                                        \
                PBA_BV_ROWS(0) PBA_BV_ROWS(1)                                        \
                PBA_BV_STEP1(QD, 0)                                                  \
                _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) asm("" : "+v"(Pv[nb]), "+v"(Mv[nb])); \
                PBA_BV_STEP1(QD, 1)                                                  \
                ta += 2; k += 2;                                                     \
            }                                                                        \
        } else if constexpr (RING) {                                                 \
            if ((kstop - k) & 1) { PBA_BV_STEP1(QD, 0) ta += 1; k += 1; }            \
            while (k < kstop) {                                                      \
                PBA_BV_STEP1(QD, 0)                                                  \
                /* the first step's Pv / Mv as registers: seen through, the compiler folds them into the second step's \
                   expressions and spends two instructions more per block on that */ \
                _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) asm("" : "+v"(Pv[nb]), "+v"(Mv[nb])); \
                PBA_BV_STEP1(QD, 1)                                                  \
                ta += 2; k += 2;                                                     \
            }                                                                        \
        } else {                                                                     \
            do { PBA_BV_STEP1(QD, 0) } while (++k < kstop);                          \
        }
    // ------------------------------------------------------------------ phase 1: down to cell (m,m)
    // The step loop is cut into chunks of 32 steps (one pair of text planes): the scalar unit is shared by the CU's
    // four SIMDs, so every SALU instruction of the step costs four issue cycles -- the inner loop carries nothing
    // but its counter.  Everything in it is wave-uniform and stays in SGPRs.
    // Within a chunk the steps run in stretches that end at the next scheduled event: the stretch's bound is its loop
    // counter, and its body is the block updates, the hand-off rotate and the one-hot's scalar shift -- no compare, no
    // branch on a lane mask.
    for (int tbv = 1; tbv <= t1; tbv += 32) {
        const int tb = __builtin_amdgcn_readfirstlane(tbv);   // (the early exit below makes the compiler treat tbv as divergent)
        if constexpr (TRACE == 2) bv_ckpt_store<NB>(tr, tb, lane, Pv, Mv, PBA_BV_LANE_SB(), LANE_SB ? opened : (PBA_BV_LANE_OPEN() ? 1u : 0u), hp_last, hn_last);
        load_text(tb);                           // next text planes
        if (fail_row) break;
        int kend = min(32, t1 - tb + 1);
        for (int k = 0; k < kend;) {
        bool closed = false;                     // SHIFT: a close fired in front of this step
        (void)closed;
        if (tb + k == s_next) {
            const int t = tb + k;
            int seg_fail = 0;
            PBA_BV_EVENTS(true);
            // a segment that just ended may have failed the reference's check: leave right after this step (false
            // candidates die on their first segment, so they cost 33 steps, not the 64 of a poll per chunk)
            if (seg_fail) { fail_row = seg_fail; kend = k + 1; }
        }
        if constexpr (SHIFT && !PBA_BV_CLOSE_INLINE) {
            // (-DPBA_BV_CLOSE_INLINE=0: the step behind a close ends the handler's iteration and runs on its own in another)
            if (closed) {
                onehot_t oh = (onehot_t)bv_uniform64(one);
                uint32_t cq[1] = {ta[0]}, eqn[1][NB];
                PBA_BV_ROWS(0)
                PBA_BV_STEP1X(NB == 1 ? 0 : -1, 0, true)
                one = oh;
                ta += 1; k += 1;
                continue;
            }
        }
        // The one-hot goes through the stretch in a local read with v_readfirstlane: `one` is set inside a loop that a
        // failing segment leaves early, so the compiler would carry it in a vector register and shift it there (the
        // same effect as for tbv and score).  qd is constant within a stretch (a segment end is a scheduled event), so with
        // two blocks the stretch exists once per block, behind a scalar branch: no word of the other block is touched.
        // Not in the streamed trace form, where the second copy costs k_trace_pairs<2, false> a wave per SIMD, and not for
        // NB >= 3, where the copies cost registers or scratch in every kernel: there every block's
        // word collects under the scalar one-hot.
        onehot_t oh = 0;
        if constexpr (DIAG_FOLD) oh = (onehot_t)bv_uniform64(one);
        else if constexpr (!LANE_HOT) oh = __builtin_amdgcn_readfirstlane(one);
        if constexpr (SHIFT && PBA_BV_CLOSE_INLINE) {
            // The step behind a close takes the carries unshifted (PBA_BV_HIN).  It runs here, inside the close's own
            // iteration, under the one-hot the stretch behind it goes on with: the iteration's one pass through the
            // stretch's prologue serves both.  Every block's word collects under the one-hot (what lands in a word the
            // diagonal is not in is cleared at the segment's end, as in the rings 3 and up).  The stretch then runs from
            // the step behind it: k <= kend and tb + k <= s_next hold (k < kend in front of the step; the events of step t
            // leave s_next > t), so the stretch's bound is never below k, and it is k where a failed segment or the
            // chunk's end or another event ends the iteration right here.
            if (closed) {
                uint32_t cq[1] = {ta[0]}, eqn[1][NB];
                PBA_BV_ROWS(0)
                PBA_BV_STEP1X(NB == 1 ? 0 : -1, 0, true)
                ta += 1; k += 1;
            }
        }
        const int kstop = min(kend, s_next - tb);
        if constexpr (NB == 2 && TRACE != 1 && !LANE_HOT) {
            if (__builtin_amdgcn_readfirstlane(qd) == 0) { PBA_BV_STRETCH1(0); } else { PBA_BV_STRETCH1(1); }
        } else {
            PBA_BV_STRETCH1(NB == 1 ? 0 : -1);
        }
        if constexpr (!LANE_HOT) one = oh;
        }
    }
    if (fail_row == 0) fail_row = segment_done(s_m, m);   // the segment that ended in the last step: the one holding row m
    if (fail_row) return __builtin_amdgcn_readfirstlane(fail_row);
    s_next = min(T_open, T_close);               // the diagonal is done: what is left opens and closes windows
    // (Formed again from the raw carries rather than carried over: phase 1's loop has an early exit, and the compiler takes
    // what that loop leaves behind for divergent -- two values fewer to bring back to the scalar side.)
    if constexpr (SHIFT) { hpm = bv_uniform64(hpm); hnm = bv_uniform64(hnm); }        // (SHIFT: the carries as they are, no mask)
    else { hpm = bv_orn2(hp_last, live); hnm = bv_and2(hn_last, live); }

    // ------------------------------------------------------------------ phase 2: the superblocks below row m take the last column
    for (int tb = t1 + 1; tb <= t_end;) {
        const int k0 = (tb - 1) & 31;            // phase 2 starts inside a chunk whose planes are already loaded
        if (k0 == 0) {
            if constexpr (TRACE == 2) bv_ckpt_store<NB>(tr, tb, lane, Pv, Mv, PBA_BV_LANE_SB(), LANE_SB ? opened : (PBA_BV_LANE_OPEN() ? 1u : 0u), hp_last, hn_last);
            load_text(tb);
        }
        const int kend = min(32, k0 + (t_end - tb + 1));
        const int tc = tb - k0;                  // first step of the chunk
        for (int k = k0; k < kend;) {
        bool closed = false;
        (void)closed;
        if (tc + k == s_next) {
            const int t = tc + k;
            int seg_fail = 0;
            (void)seg_fail;
            PBA_BV_EVENTS(false);
        }
#define PBA_BV_STEP2(CLOSED)                                                          \
        {                                                                             \
        const int t = tc + k;                                                         \
        (void)t;                                                                      \
        uint32_t cq[1] = {0u}, eqn[1][NB] = {};                                       \
        (void)cq; (void)eqn;                                                          \
        if constexpr (EQT) { cq[0] = ta[0]; PBA_BV_ROWS(0) }                          \
        PBA_BV_TEXT(0)                                                                \
        PBA_BV_HIN(CLOSED);                                                           \
        _Pragma("unroll")                                                             \
        for (int nb = 0; nb < NB; ++nb) {                                             \
            uint32_t d0, php, mhp, eq;                                                \
            PBA_BV_BLOCK(nb, php, mhp, d0, eq);                                       \
            (void)d0; (void)eq; (void)php; (void)mhp;                                 \
            if constexpr (TRACE == 1) {      /* whole 128-byte lines only: a 16-lane group stores when any of its lanes is */ \
                if (st_on)                   /* inside its window (masking lane by lane was measured 1.5x SLOWER: partial lines) */ \
                    PBA_BV_TRP()[nb * 64] = make_uint2(eq | ~d0, swap_roles ? Pv[nb] : php); \
            }                                                                         \
        }                                                                             \
        PBA_BV_HOUT()                                                                 \
        if constexpr (RING) ta += 1;                                                  \
        }
        if constexpr (SHIFT) {
            if (closed) {                                          // the step behind a close (phase 1 above)
                PBA_BV_STEP2(true)
                k += 1;
                if (!PBA_BV_CLOSE_INLINE || k >= min(kend, s_next - tc)) continue;
            }
        }
        const int kstop = min(kend, s_next - tc);
        do { PBA_BV_STEP2(false) } while (++k < kstop);
        }
        tb += kend - k0;
    }
#undef PBA_BV_STRETCH1
#undef PBA_BV_STEP2
#undef PBA_BV_STEP1X
#undef PBA_BV_STEP1
#undef PBA_BV_ROWS
#undef PBA_BV_TEXT
#undef PBA_BV_FILL_ROWS
#undef PBA_BV_BLOCK
#undef PBA_BV_TRP
#undef PBA_BV_HOUT
#undef PBA_BV_HIN
#undef PBA_BV_EVENTS
    // ------------------------------------------------------------------ the free end: first strict minimum down the last column
    // D(i,m) = D(m,m) + the vertical deltas of column m over rows m+1..i (seq_aligner.h:192-211 scans exactly these cells,
    // upward from the diagonal, and keeps the first strict minimum).  A lane whose window is still open holds the
    // column in Pv / Mv, the others put it aside when their window closed.
    // SHIFT: into the superblock's column, sb & 63 -- what follows reads column `lane`, whichever lane wrote it
    if (const int sb = PBA_BV_LANE_SB(); PBA_BV_LANE_OPEN() && sb >= s_m && sb < S) {
        const int col = SHIFT ? lsh_col(lane, s_cl) : lane;
        fin[FIN_SB + col] = (uint32_t)sb;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) { fin[2 * nb * PBA_WAVE + col] = Pv[nb]; fin[(2 * nb + 1) * PBA_WAVE + col] = Mv[nb]; }
    }
#undef PBA_BV_LANE_OPEN
#undef PBA_BV_LANE_SB
#undef PBA_BV_LANE_OF
#undef tab_lane
    const int fin_s = (int)fin[FIN_SB + lane];      // (a wavefront's LDS operations complete in order: no barrier)
    int b_tot[NB], b_min[NB], b_pos[NB];          // per block of this lane's last superblock: sum, lowest prefix sum, its bit
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row0 = fin_s * RB + nb * 32;    // bit r is row row0 + r + 1
        const uint32_t fpv = fin_s >= 0 ? fin[2 * nb * PBA_WAVE + lane] : 0u, fmv = fin_s >= 0 ? fin[(2 * nb + 1) * PBA_WAVE + lane] : 0u;
        int v = 0, pm = INT_MAX, pp = 0;
        for (int r = 0; r < 32; ++r) {
            const int row = row0 + r + 1;
            if (fin_s >= 0 && row > m && row <= nr) {
                v += (int)((fpv >> r) & 1u) - (int)((fmv >> r) & 1u);
                if (v < pm) { pm = v; pp = r; }
            }
        }
        b_tot[nb] = v; b_min[nb] = pm; b_pos[nb] = pp;
    }
    // v_readlane: the results are wave-uniform and the compiler must know it, or every loop that depends on
    // them (the callers' candidate walks, and through their lengths this function's own step loop) is treated
    // as divergent and its counters and bounds move from SGPRs into VGPRs
    int gbest = __builtin_amdgcn_readfirstlane(score), gi = m, run = gbest;   // D(m,m): where the scan down the last column starts
    diag_out = gbest;
    for (int sb = s_m; sb < S; ++sb) {
        const int L = sb & (PBA_WAVE - 1);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const int pm = __builtin_amdgcn_readlane(b_min[nb], L);
            if (pm != INT_MAX && run + pm < gbest) {
                gbest = run + pm;
                gi = sb * RB + nb * 32 + __builtin_amdgcn_readlane(b_pos[nb], L) + 1;
            }
            run += __builtin_amdgcn_readlane(b_tot[nb], L);
        }
    }
    best_out = gbest;
    besti_out = gi;
    return 0;
}

// true when the bit-vector kernel can take a pair with this max_dst (else: row sweep)
// window of the certifying ("full band") sweep
__device__ __host__ inline int bv_full_wl(int md) { return md / 2 + 1 < md ? md / 2 + 1 : md; }
__device__ __host__ inline bool bitvec_supports(int max_dst) { return bv_nb_for_span(bv_full_wl(max_dst) + max_dst) != 0; }
// first-pass window for a given max_dst: w columns right of the diagonal, wl left of it
__device__ __host__ inline int bv_first_w(int md) {
    const int w = (md / 2 > (int)((long long)md * PBA_BV_BAND_NUM / PBA_BV_BAND_DEN)
                       ? md / 2 : (int)((long long)md * PBA_BV_BAND_NUM / PBA_BV_BAND_DEN)) + 1;
    return w > md ? md : w;
}
__device__ __host__ inline int bv_first_wl(int md) {
    const int wl = bv_first_w(md) / 2 + 1;
    return wl > md ? md : wl;
}
// The first-pass window of a launch whose lanes hold NB blocks: with NB fixed the number of steps does not depend on the
// window (lanes that would idle fill up), so it is as wide as the ring lets it be -- the whole band for short pairs,
// 18 % instead of 16.9 % divergence certified at 15 kb -- at no cost.
__device__ __host__ inline int bv_pass1_w(int md, int nb) {
    int w = bv_first_w(md);
    const int room = (bv_max_span(nb) - 4) * 2 / 3;      // w + (w/2 + 1) <= span
    if (room > w) w = room;
    return w > md ? md : w;
}
__device__ __host__ inline int bv_pass1_wl(int md, int nb) {
    const int wl = bv_pass1_w(md, nb) / 2 + 1;
    return wl > md ? md : wl;
}
// the verdicts of a sweep over [i - wl, i + w] (header comment): a failure at row fr / a goal minimum `best`
__device__ __forceinline__ bool bv_fail_certified(int fr, double R, int wl, int md) {
    return 2 * wl + 2 > md || (double)fr * R < (double)(2 * wl + 2);      // floor(i*R) <= md - 1 for every row
}
__device__ __forceinline__ bool bv_goal_certified(int best, int wl, int w, int md) {
    return (w >= md && 2 * wl + 1 >= md) || (best <= w && best <= 2 * wl + 1);   // a passing pair has best <= md - 1
}

#define PBA_RC_UNCERTIFIED (-3)   // narrow pass could not certify the goal row: re-run with full_band

// One pair.  NB is chosen by the host from the largest max_dst in the launch (any NB >= the pair's own
// need is valid).  full_band = false runs the narrow first pass and reports PBA_RC_UNCERTIFIED when the
// goal row cannot be certified; the host then re-launches those pairs with full_band = true.
// There is deliberately no device function call in here: everything inlines into the kernel.
// lds: PBA_BV_LDS_BYTES(NB) of this wavefront's own: the fin words (>= 256 bytes: the m <= 10 corner runs the row sweep in
// them), then the text ring; in rings 1 and 2 the match-mask table, the ring and the fin superblock word (eq_table.h: the
// corner's row then lies in the table, which every sweep fills for itself)
// need_diag: the caller reports D(m,m) (locator.cpp:86): a narrow pass whose window cannot vouch for that cell too
// answers PBA_RC_UNCERTIFIED; without it o.diag is -1 in that case.
// BAIL: give a narrow first pass up early when the pair is heading for a cost its window cannot certify (bitvec_pass:
// bail_w).  For callers whose true pairs are expected beyond the first-pass window (the all-vs-all walk: two noisy reads);
// compiled out elsewhere -- the test costs the step loop three scalar registers, 6 % of k_locate's time at 8 waves per SIMD.
// The score-only sweeps of the aligning kernels (k_align_pairs, k_locate, k_spaced_round) take their text from the ring.  The
// BAIL form does not: the all-vs-all walk lives on ramps, where a stretch is one step and a chunk's write is paid for a few
// steps.  -DPBA_BV_RING=0 builds every form with the register planes (tools/build_variant.py: the parent's step).
#ifndef PBA_BV_RING
#define PBA_BV_RING 1
#endif
template <int NB, bool BAIL = false>
__device__ __forceinline__ void align_bitvec(const PackedFetch &fa, int la, const PackedFetch &fb, int lb, double R,
                                             int maxn, int maxm, bool full_band, uint16_t *lds, int lds_cells,
                                             AlnOut &o, bool need_diag = false) {
    aln_params(la, lb, R, o);
    const int len_a = o.len_a, len_b = o.len_b, md = o.max_dst;
    if (maxn > 0 && (len_a >= maxn + maxm || md >= maxm)) return;      // seq_aligner.h:104-107
    const bool a_rows = len_a > len_b;          // the DP is symmetric under transposition: rows = the LONGER side
    const int m = a_rows ? len_b : len_a, n = a_rows ? len_a : len_b;
    if (m <= 10) {                              // no diagonal check ever fires: plain DP on a <= 23-cell band
        align_rowsweep(fa, la, fb, lb, R, maxn, maxm, lds, lds_cells, o);
        return;
    }
    // w: towards the free end (below the diagonal now that the longer side runs down the rows), wl: the other side
    const int w = full_band ? md : bv_pass1_w(md, NB), wl = full_band ? bv_full_wl(md) : bv_pass1_wl(md, NB);
    if (wl + w > bv_max_span(NB)) { o.rc = -2; return; }   // host sizes NB for the launch: cannot happen
    const PackedFetch rowsF = a_rows ? fa : fb, colsF = a_rows ? fb : fa;
    int best = 0, besti = 0, diag = 0;
    // A narrow window certifies a goal minimum <= w only: a pair whose diagonal is heading past that (two noisy reads of an
    // all-vs-all run differ by ~28 %, against a window sized for a read against its genome) is given up after ~1000 rows
    // instead of being swept to the end for an answer nobody can use.
    const int bail_w = (BAIL && !full_band && w < md) ? w : 0;
    const int fr = bitvec_pass<NB, 0, BAIL, PBA_BV_RING && !BAIL>(rowsF, min(n, m + w), colsF, m, w, wl, R, best, besti, diag, (uint32_t *)lds, nullptr, false, bail_w);
    if (fr) {
        bool gave_up = false;
        if constexpr (BAIL) gave_up = fr == PBA_BV_BAIL;
        if (!gave_up && bv_fail_certified(fr, R, wl, md)) o.fail_row = fr; else o.rc = PBA_RC_UNCERTIFIED;
        return;
    }
    if (!bv_goal_certified(best, wl, w, md)) { o.rc = PBA_RC_UNCERTIFIED; return; }   // header comment
    // D(m,m) is a cell like the goal cells: exact when it is small enough for its path to lie inside the windows
    const bool diag_ok = bv_goal_certified(diag, wl, w, md);
    if (need_diag && !diag_ok) { o.rc = PBA_RC_UNCERTIFIED; return; }
    o.cost = best;
    o.diag = diag_ok ? diag : -1;
    o.matlen_a = a_rows ? besti : m;
    o.matlen_b = a_rows ? m : besti;
    o.rc = ((double)o.matlen_b < (double)len_b * (1.0 - R)) ? -1 : o.matlen_b;   // seq_aligner.h:114
}

#endif
