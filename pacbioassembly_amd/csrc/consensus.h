// consensus.h -- vote boxes, elect and evolve of the unlocked ref_seq (/root/reference/src/ref_seq.h:25-188,
// 207-242, 317-362) on the device.  SURVEY.md 8f-3.
//
// Layout: like ref_seq::txt_buf the object spans 3*max_len positions with the origin (`beg`) at max_len, and
// the vote box of a text position sits at the same index -- the reference's std::list<vote_box> is positional
// (one box per character of [pre, post)), so append / prepend are range fills and need no shifting.
//   sel[p], sup[p] : 4 x u16 counters (base_vote::acgt, ref_seq.h:49) packed in one u64, A in bits 15:0
//   tot[p]         : vote_box::total
// Votes are commutative, so elect runs one wavefront per edit script with atomics; the counters are bumped with
// 32-bit atomics on the half-word's dword (they wrap like the reference's unsigned short only below 65 536 votes
// per counter: far beyond any coverage this code meets).
// evolve (ref_seq.h:317-349) is a stream compaction: every box yields 0..2 output boxes (itself if its selection
// wins a majority, a box split from its suppliment if that does), a deleted box's selection is absorbed by the
// suppliment of the last box kept before it.  One workgroup sweeps the list in chunks of 1024 with an LDS scan:
// it runs once per assembly round on at most a few million boxes.
#ifndef PBA_CONSENSUS_H
#define PBA_CONSENSUS_H

#include "align_bvtrace.h"
#include "dev_common.h"

struct ConsDev {
    unsigned long long *sel, *sup;   // 4 x u16 each
    int *tot;
    char *txt;
};

// Where a batch of walks votes (VoteJob below, run by k_vote_pairs in pba_align.hip), and a pile-up's arena as its own kernels see it.  One
// reference: boxes C, pair.a_pos counted from box `beg`, live range [pre, post).  box_off non-null: C is a pile-up's arena
// (pba_pileup.hip; txt unused), one segment per pair's own a_seq -- target t owns boxes [box_off[t - t_lo], + len(t)) and
// beg / pre / post are unused.
struct VoteInto {
    ConsDev C;
    int beg, pre, post;
    const unsigned long long *box_off;
    uint32_t t_lo;
};

__device__ __forceinline__ int cons_c2i(int ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : 3; }   // dna_seq.h:21
__device__ __forceinline__ int cons_max4(unsigned long long v) {          // base_vote::max_vote, ref_seq.h:88-91
    const int a = (int)(v & 0xFFFF), b = (int)((v >> 16) & 0xFFFF), c = (int)((v >> 32) & 0xFFFF), d = (int)(v >> 48);
    return max(max(a, b), max(c, d));
}
__device__ __forceinline__ char cons_winner(unsigned long long v) {        // base_vote::winner, ref_seq.h:96-100
    const int mv = cons_max4(v);
    return mv == (int)(v & 0xFFFF) ? 'A' : (mv == (int)((v >> 16) & 0xFFFF) ? 'C' : (mv == (int)((v >> 32) & 0xFFFF) ? 'G' : 'T'));
}
// the sel word of vote_box(base, weight) (ref_seq.h:118: selection(c, n)); sup = 0 and total = 1 go with it
__device__ __forceinline__ unsigned long long cons_vote_box(int code, int weight) {
    return (unsigned long long)(unsigned)(weight & 0xFFFF) << (16 * code);
}
// what a box yields in evolve: bit 0 = its selection is kept, bit 1 = its suppliment splits off
__device__ __forceinline__ int cons_yield(unsigned long long sel, unsigned long long sup, int tot) {
    const bool S = (double)cons_max4(sup) > 0.5 * (double)tot;    // has_supply(0.5), ref_seq.h:327
    const bool V = (double)cons_max4(sel) > 0.5 * (double)tot;    // is_valid(0.5),   ref_seq.h:336
    return (V ? 1 : 0) | (S ? 2 : 0);
}
__device__ __forceinline__ void cons_bump(unsigned long long *box, int c, unsigned n) {   // counter c += n
    atomicAdd((unsigned *)box + (c >> 1), n << (16 * (c & 1)));
}

// boxes [first, first+len) <- vote_box(text[k], weight); text copied too
static __global__ void __launch_bounds__(256)
k_cons_fill(ConsDev C, int first, int len, const char *text, int weight) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= len) return;
    const char ch = text[k];
    C.txt[first + k] = ch;
    C.sel[first + k] = cons_vote_box(cons_c2i(ch), weight);
    C.sup[first + k] = 0ull;
    C.tot[first + k] = 1;
}

// apply_edits (ref_seq.h:25-41) for n scripts, one wavefront each.  pos is relative to `beg`.
static __global__ void __launch_bounds__(PBA_WAVE)
k_cons_elect(ConsDev C, int beg, int pre, int post, uint32_t n, const int *pos, const uint8_t *fwd, const uint8_t *ops,
             const char *vals, const unsigned long long *ops_off, const int *nedit) {
    const uint32_t q = blockIdx.x;
    if (q >= n) return;
    const int lane = threadIdx.x;
    const bool forward = fwd[q] != 0;
    const int it0 = beg + pos[q], ne = nedit[q];
    const uint8_t *o = ops + ops_off[q];
    const char *v = vals + ops_off[q];
    int done = 0;                                   // boxes consumed by the ops of earlier chunks
    for (int k0 = 0; k0 < ne; k0 += PBA_WAVE) {
        const int k = k0 + lane;
        const int op = k < ne ? o[k] : 0;
        const bool adv = op == 1 || op == 3;        // MATCH and DELETE move the iterator
        const unsigned long long m = __builtin_amdgcn_ballot_w64(adv);
        const int before = done + __builtin_popcountll(m & ((1ull << lane) - 1ull));
        int at = forward ? it0 + before : it0 - before;
        if (op == 2 && forward) at -= 1;            // INSERT: `--it; supply; ++it` forward, the box itself backward
        if (op != 0 && at >= pre && at < post) {
            if (op == 1) { cons_bump(C.sel + at, cons_c2i(v[k]), 1u); atomicAdd(C.tot + at, 1); }   // select
            else if (op == 3) atomicAdd(C.tot + at, 1);                                                // ignore
            else cons_bump(C.sup + at, cons_c2i(v[k]), 1u);                                            // supply
        }
        done += __builtin_popcountll(m);
    }
}

// Votes straight from the traceback walk (align_bvtrace.h), no script in memory: a sink that turns the reference's
// op at cell (i, j) into its vote.  The cell says it all: a MATCH / DELETE at (i, j) consumes a-element i-1, i.e. the
// box `it0 +/- (i-1)`; an INSERT at (i, j) comes after i consumed elements, i.e. supplies box `it0 + i - 1` forward
// (`--it; supply; ++it`) or `it0 - i` backward (apply_edits, ref_seq.h:25-41); the value is b-element j-1.
// 64 votes are gathered (one per lane, GroupQueue: align_bvtrace.h) and applied together, each lane working out its own box
// and fetching its own b element.
struct VoteSink : GroupQueue<VoteSink> {
    ConsDev C;
    int it0, pre, post;         // box of the start position; the live range of boxes
    bool fwd;
    PackedFetch fb;             // the segment (b)
    __device__ __forceinline__ void init(const ConsDev &c, int box0, int w_pre, int w_post, bool forward, const PackedFetch &b) {
        C = c; it0 = box0; pre = w_pre; post = w_post; fwd = forward; fb = b;
        reset();
    }
    __device__ __forceinline__ void flush(int cnt) {
        if ((int)(threadIdx.x & (PBA_WAVE - 1)) >= cnt) return;
        const int at = p_op == 2u ? (fwd ? it0 + p_i - 1 : it0 - p_i) : (fwd ? it0 + (p_i - 1) : it0 - (p_i - 1));
        if (at < pre || at >= post) return;
        if (p_op == 3u) atomicAdd(C.tot + at, 1);                                       // ignore
        else {
            const int c = fb(p_j - 1);                                                  // 2-bit code == C2I of the base
            if (p_op == 1u) { cons_bump(C.sel + at, c, 1u); atomicAdd(C.tot + at, 1); }   // select
            else cons_bump(C.sup + at, c, 1u);                                          // supply
        }
    }
    __device__ __forceinline__ void finish() { flush_tail(); }
};

// votes: pair q's path into the boxes V names, gated by overlap_min; a is the reference, pair.a_pos the position the votes
// start at.  SEG: V is a pile-up's arena (VoteInto with box_off), one segment per target read: pair q votes into the window
// of ITS a_seq, the box of a_pos at that segment's offset + a_pos.  The arena holds fewer than 2^31 boxes (the host refuses
// or chunks beyond that), so the window fits VoteSink's ints.  Nothing but the boxes is written.
template <bool SEG>
struct VoteJob {
    using Sink = VoteSink;
    VoteInto V;
    int gate;
    __device__ __forceinline__ void open(VoteSink &s, uint32_t, const pba_pair &pr, const PackedFetch &, const PackedFetch &fb,
                                         const SeqSetDev &A, uint32_t *, uint64_t) const {
        int it0 = V.beg + pr.a_pos, w_pre = V.pre, w_post = V.post;
        if constexpr (SEG) {
            w_pre = (int)V.box_off[pr.a_seq - V.t_lo];
            w_post = w_pre + (int)A.len[pr.a_seq];
            it0 = w_pre + pr.a_pos;
        }
        s.init(V.C, it0, w_pre, w_post, !(pr.flags & PBA_A_BACKWARD), fb);
    }
    __device__ __forceinline__ int overlap_min() const { return gate; }
    __device__ __forceinline__ void close(VoteSink &s, uint32_t, bool walked) const { if (walked) s.finish(); }
};

// evolve: [pre, post) of `in` -> boxes and text from index `beg` of `out`; *n_out = boxes kept
static __global__ void __launch_bounds__(1024)
k_cons_evolve(ConsDev in, ConsDev out, int pre, int post, int beg, int *n_out) {
    __shared__ int scan[1024];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = pre; base < post; base += 1024) {
        const int i = base + tid;
        const bool live = i < post;
        unsigned long long sel = 0, sup = 0;
        int tot = 0;
        if (live) { sel = in.sel[i]; sup = in.sup[i]; tot = in.tot[i]; }
        const int y = cons_yield(sel, sup, tot);                // (0 beyond the list: no count exceeds half of tot = 0)
        const bool S = (y & 2) != 0, V = (y & 1) != 0;
        const int cnt = (V ? 1 : 0) + (S ? 1 : 0);
        scan[tid] = cnt;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {       // inclusive scan (Hillis-Steele; once per round, not hot)
            const int t = tid >= d ? scan[tid - d] : 0;
            __syncthreads();
            scan[tid] += t;
            __syncthreads();
        }
        const int off = beg + carry + scan[tid] - cnt;          // first output slot of this box
        if (V) {                                                // kept; its suppliment moves out if it was split
            out.sel[off] = sel; out.sup[off] = S ? 0ull : sup; out.tot[off] = tot;
            out.txt[off] = cons_winner(sel);
        }
        if (S) {                                                // the split box, inserted right behind (ref_seq.h:328-334)
            out.sel[off + (V ? 1 : 0)] = sup; out.sup[off + (V ? 1 : 0)] = 0ull; out.tot[off + (V ? 1 : 0)] = tot;
            out.txt[off + (V ? 1 : 0)] = cons_winner(sup);
        }
        __threadfence();
        __syncthreads();                                        // every box of this chunk is in place ...
        if (live && !V && off - 1 >= beg) {                     // ... before a deleted one is absorbed by its predecessor
            for (int c = 0; c < 4; ++c) {
                const unsigned add = (unsigned)((sel >> (16 * c)) & 0xFFFF);
                if (add) cons_bump(out.sup + (off - 1), c, add);
            }
        }
        __syncthreads();
        if (tid == 1023) carry += scan[1023];
        __syncthreads();
    }
    if (tid == 0) *n_out = carry;
}

#endif
