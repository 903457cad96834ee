// align_windows.h -- per-window alignment counts straight from the traceback walk (align_bvtrace.h): a fourth sink beside
// OpSink (bytes), VoteSink (votes) and CigarSink (runs); the op queue is GroupQueue's, the classes of the ops OpClasses'.  The a sequence carries a fixed grid of W-base windows on its own
// coordinates; every op of the path is counted (=, X, I, D: align_cigar.h's codes) in the window of the a-element it belongs
// to, and one pba_aln_counts per window goes to memory.  No script and no run exists anywhere.
//
// a-element e lies at x(e) = a_pos + e (forward accessor) or a_pos - e (backward); g(e) = x(e) / W, and the pair's local
// window index is w(e) = |g(e) - g(0)|: monotone in e either way.
//   MATCH  at (i, j): a-element i-1               -> window w(i-1)
//   DELETE at (i, j): a-element i-1               -> window w(i-1)
//   INSERT at (i, j): no a-element; the one before -> window w(max(i-1, 0))
// The walk meets the ops goal-first, so window indices never grow along it: the boundaries inside a group of 64 ops are a
// ballot of "differs from the lane before", a window's four counts are popcounts of the code ballots under its segment's
// mask, and the window that is still open is carried wave-uniform from group to group.  The first op the walk puts sits at
// the goal cell, so n_win = w(max(matlen_a - 1, 0)) + 1 is known before any window closes and a closed window goes to its
// final place at once: slot w, or n_win - 1 - w when the windows are wanted goal-first.
#ifndef PBA_ALIGN_WINDOWS_H
#define PBA_ALIGN_WINDOWS_H

#include "align_cigar.h"

struct WindowSink : GroupQueue<WindowSink> {
    OpClasses cls;
    pba_aln_counts *out;        // this pair's slot
    int cap;                    // windows the slot holds (n_win is an int: a larger slot counts as INT_MAX): with fewer than n_win nothing is written
    int a_pos, a_step, W, g0;   // x(e) = a_pos + a_step * e;  g0 = g(0)
    bool reversed;
    // wave-uniform: the windows of the pair (-1 before the first op), the open window and its counts
    int n_win, cur_w;
    int o_eq, o_x, o_ins, o_del;

    __device__ __forceinline__ void init(const PackedFetch &a, const PackedFetch &b, int pos, bool a_backward, int w, pba_aln_counts *slot,
                                         uint64_t slot_cap, bool swap, bool rev) {
        cls.init(a, b, swap); out = slot; cap = (int)min(slot_cap, (uint64_t)INT_MAX); a_pos = pos; a_step = a_backward ? -1 : 1; W = w; g0 = pos / w;
        reversed = rev;
        reset(); n_win = -1; cur_w = -1;
        o_eq = 0; o_x = 0; o_ins = 0; o_del = 0;
    }
    __device__ __forceinline__ int window_of(int e) const {
        const int g = (a_pos + a_step * e) / W - g0;
        return g < 0 ? -g : g;
    }
    // one window to its final place: a 16-byte vector store by the calling lane; never outside the slot
    __device__ __forceinline__ void store(int w, int eq, int x, int ins, int del) const {
        if (w < 0 || w >= n_win || n_win > cap) return;
        *(int4 *)(out + (reversed ? n_win - 1 - w : w)) = make_int4(eq, x, ins, del);
    }
    // lanes 0 .. cnt-1 hold an op each: classify, find the window boundaries, write the windows that close, keep the last open
    __device__ __forceinline__ void flush(int cnt) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        const int w = lane < cnt ? window_of(max(p_i - 1, 0)) : 0;             // (MATCH and DELETE sit at i >= 1)
        OpBallots ob;
        cls.classify(p_op, p_i, p_j, cnt, ob);
        const uint64_t E = ob.E, X = ob.X, I = ob.I, D = ob.D;
        const int w0 = __builtin_amdgcn_readfirstlane(w);
        if (n_win < 0) n_win = w0 + 1;                                          // the first op sits at the goal cell
        if (cur_w >= 0 && cur_w != w0) {                                        // the carried window closed at the group's edge
            if (lane == PBA_WAVE - 1) store(cur_w, o_eq, o_x, o_ins, o_del);
            o_eq = 0; o_x = 0; o_ins = 0; o_del = 0;
        }
        const int up = __shfl_up(w, 1, PBA_WAVE);
        const uint64_t B = __builtin_amdgcn_ballot_w64(lane >= 1 && lane < cnt && w != up);
        if (B == 0ull) {                                                        // the whole group lies in the open window
            o_eq += __builtin_popcountll(E); o_x += __builtin_popcountll(X); o_ins += __builtin_popcountll(I); o_del += __builtin_popcountll(D);
            cur_w = w0;
            return;
        }
        const int first = (int)__builtin_ctzll(B), last = 63 - (int)__builtin_clzll(B);
        if (lane == 0) {                                                        // the open window closes at the first boundary
            const uint64_t m = (1ull << first) - 1ull;
            store(w0, o_eq + __builtin_popcountll(E & m), o_x + __builtin_popcountll(X & m), o_ins + __builtin_popcountll(I & m),
                  o_del + __builtin_popcountll(D & m));
        } else if ((B >> lane) & 1ull) {
            const uint64_t above = lane == PBA_WAVE - 1 ? 0ull : B >> (lane + 1);
            if (above) {                                                        // opened and closed inside this group
                const int end = lane + 1 + (int)__builtin_ctzll(above);        // the next boundary: <= 63
                const uint64_t m = ((1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
                store(w, __builtin_popcountll(E & m), __builtin_popcountll(X & m), __builtin_popcountll(I & m), __builtin_popcountll(D & m));
            }
        }
        const uint64_t m = ~((1ull << last) - 1ull);                            // (lanes beyond cnt hold code 0: in no ballot)
        o_eq = __builtin_popcountll(E & m); o_x = __builtin_popcountll(X & m); o_ins = __builtin_popcountll(I & m); o_del = __builtin_popcountll(D & m);
        cur_w = __builtin_amdgcn_readlane(w, last);
    }
    // Closes the open window; returns n_win (a path without ops: one empty window).  Lane 0 writes the counts.
    __device__ __forceinline__ int finish(pba_aln_counts *counts) {
        const int lane = threadIdx.x & (PBA_WAVE - 1);
        flush_tail();
        if (n_win < 0) { n_win = 1; cur_w = 0; }
        if (lane == 0) {
            store(cur_w, o_eq, o_x, o_ins, o_del);
            cls.store(counts);
        }
        return n_win;
    }
};

// per-window counts: pair q's windows to its slot, their number to n[q], their sum to counts[q].  No temporary: a closed window
// goes straight to its final place.
struct WindowJob {
    using Sink = WindowSink;
    SlotsInto s;
    __device__ __forceinline__ void open(WindowSink &k, uint32_t q, const pba_pair &pr, const PackedFetch &fa, const PackedFetch &fb,
                                         const SeqSetDev &, uint32_t *, uint64_t) const {
        const uint32_t fl = s.flags_of(q);
        const uint64_t o0 = s.off[q], o1 = s.off[q + 1];
        k.init(fa, fb, pr.a_pos, (pr.flags & PBA_A_BACKWARD) != 0, s.W, (pba_aln_counts *)s.slot + o0, o1 - o0,
               (fl & PBA_CIG_B_IS_QUERY) != 0, (fl & PBA_CIG_REVERSED) != 0);
    }
    __device__ __forceinline__ int overlap_min() const { return 0; }
    __device__ __forceinline__ void close(WindowSink &k, uint32_t q, bool walked) const {
        s.close(q, walked, walked ? k.finish(s.counts + q) : 0);
    }
};

#endif
