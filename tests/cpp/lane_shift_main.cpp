// lane_shift_main.cpp -- csrc/lane_shift.h (with eq_table.h and text_ring.h under it) alone, as a host program
// (tests/test_lane_shift_cpu.py builds it, with the sanitizers where the compiler has them).  Every line of stdin is one
// sweep: m nr wleft w NB (bitvec_pass's arguments, as in eq_table_main.cpp).  The program plays the sweep's schedule step by
// step and, side by side, the two lane-to-lane hand-offs of the horizontal deltas over it:
//   RING   superblock s in lane s & 63, the carries masked with `live` where they are handed out and rotated one lane up
//          with wrap -- exactly as the comment above `live` in bitvec_pass derives it (hp_last / hn_last, the re-forming at
//          the close included);
//   SHIFT  lane k holds superblock s_cl + k (lane_shift.h): no mask, a shift with the border entering lane 0, and at a close
//          every lane takes the state of the lane below it; the step behind a close takes the carries unshifted.
// What a superblock hands out at a step is a pseudo-random pair of bits of (superblock, step), so a lane that takes the
// wrong neighbour's, the wrong step's or the border for a cell is seen at once.  The LDS of the shifted form is an exact-size
// heap array of tags, as in eq_table_main.cpp: an address outside it is the sanitizer's to report.
// It exits non-zero at the first of:
//   3  RING: an open superblock takes something else than hout(s - 1, t - 1) or the border (the model is wrong, not the form)
//   4  SHIFT: the same
//   5  an address outside its region, a cell that is no letter's offset, a lane select outside 0 .. 63
//   6  lane <-> superblock <-> column is no bijection, a superblock's column is not s & 63, or two lanes hit one bank
//   7  a column receives fin words (or rows) while a lane with an open window still reads its rows there
//   8  at the end: a fin superblock word that is not its column's last superblock, fin words that are not that superblock's
//   9  an open lane reads a row that is not (its superblock, its column's letter, the block), or a stale ring cell
// and prints per sweep: steps, checked hand-offs (one per open lane and step), closes, fin writes.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "lane_shift.h"

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }
static int letter_of(int e) { return (int)(((unsigned)e * 2654435761u) >> 13) & 3; }
static unsigned mix(int s, int t) { return ((unsigned)s * 73856093u ^ (unsigned)t * 19349663u) * 2654435761u; }
static uint64_t out_p(int s, int t) { return (mix(s, t) >> 17) & 1u; }
static uint64_t out_n(int s, int t) { return (mix(s, t) >> 23) & 1u; }

enum { STALE = -1, FIN = 1 << 28 };
static int row_tag(int s, int letter, int b) { return (s * 4 + letter) * 2 + b; }

int main() {
    int m, nr, wleft, w, NB;
    while (scanf("%d %d %d %d %d", &m, &nr, &wleft, &w, &NB) == 5) {
        if (NB < 1 || NB > 2) return 2;
        const int RB = 32 * NB, S = (nr + RB - 1) / RB, t_end = m + S - 1, s_m = (m - 1) / RB, t1 = m + s_m;
        std::vector<int> lo(S + 130), hi(S + 130);
        for (int s = 0; s < S + 130; ++s) { lo[s] = imax(1, s * RB + 1 - wleft); hi[s] = imin(m, s * RB + RB + w); }
        auto open_at = [&](int s, int t) { return s >= 0 && s < S && t - s >= lo[s] && t - s <= hi[s]; };
        const int TW = eqt_table_words(NB), RW = eqt_ring_word(NB), SW = eqt_sb_word(NB), LW = eqt_lds_words(NB);
        std::vector<int> lds(LW, STALE), ring_elem(PBA_TXR_SLOTS, INT_MIN);
        std::vector<char> col_fin(64, 0);
        long long checked = 0;
        int closes = 0, fins = 0;
        auto fill = [&](int col, int s) -> int {
            if (col_fin[col]) return 7;
            for (int l = 0; l < PBA_EQT_LETTERS; ++l)
                for (int b = 0; b < NB; ++b) {
                    const int wd = eqt_row_word(l, b, NB, col);
                    if (wd < 0 || wd >= TW) return 5;
                    lds[wd] = row_tag(s, l, b);
                }
            return 0;
        };
        auto fin_write = [&](int col, int s) -> int {
            if (s + 64 < S || (s & 63) != col) return s + 64 < S ? 7 : 6;
            for (int k = 0; k < 2 * NB; ++k) {
                const int wd = eqt_fin_word(k, col);
                if (wd < 0 || wd >= TW) return 5;
                lds[wd] = FIN + s;
            }
            lds[SW + col] = s;
            col_fin[col] = 1;
            ++fins;
            return 0;
        };
        for (int c = 0; c < PBA_TXR_SLOTS; ++c) lds[RW + c] = eqt_cell(0, NB);
        for (int l = 0; l < 64; ++l) { lds[SW + l] = -1; if (l < S) { const int rc = fill(l, l); if (rc) return rc; } }
        // the schedule, as bitvec_pass keeps it
        int T_open = 1, s_op = 0, T_close = imin(m, RB + w) + 1, s_cl = 0, T_seg = imin(32, m) + 1, s_sg = 0;
        // RING
        int sbR[64];
        for (int l = 0; l < 64; ++l) sbR[l] = l;
        uint64_t live = (S >= 64 ? ~0ull : (1ull << S) - 1ull) >> 1, hpmR = ~0ull, hnmR = 0ull, hp_last = ~0ull, hn_last = 0ull;
        // SHIFT: the border is what the very first step takes everywhere (no lane's window but superblock 0's is open)
        uint64_t hpmS = ~0ull, hnmS = 0ull;
        bool after_close = false;
        int addr[64];
        for (int l = 0; l < 64; ++l) addr[l] = 0;
        auto lane_ok = [&](int L) { return L >= 0 && L < PBA_LSH_LANES; };
        for (int t = 1; t <= t_end; ++t) {
            if (((t - 1) & (PBA_TXR_CHUNK - 1)) == 0) {         // the chunk's write and every lane's address, with s_cl as it is
                const int first = txr_fetch_first(t, s_cl);
                for (int i = 0; i < PBA_TXR_CHUNK; ++i) {
                    const int slot = txr_slot(first + i), mir = txr_mirror(slot);
                    if (slot < 0 || slot >= PBA_TXR_COLS || mir >= PBA_TXR_SLOTS) return 5;
                    const int cell = eqt_cell(letter_of(first + i), NB);
                    lds[RW + slot] = cell; ring_elem[slot] = first + i;
                    if (mir >= 0) { lds[RW + mir] = cell; ring_elem[mir] = first + i; }
                }
                for (int l = 0; l < 64; ++l) addr[l] = lsh_ring_addr(t, l, s_cl);
            }
            // events, in the handler's order: segment end, close, open
            if (t <= t1 && t == T_seg) {
                const int s = s_sg, i = t - 1 - s;
                const bool leaves = i - 1 - s * RB == RB - 1 && i != m;
                if (!lane_ok(lsh_lane(s, s_cl)) || lsh_sb(lsh_lane(s, s_cl), s_cl) != s) return 5;
                if (leaves && !lane_ok(lsh_lane(s + 1, s_cl))) return 5;
                if (i == m) T_seg = INT_MAX;
                else { s_sg = s + (i == s * RB + RB ? 1 : 0); T_seg = imin(i + 32, m) + s_sg + 1; }
            }
            if (t == T_close) {
                const int s = s_cl;
                // RING
                if (sbR[s & 63] != s) return 3;
                sbR[s & 63] = s + 64;
                if (s + 64 < S) { live |= 1ull << ((s - 1) & 63); hpmR = hp_last | ~live; hnmR = hn_last & live; }
                live &= ~(1ull << (s & 63));
                // SHIFT: lane 0's last column, the lanes' move, the last lane's next superblock
                if (lsh_col(0, s_cl) != (s & 63)) return 6;
                if (s >= s_m) { const int rc = fin_write(lsh_col(0, s_cl), s); if (rc) return rc; }
                for (int l = 0; l < 64; ++l) if (lsh_src_lane(l) != ((l + 1) & 63)) return 6;
                if (lsh_col(63, s_cl + 1) != (s & 63)) return 6;
                if (s + 64 < S) { const int rc = fill(lsh_col(63, s_cl + 1), s + 64); if (rc) return rc; }
                for (int l = 0; l < 64; ++l) addr[l] = lsh_ring_addr(t, l, s_cl + 1);
                after_close = true;
                ++closes;
                s_cl = s + 1;
                T_close = s_cl < S ? imin(m, s_cl * RB + RB + w) + s_cl + 1 : INT_MAX;
            }
            if (t == T_open) {
                if (!lane_ok(lsh_lane(s_op, s_cl)) || sbR[s_op & 63] != s_op) return 5;
                s_op += 1;
                T_open = s_op < S ? imax(1, s_op * RB + 1 - wleft) + s_op : INT_MAX;
            }
            // lane <-> superblock <-> column, and the banks
            {
                uint64_t cols = 0, sbs = 0;
                for (int l = 0; l < 64; ++l) {
                    const int s = lsh_sb(l, s_cl), c = lsh_col(l, s_cl);
                    if (c < 0 || c > 63 || c != (s & 63) || lsh_lane(s, s_cl) != l || sbR[c] != s) return 6;
                    cols |= 1ull << c; sbs |= 1ull << (s - s_cl);
                }
                if (cols != ~0ull || sbs != ~0ull) return 6;
            }
            // the step: what every lane takes
            const uint64_t hpR = (hpmR << 1) | (hpmR >> 63), hnR = (hnmR << 1) | (hnmR >> 63);
            const uint64_t hpS = after_close ? lsh_hin_plus_closed(hpmS) : lsh_hin_plus(hpmS);
            const uint64_t hnS = after_close ? lsh_hin_minus_closed(hnmS) : lsh_hin_minus(hnmS);
            after_close = false;
            for (int b = 0; b < NB; ++b) {
                uint64_t banks = 0;
                for (int l = 0; l < 64; ++l) {
                    if (addr[l] < 0 || addr[l] >= PBA_TXR_SLOTS) return 5;
                    const int cell = lds[RW + addr[l]];
                    bool letter = false;
                    for (int q = 0; q < PBA_EQT_LETTERS; ++q) letter = letter || cell == eqt_cell(q, NB);
                    if (!letter) return 5;
                    const int wd = lsh_read_word(cell, b, l, s_cl), s = lsh_sb(l, s_cl), j = t - s;
                    if (wd < 0 || wd >= TW) return 5;
                    banks |= 1ull << (wd & 63);
                    if (open_at(s, t)) {
                        if (lds[wd] >= FIN) return 7;
                        if (ring_elem[addr[l]] != j - 1 || lds[wd] != row_tag(s, letter_of(j - 1), b)) return 9;
                    }
                }
                if (banks != ~0ull) return 6;
            }
            for (int s = s_cl; s < imin(S, s_cl + 64); ++s) {
                if (!open_at(s, t)) continue;
                // the cell above the superblock's first row in column t - s: superblock s - 1 had it in the step before, if its window reaches that far
                const bool cell_above = s >= 1 && t - 1 - (s - 1) <= hi[s - 1];
                const uint64_t ep = cell_above ? out_p(s - 1, t - 1) : 1u, en = cell_above ? out_n(s - 1, t - 1) : 0u;
                if (cell_above && !open_at(s - 1, t - 1)) return 3;
                if (((hpR >> (s & 63)) & 1u) != ep || ((hnR >> (s & 63)) & 1u) != en) return 3;
                const int L = lsh_lane(s, s_cl);
                if (((hpS >> L) & 1u) != ep || ((hnS >> L) & 1u) != en) return 4;
                ++checked;
            }
            // ... and hands out
            hp_last = 0; hn_last = 0; hpmS = 0; hnmS = 0;
            for (int l = 0; l < 64; ++l) {
                hp_last |= out_p(sbR[l], t) << l; hn_last |= out_n(sbR[l], t) << l;
                hpmS |= out_p(lsh_sb(l, s_cl), t) << l; hnmS |= out_n(lsh_sb(l, s_cl), t) << l;
                addr[l] += 1;
            }
            hpmR = hp_last | ~live; hnmR = hn_last & live;
        }
        // behind the last step: the lanes whose window is still open put their column aside, each into its superblock's column
        for (int l = 0; l < 64; ++l) {
            const int s = lsh_sb(l, s_cl);
            if (s < s_op && s >= s_m && s < S) { const int rc = fin_write(lsh_col(l, s_cl), s); if (rc) return rc; }
        }
        for (int c = 0; c < 64; ++c) {
            const int fs = lds[SW + c];
            if (fs == -1) continue;
            if (fs < s_m || fs >= S || (fs & 63) != c) return 8;
            for (int k = 0; k < 2 * NB; ++k) if (lds[eqt_fin_word(k, c)] != FIN + fs) return 8;
        }
        for (int s = s_m; s < S; ++s) if (lds[SW + (s & 63)] != s) return 8;
        printf("%d %lld %d %d\n", t_end, checked, closes, fins);
    }
    return 0;
}
