// eq_table_main.cpp -- csrc/eq_table.h (with csrc/text_ring.h under it) alone, as a host program (tests/test_eq_table_cpu.py
// builds it, with the sanitizers where the compiler has them).  Every line of stdin is one sweep: m nr wleft w NB
// (bitvec_pass's arguments, as in text_ring_main.cpp).  The program plays the sweep step by step the way the kernel uses the
// two headers -- every ring cell set to letter 0 and the first 64 superblocks' rows filled in front of the sweep, a chunk's
// 32 cells written in front of every 32 steps, at a close the fin words (superblock >= s_m) and the next superblock's rows
// (s + 64 < S), every lane reading its cell and then one table word per block at every step -- against a model that knows
// nothing of the layout: superblock s works on column t - s at step t while its window is open, in lane s mod 64, and needs
// the match masks of ITS rows for the letter of THAT column.  The wavefront's LDS is an exact-size heap array of tags: an
// address outside it is the sanitizer's to report.  The text is pseudo-random letters; outside [0, m) it is whatever the
// slack holds, any letter.
// It exits non-zero at the first of:
//   3  a lane with an open window reads a word that is not (its superblock, its column's letter, the block)
//   5  a cell that is no letter's offset, a read outside the table, a write outside its part of the layout
//   7  a fin word written over rows that a lane with an open window still reads, or by a lane that takes another superblock
//   8  at the end: a superblock word that is not "none" or its lane's last superblock; fin words that are not that superblock's
// and prints per sweep: steps, checked reads (one per open lane and step), row fills, fin writes.
#include <climits>
#include <cstdio>
#include <vector>

#include "eq_table.h"

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }
static int letter_of(int e) { return (int)(((unsigned)e * 2654435761u) >> 13) & 3; }

enum { STALE = -1, FIN = 1 << 28 };                            // tags of a table word; a row is (s * 4 + letter) * 2 + block
static int row_tag(int s, int letter, int b) { return (s * 4 + letter) * 2 + b; }

int main() {
    int m, nr, wleft, w, NB;
    while (scanf("%d %d %d %d %d", &m, &nr, &wleft, &w, &NB) == 5) {
        if (NB < 1 || NB > 2) return 2;
        const int RB = 32 * NB, S = (nr + RB - 1) / RB, t_end = m + S - 1, s_m = (m - 1) / RB;
        std::vector<int> lo(S), hi(S);
        for (int s = 0; s < S; ++s) { lo[s] = imax(1, s * RB + 1 - wleft); hi[s] = imin(m, s * RB + RB + w); }
        const int TW = eqt_table_words(NB), RW = eqt_ring_word(NB), SW = eqt_sb_word(NB), LW = eqt_lds_words(NB);
        if (RW != TW || SW != RW + PBA_TXR_SLOTS || LW != SW + 64) return 5;
        std::vector<int> lds(LW, STALE);                      // table: tags; ring: cell values; sb: superblock numbers
        std::vector<int> ring_elem(PBA_TXR_SLOTS, INT_MIN);
        std::vector<int> last_read(64, 0);                    // last step at which the lane reads with an open window
        for (int s = 0; s < S; ++s) if (lo[s] <= hi[s]) last_read[s & 63] = imax(last_read[s & 63], hi[s] + s);
        long long reads = 0;
        int fills = 0, fins = 0;
        auto fill = [&](int lane, int s) -> bool {
            for (int l = 0; l < PBA_EQT_LETTERS; ++l)
                for (int b = 0; b < NB; ++b) {
                    const int wd = eqt_row_word(l, b, NB, lane);
                    if (wd < 0 || wd >= TW) return false;
                    lds[wd] = row_tag(s, l, b);
                }
            ++fills;
            return true;
        };
        auto fin_write = [&](int lane, int s, int t) -> int {   // t: the first step that runs after the write
            if (s + 64 < S) return 7;                         // the lane would fill its rows again, over the fin words
            if (last_read[lane] >= t) return 7;
            for (int k = 0; k < 2 * NB; ++k) {
                const int wd = eqt_fin_word(k, lane);
                if (wd < 0 || wd >= TW) return 5;
                lds[wd] = FIN + s;
            }
            lds[SW + lane] = s;
            ++fins;
            return 0;
        };
        // in front of the sweep
        for (int c = 0; c < PBA_TXR_SLOTS; ++c) lds[RW + c] = eqt_cell(0, NB);
        for (int l = 0; l < 64; ++l) { lds[SW + l] = -1; if (l < S && !fill(l, l)) return 5; }
        int sb[64], addr[64];
        for (int l = 0; l < 64; ++l) { sb[l] = l; addr[l] = 0; }
        for (int t = 1; t <= t_end; ++t) {
            if (((t - 1) & (PBA_TXR_CHUNK - 1)) == 0) {
                int s_cl = 0;
                while (s_cl < S && hi[s_cl] + s_cl + 1 < t) ++s_cl;
                const int first = txr_fetch_first(t, s_cl);
                for (int i = 0; i < PBA_TXR_CHUNK; ++i) {
                    const int slot = txr_slot(first + i), mir = txr_mirror(slot);
                    if (slot < 0 || slot >= PBA_TXR_COLS || mir >= PBA_TXR_SLOTS) return 5;
                    const int cell = eqt_cell(letter_of(first + i), NB);
                    lds[RW + slot] = cell; ring_elem[slot] = first + i;
                    if (mir >= 0) { lds[RW + mir] = cell; ring_elem[mir] = first + i; }
                }
                for (int l = 0; l < 64; ++l) addr[l] = txr_addr(t, s_cl + ((l - s_cl) & 63));
            }
            for (int s = 0; s < S; ++s)                       // the close event of the superblock whose window ended with the step before
                if (hi[s] + s + 1 == t) {
                    const int lane = s & 63;
                    if (s >= s_m) { const int rc = fin_write(lane, s, t); if (rc) return rc; }
                    sb[lane] = s + 64;
                    if (s + 64 < S && !fill(lane, s + 64)) return 5;
                    addr[lane] = txr_addr(t, s + 64);
                }
            for (int l = 0; l < 64; ++l) {
                if (addr[l] < 0 || addr[l] >= PBA_TXR_SLOTS) return 5;
                const int cell = lds[RW + addr[l]];
                bool letter = false;
                for (int q = 0; q < PBA_EQT_LETTERS; ++q) letter = letter || cell == eqt_cell(q, NB);
                if (!letter) return 5;
                const int s = sb[l], j = t - s;
                const bool open = s < S && j >= lo[s] && j <= hi[s];
                for (int b = 0; b < NB; ++b) {
                    const int wd = eqt_read_word(cell, b, l);
                    if (wd < 0 || wd >= TW || (wd & 63) != l) return 5;
                    if (open) {
                        if (lds[wd] >= FIN) return 7;
                        if (ring_elem[addr[l]] != j - 1 || lds[wd] != row_tag(s, letter_of(j - 1), b)) return 3;
                    }
                }
                if (open) ++reads;
                addr[l] += 1;
            }
        }
        // behind the last step: the lanes whose window is still open and reaches the last column put their words aside
        for (int l = 0; l < 64; ++l) {
            const int s = sb[l];
            if (s >= s_m && s < S && lo[s] + s <= t_end) { const int rc = fin_write(l, s, t_end + 1); if (rc) return rc; }
        }
        for (int l = 0; l < 64; ++l) {
            const int fs = lds[SW + l];
            if (fs == -1) continue;
            if (fs < s_m || fs >= S || (fs & 63) != l) return 8;
            for (int k = 0; k < 2 * NB; ++k) if (lds[eqt_fin_word(k, l)] != FIN + fs) return 8;
        }
        for (int s = s_m; s < S; ++s) if (lds[SW + (s & 63)] != s) return 8;
        printf("%d %lld %d %d\n", t_end, reads, fills, fins);
    }
    return 0;
}
