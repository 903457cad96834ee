// text_ring_main.cpp -- csrc/text_ring.h alone, as a host program (tests/test_text_ring_cpu.py builds it, with the sanitizers
// where the compiler has them).  Every line of stdin is one sweep: m nr wleft w NB (bitvec_pass's arguments: m columns, nr
// rows, row i sees the columns [i - wleft, i + w], NB blocks per lane).  The program plays the sweep step by step the way
// the kernel uses the header -- a write in front of every chunk of 32 steps, a lane's address taken at the chunk's start and
// when the lane takes its next superblock, one byte further every step -- against a model that knows nothing of the ring:
// superblock s works on column t - s at step t while max(1, s RB + 1 - wleft) <= t - s <= min(m, s RB + RB + w), in lane
// s mod 64.  The ring is an exact-size heap array of element numbers: an address outside it is the sanitizer's to report.
// It exits non-zero at the first of:
//   3  a lane with an open window does not find element t - 1 - s at its address
//   4  a write replaces an element that an open window still has to read
//   5  an address (of any lane, open or not) or a written slot outside the ring
//   6  the superblock the kernel derives for a lane (s_cl + ((lane - s_cl) & 63)) is not the one the lane holds
// and prints per sweep: steps, checked reads, the widest span between the oldest element still to be read and the frontier.
#include <climits>
#include <cstdio>
#include <vector>

#include "text_ring.h"

static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

int main() {
    int m, nr, wleft, w, NB;
    while (scanf("%d %d %d %d %d", &m, &nr, &wleft, &w, &NB) == 5) {
        const int RB = 32 * NB, S = (nr + RB - 1) / RB, t_end = m + S - 1;
        // the model: first and last column of every superblock's window; an empty window (lo > hi) never opens
        std::vector<int> lo(S), hi(S);
        for (int s = 0; s < S; ++s) { lo[s] = imax(1, s * RB + 1 - wleft); hi[s] = imin(m, s * RB + RB + w); }
        // last step at which element e (column e + 1) is read by an open window
        std::vector<int> last_use(m, 0);
        for (int s = 0; s < S; ++s)
            for (int j = lo[s]; j <= hi[s]; ++j) last_use[j - 1] = imax(last_use[j - 1], j + s);
        std::vector<int> ring(PBA_TXR_SLOTS, INT_MIN);       // which element a cell holds
        int sb[64], addr[64];
        for (int l = 0; l < 64; ++l) { sb[l] = l; addr[l] = 0; }
        long long reads = 0;
        int span = 0;
        for (int t = 1; t <= t_end; ++t) {
            if (((t - 1) & (PBA_TXR_CHUNK - 1)) == 0) {
                int s_cl = 0;                                 // superblocks closed by the steps before t (step after the window: hi + s + 1)
                while (s_cl < S && hi[s_cl] + s_cl + 1 < t) ++s_cl;
                const int first = txr_fetch_first(t, s_cl);
                for (int i = 0; i < PBA_TXR_CHUNK; ++i) {
                    const int slot = txr_slot(first + i), mir = txr_mirror(slot);
                    if (slot < 0 || slot >= PBA_TXR_COLS || mir >= PBA_TXR_SLOTS) return 5;
                    const int old = ring[slot];
                    if (old != first + i && old >= 0 && old < m && last_use[old] >= t) return 4;
                    ring[slot] = first + i;
                    if (mir >= 0) ring[mir] = first + i;
                }
                for (int e = imax(0, first - 200); e < imin(m, first + PBA_TXR_CHUNK); ++e)
                    if (last_use[e] >= t) { span = imax(span, first + PBA_TXR_CHUNK - e); break; }
                if (txr_oldest_live(t, s_cl) < first + PBA_TXR_CHUNK - PBA_TXR_COLS) return 4;   // the header's own claim
                for (int l = 0; l < 64; ++l) {
                    const int derived = s_cl + ((l - s_cl) & 63);
                    // (a close due at this very step is handled below, as the kernel's events are: after the write)
                    if (derived != sb[l]) return 6;
                    addr[l] = txr_addr(t, derived);
                }
            }
            for (int s = 0; s < S; ++s)                       // the lane of a superblock that closed with the step before moves on
                if (hi[s] + s + 1 == t) { sb[s & 63] = s + 64; addr[s & 63] = txr_addr(t, s + 64); }
            for (int l = 0; l < 64; ++l) {
                if (addr[l] < 0 || addr[l] >= PBA_TXR_SLOTS) return 5;
                const int s = sb[l], j = t - s;
                if (s < S && j >= lo[s] && j <= hi[s]) {
                    if (ring[addr[l]] != txr_elem(t, s) || txr_elem(t, s) != j - 1) return 3;
                    ++reads;
                }
                addr[l] += 1;
            }
        }
        printf("%d %lld %d\n", t_end, reads, span);
    }
    return 0;
}
