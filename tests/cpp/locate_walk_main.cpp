// locate_walk_main.cpp -- csrc/locate_walk.h alone, as a host program (tests/test_locate_walk_cpu.py builds it, with the
// sanitizers where the compiler has them).  Every line of stdin is a lane block: its 64 hit counts, the number of list slots
// asked about, and those slots.  Per block it prints the offsets of lw_offsets with the list's length, the offsets of lw_offset
// (l = 0 .. 64), probe and hit-within-probe of every slot asked about, and lw_hits_upto of every probe under the mask of the
// counts that are not 0.  The arrays are exact-size heap arrays: a read past probe 63 is the sanitizer's to report.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "locate_walk.h"

int main() {
    for (;;) {
        std::vector<uint32_t> cnt(PBA_LW_PROBES);
        for (uint32_t &c : cnt)
            if (scanf("%" SCNu32, &c) != 1) return 0;
        size_t nq;
        if (scanf("%zu", &nq) != 1) return 2;
        std::vector<uint64_t> q(nq), off(PBA_LW_PROBES);
        for (uint64_t &s : q)
            if (scanf("%" SCNu64, &s) != 1) return 2;
        const uint64_t total = lw_offsets(cnt.data(), off.data());
        printf("off");
        for (uint64_t v : off) printf(" %" PRIu64, v);
        printf(" %" PRIu64 "\noff1", total);
        for (int l = 0; l <= PBA_LW_PROBES; ++l) printf(" %" PRIu64, lw_offset(cnt.data(), l));
        printf("\nslots");
        for (uint64_t s : q) {
            if (s >= total) return 3;                       // (the kernel never asks: a lane past the list is idle)
            const int p = lw_slot_probe(off.data(), s);
            printf(" %d:%" PRIu64, p, s - off[p]);
        }
        uint64_t hitmask = 0;
        for (int p = 0; p < PBA_LW_PROBES; ++p)
            if (cnt[p]) hitmask |= 1ull << p;
        printf("\nupto");
        for (int p = 0; p < PBA_LW_PROBES; ++p) printf(" %d", lw_hits_upto(hitmask, p));
        printf("\n");
    }
}
