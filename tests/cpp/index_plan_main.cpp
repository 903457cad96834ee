// index_plan_main.cpp -- csrc/index_plan.h alone, as a host program (tests/test_index_plan_cpu.py builds it, with the
// sanitizers where the compiler has them and seed_index.h's regime constants as -D).  Every argument is "v:LEN:MODE" or
// "p:N_UPPER"; per argument it prints one line:
//   visit LEN MODE visited nhead tail_top bad nseg {lo hi ord0 descending}   bad: ordinals of the segments that ix_ord_pos does not
//                                                                          map back to their position
//   plan N logP n_levels P ov_cap list_off stat ov offs_words cursor tile_pre scan work_words {bits done lvl_off} per level
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "index_plan.h"

static void visit_line(uint32_t len, int mode) {
    const VisitPlan v = visit_plan(len, mode);
    uint64_t bad = 0;
    for (int s = 0; s < v.nseg; ++s)
        for (uint32_t pos = v.segs[s].lo; pos < v.segs[s].hi; ++pos) {
            const uint32_t ord = v.segs[s].ord0 + (v.segs[s].descending ? v.segs[s].hi - 1 - pos : pos - v.segs[s].lo);
            bad += ix_ord_pos(v.nhead, v.tail_top, ord) != (int32_t)pos;
        }
    printf("visit %u %d %u %u %d %" PRIu64 " %d", len, mode, v.visited, v.nhead, v.tail_top, bad, v.nseg);
    for (int s = 0; s < v.nseg; ++s) printf(" %u %u %u %d", v.segs[s].lo, v.segs[s].hi, v.segs[s].ord0, v.segs[s].descending);
    printf("\n");
}

static void plan_line(uint64_t n) {
    const IndexPlan p = index_plan(n);
    printf("plan %" PRIu64 " %d %d %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64,
           n, p.logP, p.n_levels, p.P, p.ov_cap, p.list_off, p.stat, p.ov, p.offs_words, p.cursor, p.tile_pre, p.scan, p.work_words);
    for (int k = 0; k < p.n_levels; ++k) printf(" %d %d %" PRIu64, p.bits[k], p.done[k], p.lvl_off[k]);
    printf("\n");
}

int main(int argc, char **argv) {
    printf("consts %d %d %d\n", PBA_IX_MAX_LOGP, PBA_IX_LVL_BITS, PBA_IX_PART_AVG);
    for (int i = 1; i < argc; ++i) {
        unsigned long long a = 0;
        int mode = 0;
        if (sscanf(argv[i], "v:%llu:%d", &a, &mode) == 2) visit_line((uint32_t)a, mode);
        else if (sscanf(argv[i], "p:%llu", &a) == 1) plan_line(a);
        else return 2;
    }
    return 0;
}
