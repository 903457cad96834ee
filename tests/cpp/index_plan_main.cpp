// index_plan_main.cpp -- csrc/index_plan.h alone, as a host program (tests/test_index_plan_cpu.py builds it, with the
// sanitizers where the compiler has them and seed_index.h's regime constants as -D).  Per argument it prints:
//   v:LEN:MODE   visit LEN MODE visited nhead tail_top bad nseg {lo hi ord0 descending}   bad: ordinals of the segments that ix_ord_pos
//                does not map back to their position
//   p:N_UPPER    plan N logP n_levels P ov_cap list_off stat ov offs_words cursor tile_pre scan work_words {bits done lvl_off} per level
//   r:LO:HI      one line per length LO .. HI, both modes on it (PBA_INDEX_ALL first):
//                rule LEN { nhead tail_lo tail_top visited head_chunks tail_chunk0 tail_chunks  (visit_rule)
//                           visited nhead tail_top nseg lo hi ord0 descending lo hi ord0 descending  (visit_plan; a segment it has not: zeros) }
//   o:LEN:MODE   ord LEN MODE visited seen bad_inverse bad_cover   over the positions 0 .. LEN + 16: seen = those with ord_of >= 0,
//                bad_inverse = ordinals / positions that pos_of and ord_of do not map onto each other, bad_cover = positions the chunks
//                of the rule's numbering, each cut to its segment, do not cover exactly once if visited and never if not
//   c:MASK       compress MASK tried bad   bad: seeded random x & MASK whose ix_compress(x, compress_masks(MASK)) is not the bit-by-bit gather
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

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

static void rule_lines(uint64_t lo, uint64_t hi) {
    for (uint64_t l = lo; l <= hi; ++l) {
        const uint32_t len = (uint32_t)l;
        printf("rule %u", len);
        for (int mode : {PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL}) {
            const VisitRule r = visit_rule(len, mode);
            const VisitPlan v = visit_plan(len, mode);
            printf(" %u %d %d %u %u %u %u %u %u %d %d", r.nhead, r.tail_lo, r.tail_top, r.visited, r.head_chunks(), r.tail_chunk0(), r.tail_chunks(),
                   v.visited, v.nhead, v.tail_top, v.nseg);
            for (int s = 0; s < 2; ++s) {
                if (s < v.nseg) printf(" %u %u %u %d", v.segs[s].lo, v.segs[s].hi, v.segs[s].ord0, v.segs[s].descending);
                else printf(" 0 0 0 0");
            }
        }
        printf("\n");
    }
}

static void ord_line(uint32_t len, int mode) {
    const VisitRule r = visit_rule(len, mode);
    const uint32_t npos = len + 17;                                   // positions 0 .. len + 16
    uint64_t seen = 0, bad_inverse = 0, bad_cover = 0;
    for (uint32_t pos = 0; pos < npos; ++pos) {
        const int32_t o = r.ord_of((int32_t)pos);
        if (o < 0) continue;
        ++seen;
        bad_inverse += (uint32_t)o >= r.visited || r.pos_of((uint32_t)o) != (int32_t)pos;
    }
    for (uint32_t ord = 0; ord < r.visited; ++ord) {
        const int32_t pos = r.pos_of(ord);
        bad_inverse += pos < 0 || (uint32_t)pos >= npos || r.ord_of(pos) != (int32_t)ord;
    }
    std::vector<uint32_t> times(npos + 16, 0);
    const auto take = [&](uint32_t chunk0, uint32_t n, uint32_t lo, uint32_t hi) {
        for (uint32_t c = chunk0; c < chunk0 + n; ++c)
            for (uint32_t k = 0; k < 16; ++k) {
                const uint32_t pos = 16 * c + k;
                if (pos >= lo && pos < hi) { if (pos < times.size()) ++times[pos]; else ++bad_cover; }
            }
    };
    take(0, r.head_chunks(), 0, r.nhead);
    take(r.tail_chunk0(), r.tail_chunks(), r.tail_begin(), r.tail_end());
    for (uint32_t pos = 0; pos < times.size(); ++pos) bad_cover += times[pos] != (pos < npos && r.ord_of((int32_t)pos) >= 0 ? 1u : 0u);
    printf("ord %u %d %u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", len, mode, r.visited, seen, bad_inverse, bad_cover);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rng32() {                                             // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static void compress_line(uint32_t mask) {
    uint32_t mv[5];
    compress_masks(mask, mv);
    uint64_t bad = 0;
    const int tried = 256;
    for (int t = 0; t < tried; ++t) {
        const uint32_t x = (t == 0 ? 0xFFFFFFFFu : rng32()) & mask;
        uint32_t want = 0;
        for (int b = 0, at = 0; b < 32; ++b)
            if (mask >> b & 1u) want |= (x >> b & 1u) << at++;
        bad += ix_compress(x, mv) != want;
    }
    printf("compress %u %d %" PRIu64 "\n", mask, tried, bad);
}

int main(int argc, char **argv) {
    printf("consts %d %d %d\n", PBA_IX_MAX_LOGP, PBA_IX_LVL_BITS, PBA_IX_PART_AVG);
    for (int i = 1; i < argc; ++i) {
        unsigned long long a = 0, b = 0;
        int mode = 0;
        if (sscanf(argv[i], "v:%llu:%d", &a, &mode) == 2) visit_line((uint32_t)a, mode);
        else if (sscanf(argv[i], "p:%llu", &a) == 1) plan_line(a);
        else if (sscanf(argv[i], "r:%llu:%llu", &a, &b) == 2 && a <= b && b <= 0xFFFFFFFFull) rule_lines(a, b);
        else if (sscanf(argv[i], "o:%llu:%d", &a, &mode) == 2) ord_line((uint32_t)a, mode);
        else if (sscanf(argv[i], "c:%llu", &a) == 1) compress_line((uint32_t)a);
        else return 2;
    }
    return 0;
}
