// sites.h -- the variant-site rule over one vote box as it stands before evolve (include/pba.h: pba_site): one
// body for the flag pass, the compaction pass and the host checks of pba_sites.hip.  Integers alone.
//
// Box i of a target, `weight` the pile-up's:
//   N       tot - 1 + weight: the rows that consumed the box by MATCH or DELETE, and the target itself (qual.h's N)
//   c[0..3] the four sel counters (the target's own base carries weight), c[4] = c[DEL] = N - (c[A] + c[C] + c[G] + c[T])
//   major   the first maximal allele in the order A, C, G, T, DEL (cons_winner's order, extended); minor: the first maximal
//           among the other four
// SEL site:  N >= min_depth, c[minor] >= min_alt, c[minor] * 1000 >= min_permille * N.
// SUP site:  the same three tests with max4(sup) in place of c[minor]; its minor is the winning sup base, its n_major 0.
// A counter above 65 535 does not exist in a box (consensus.h), so every product stays far below 2^63.
#ifndef PBA_SITES_H
#define PBA_SITES_H

#include <stdint.h>

#include "pba.h"

#if defined(__HIPCC__)
#define PBA_SITES_HD __host__ __device__
#else
#define PBA_SITES_HD
#endif

struct SiteRule { int min_depth, min_alt, min_permille, weight; };

// what the rule finds in one box: kinds = PBA_SITE_SEL | PBA_SITE_SUP bits (0: no site)
struct SiteCall {
    uint32_t kinds;
    uint8_t major, minor, sup_minor;
    uint32_t n, n_major, n_minor, n_sup;
};

PBA_SITES_HD static inline bool site_passes(const SiteRule &r, uint64_t n, uint64_t alt) {
    return n >= (uint64_t)r.min_depth && alt >= (uint64_t)r.min_alt && alt * 1000ull >= (uint64_t)r.min_permille * n;
}

PBA_SITES_HD static inline SiteCall site_rule(unsigned long long sel, unsigned long long sup, int tot, const SiteRule &r) {
    SiteCall o;
    int64_t c[5];
    int64_t sum = 0;
    for (int k = 0; k < 4; ++k) { c[k] = (int64_t)((sel >> (16 * k)) & 0xFFFFull); sum += c[k]; }
    const int64_t n = (int64_t)tot - 1 + r.weight;
    c[4] = n > sum ? n - sum : 0;
    int major = 0;
    for (int k = 1; k < 5; ++k) if (c[k] > c[major]) major = k;
    int minor = major == 0 ? 1 : 0;
    for (int k = 0; k < 5; ++k) if (k != major && c[k] > c[minor]) minor = k;
    int sw = 0;
    int64_t sv = (int64_t)(sup & 0xFFFFull);
    for (int k = 1; k < 4; ++k) { const int64_t v = (int64_t)((sup >> (16 * k)) & 0xFFFFull); if (v > sv) { sv = v; sw = k; } }
    const uint64_t un = n > 0 ? (uint64_t)n : 0ull;
    o.kinds = (site_passes(r, un, (uint64_t)c[minor]) ? (uint32_t)PBA_SITE_SEL : 0u) | (site_passes(r, un, (uint64_t)sv) ? (uint32_t)PBA_SITE_SUP : 0u);
    o.major = (uint8_t)major; o.minor = (uint8_t)minor; o.sup_minor = (uint8_t)sw;
    o.n = (uint32_t)un; o.n_major = (uint32_t)c[major]; o.n_minor = (uint32_t)c[minor]; o.n_sup = (uint32_t)sv;
    return o;
}

// the record of one kind (PBA_SITE_SEL or PBA_SITE_SUP) of a box the rule calls a site
PBA_SITES_HD static inline pba_site site_record(const SiteCall &c, uint32_t kind, int32_t target, int32_t pos, int own) {
    pba_site s;
    s.target = target; s.pos = pos; s.kind = (uint8_t)kind; s.own = (uint8_t)own; s.major = c.major;
    s.n = c.n;
    if (kind == (uint32_t)PBA_SITE_SEL) { s.minor = c.minor; s.n_major = c.n_major; s.n_minor = c.n_minor; }
    else { s.minor = c.sup_minor; s.n_major = 0u; s.n_minor = c.n_sup; }
    return s;
}

// the word the allele sink reads per SEL site
PBA_SITES_HD static inline uint32_t site_pack(const pba_site &s) { return (uint32_t)s.own | (uint32_t)s.major << 4 | (uint32_t)s.minor << 8; }

#endif
