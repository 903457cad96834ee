// qual.h -- per-base evidence of an evolved set (include/pba.h: pba_qual): the Phred rule, one body for the
// host entry point, the device check and the evidence write passes of pba_pileup.hip, and the object the evidence lives in.
//
// A character that evolve emits from box i carries
//   agree  max4 of the counter it was elected from (sel, or sup for a split box)
//   depth  min(tot - 1, 65535): the rows that consumed the box by MATCH or DELETE
//   src    i, with PBA_QUAL_SUP set for the character split from the suppliment
//   qv     qual_phred(agree, N, qmax), N = tot - 1 + weight
// qual_phred is the Laplace estimate (against + 1) / (N + 2) on the Phred scale, rounded down, in integers alone: the largest
// q in [0, qmax] with (against + 1) * S[q] <= (N + 2) * 1000, S[q] = d[q mod 10] * 10^(q div 10), d = floor(1000 * 10^(r/10)).
// S rises strictly with q, so the search goes up by decades (S[10 (k + 1)] = 10 S[10 k]) and then by the steps inside the
// last decade that held, each to its first failure: a handful of 64-bit products at 20x.  With N < 2^31 + 65 535 and
// q <= 60 the products stay below 2^63.
#ifndef PBA_QUAL_H
#define PBA_QUAL_H

#include <stdint.h>

#include <vector>

#include "pba.h"

#if defined(__HIPCC__)
#define PBA_QUAL_HD __host__ __device__
#else
#define PBA_QUAL_HD
#endif

PBA_QUAL_HD static inline int qual_phred(uint32_t agree, uint64_t n, int qmax) {
    const uint64_t against = n > agree ? n - agree : 0ull;      // a suppliment counter can exceed N (several INSERTs of one row)
    const uint64_t rhs = (n + 2ull) * 1000ull;
    uint64_t u = against + 1ull;                                // (against + 1) * 10^k; u * 1000 <= rhs throughout
    int q = 0;                                                  // 10 k
    while (q + 10 <= qmax && u * 10000ull <= rhs) { u *= 10ull; q += 10; }      // the decade: S[10 (k + 1)] = 10000 * 10^k
    // then the step inside it: S[10 k + r] = d[r] * 10^k, d as literals
#define PBA_QUAL_STEP(r, d) if (q + (r) > qmax || u * (d) > rhs) return q + (r) - 1
    PBA_QUAL_STEP(1, 1258ull); PBA_QUAL_STEP(2, 1584ull); PBA_QUAL_STEP(3, 1995ull);
    PBA_QUAL_STEP(4, 2511ull); PBA_QUAL_STEP(5, 3162ull); PBA_QUAL_STEP(6, 3981ull);
    PBA_QUAL_STEP(7, 5011ull); PBA_QUAL_STEP(8, 6309ull); PBA_QUAL_STEP(9, 7943ull);
#undef PBA_QUAL_STEP
    return q + 9;
}

// where an evidence write pass leaves its records: four arrays over the characters of one evolved text (pba_pileup.hip)
struct QualInto {
    uint8_t *qv;
    uint16_t *depth, *agree;
    uint32_t *src;
    int weight, qmax;
};

// the evidence of n sequences, sequence k at [h_off[k], h_off[k + 1]) of every array; all arrays on the device
struct pba_qual {
    int device;
    uint32_t n;
    uint8_t *d_qv;
    uint16_t *d_depth, *d_agree;
    uint32_t *d_src;
    unsigned long long *d_off;          // n + 1
    std::vector<uint64_t> h_off;        // n + 1
};

#endif
