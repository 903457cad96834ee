// phase.h -- the phase rule over allele records (include/pba.h: pba_phase_*): one body for the kernels of
// pba_phase.hip and the host checks.  Integers alone.
//
//   v        of a record at a site whose packed word (sites.h: site_pack) is `pack`: +1 if allele == major, -1 if allele ==
//            minor, else 0 (major is asked first: a caller's list may name one allele twice)
//   o0       of a SEL site: +1 if own == major, -1 if own == minor, else 0
//   lab(g)   sign(g) if |g| >= min_margin, else 0
// A classified record is one word: the SEL rank of its site above two bits of v, so that no pass after the first touches a
// pba_site or an allele.
#ifndef PBA_PHASE_H
#define PBA_PHASE_H

#include <stdint.h>

#include "pba.h"

#if defined(__HIPCC__)
#define PBA_PHASE_HD __host__ __device__
#else
#define PBA_PHASE_HD
#endif

static const uint32_t kPhaseMaxSel = 1u << 30;       // SEL ranks must fit the 30 bits of a classified record
static const int kPhaseMaxSelfWeight = 0xFFFF;

PBA_PHASE_HD static inline int phase_sign(int x) { return (x > 0) - (x < 0); }
PBA_PHASE_HD static inline int phase_lab(int g, int min_margin) { return (g >= min_margin) - (g <= -min_margin); }
PBA_PHASE_HD static inline int phase_value(uint32_t pack, uint32_t allele) {
    return allele == ((pack >> 4) & 15u) ? 1 : (allele == ((pack >> 8) & 15u) ? -1 : 0);
}
PBA_PHASE_HD static inline int phase_seed(uint32_t pack) { return phase_value(pack, pack & 15u); }
// the classified record: rank << 2 | (0: v = 0, 1: v = +1, 2: v = -1)
PBA_PHASE_HD static inline uint32_t phase_rec(uint32_t rank, int v) { return rank << 2 | (v > 0 ? 1u : (v < 0 ? 2u : 0u)); }
PBA_PHASE_HD static inline uint32_t phase_rec_rank(uint32_t w) { return w >> 2; }
PBA_PHASE_HD static inline int phase_rec_value(uint32_t w) { return (int)(w & 1u) - (int)((w >> 1) & 1u); }

static inline bool phase_params_ok(const pba_phase_params &p) {
    return p.n_iter >= 0 && p.n_iter <= PBA_PHASE_MAX_ITER && p.min_margin >= 1 && p.self_weight >= 0 && p.self_weight <= kPhaseMaxSelfWeight;
}

#endif
