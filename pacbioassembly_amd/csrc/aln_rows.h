// aln_rows.h -- what the host twins and the row-level entry points of pba_cigar.hip and pba_windows.hip share that needs no
// device: the walker over an edit script in the CIGAR's words, and the layout of per-row results in the caller's array.
// Plain C++ (tests/cpp/aln_rows_main.cpp plays both under the sanitizers).
#ifndef PBA_ALN_ROWS_H
#define PBA_ALN_ROWS_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "pba.h"

// Every op of a script (the reference's numbering: 1 MATCH, 2 INSERT, 3 DELETE), origin-first, as f(code, op, i, j): code is
// the op in the CIGAR's words (PBA_CIG_*: `=` / `X` per element pair, the gaps named with a or, b_is_query, b as the query);
// i and j are the a- and b-elements consumed before it, so a MATCH compares a[i] with b[j], a DELETE consumes a[i], an INSERT
// b[j].  Stops with false at a byte that is no op, or where f says false.
template <class F>
static inline bool script_walk(const uint8_t *ops, int32_t nedit, const char *a_elems, const char *b_elems, bool b_is_query, F f) {
    int i = 0, j = 0;
    for (int32_t k = 0; k < nedit; ++k) {
        const int op = ops[k];
        uint32_t code;
        if (op == 1) code = a_elems[i] == b_elems[j] ? PBA_CIG_EQ : PBA_CIG_X;
        else if (op == 2) code = b_is_query ? PBA_CIG_INS : PBA_CIG_DEL;        // INSERT consumes b only
        else if (op == 3) code = b_is_query ? PBA_CIG_DEL : PBA_CIG_INS;        // DELETE consumes a only
        else return false;
        if (!f(code, op, i, j)) return false;
        if (op != 2) ++i;
        if (op != 3) ++j;
    }
    return true;
}
static inline void aln_count(pba_aln_counts &c, uint32_t code) {
    if (code == PBA_CIG_EQ) ++c.n_eq; else if (code == PBA_CIG_X) ++c.n_x; else if (code == PBA_CIG_INS) ++c.n_ins; else ++c.n_del;
}

// The results of the jobs (of[j]: job j's elements; row_of[j]: its row, ascending) dense and in row order at dst: whole rows
// only, up to the first that does not fit cap.  off[0 .. n_rows] and *n_slots are complete whatever fits (a row without a job
// has nothing).
template <class T>
static inline void rows_layout(const std::vector<std::vector<T>> &of, const std::vector<uint64_t> &row_of, uint64_t n_rows, T *dst,
                               uint64_t cap, uint64_t *off, uint64_t *n_slots) {
    std::vector<uint32_t> row_n(n_rows, 0);
    uint64_t pos = 0;
    bool fits = true;
    for (size_t j = 0; j < of.size(); ++j) {
        const std::vector<T> &r = of[j];
        row_n[row_of[j]] = (uint32_t)r.size();
        if (fits && pos + r.size() <= cap) { if (!r.empty()) memcpy(dst + pos, r.data(), sizeof(T) * r.size()); }
        else fits = false;
        pos += r.size();
    }
    off[0] = 0;
    for (uint64_t k = 0; k < n_rows; ++k) off[k + 1] = off[k] + row_n[k];
    *n_slots = off[n_rows];
}

#endif
