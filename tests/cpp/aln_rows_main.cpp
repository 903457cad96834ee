// aln_rows_main.cpp -- csrc/aln_rows.h alone, as a host program (tests/test_aln_rows_cpu.py builds it, with the sanitizers
// where the compiler has them): the script walker against hand-written scripts and the row layout against hand-written rows.
// Every buffer is an exact-size heap array, so a read or write outside one is the sanitizer's to report.  It exits non-zero
// at the first check that fails (the exit code is the check's line) and prints "ok <checks>" at the end.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "aln_rows.h"

static int n_checks = 0;
#define CHECK(cond) do { ++n_checks; if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); exit(__LINE__ % 250 + 1); } } while (0)

struct Met { uint32_t code; int op, i, j; };
static bool same(const Met &m, uint32_t code, int op, int i, int j) { return m.code == code && m.op == op && m.i == i && m.j == j; }

// the walk of a script over exact-size copies of its inputs; *ok: what script_walk returned
static std::vector<Met> walk(const std::vector<uint8_t> &ops, const std::vector<char> &a, const std::vector<char> &b, bool b_is_query,
                             bool *ok, int stop_after = -1) {
    std::vector<Met> met;
    *ok = script_walk(ops.empty() ? nullptr : ops.data(), (int32_t)ops.size(), a.empty() ? nullptr : a.data(),
                      b.empty() ? nullptr : b.data(), b_is_query, [&](uint32_t code, int op, int i, int j) {
                          met.push_back(Met{code, op, i, j});
                          return (int)met.size() != stop_after;
                      });
    return met;
}

// runs and counts on top of the walker, the way pba_cigar_from_script folds it (flags: PBA_CIG_*)
static std::vector<uint32_t> runs_of(const std::vector<uint8_t> &ops, const std::vector<char> &a, const std::vector<char> &b, uint32_t flags,
                                     pba_aln_counts *c) {
    std::vector<uint32_t> runs;
    *c = pba_aln_counts{0, 0, 0, 0};
    const bool ok = script_walk(ops.data(), (int32_t)ops.size(), a.data(), b.data(), (flags & PBA_CIG_B_IS_QUERY) != 0,
                                [&](uint32_t code, int, int, int) {
                                    aln_count(*c, code);
                                    if (!runs.empty() && (runs.back() & 15u) == code) runs.back() += 16u;
                                    else runs.push_back(16u | code);
                                    return true;
                                });
    CHECK(ok);
    if (flags & PBA_CIG_REVERSED) return std::vector<uint32_t>(runs.rbegin(), runs.rend());
    return runs;
}

static void walker() {
    bool ok = false;
    // the empty script: nothing is met, nothing is read
    CHECK(walk({}, {}, {}, false, &ok).empty() && ok);
    CHECK(walk({}, {}, {}, true, &ok).empty() && ok);
    // a leading INSERT, a mismatch, a DELETE, a trailing INSERT: a = ACGT, b = TAGTG
    const std::vector<uint8_t> s1{2, 1, 1, 3, 1, 2};
    const std::vector<char> a1{'A', 'C', 'G', 'T'}, b1{'T', 'A', 'G', 'T', 'G'};
    std::vector<Met> m = walk(s1, a1, b1, false, &ok);
    CHECK(ok && m.size() == 6);
    CHECK(same(m[0], PBA_CIG_DEL, 2, 0, 0) && same(m[1], PBA_CIG_EQ, 1, 0, 1) && same(m[2], PBA_CIG_X, 1, 1, 2));
    CHECK(same(m[3], PBA_CIG_INS, 3, 2, 3) && same(m[4], PBA_CIG_EQ, 1, 3, 3) && same(m[5], PBA_CIG_DEL, 2, 4, 4));
    m = walk(s1, a1, b1, true, &ok);                       // b as the query: the gaps change names, nothing else does
    CHECK(ok && m.size() == 6);
    CHECK(same(m[0], PBA_CIG_INS, 2, 0, 0) && same(m[1], PBA_CIG_EQ, 1, 0, 1) && same(m[2], PBA_CIG_X, 1, 1, 2));
    CHECK(same(m[3], PBA_CIG_DEL, 3, 2, 3) && same(m[4], PBA_CIG_EQ, 1, 3, 3) && same(m[5], PBA_CIG_INS, 2, 4, 4));
    // every flag combination, folded to runs and counts
    pba_aln_counts c;
    CHECK((runs_of(s1, a1, b1, 0u, &c) == std::vector<uint32_t>{18, 23, 24, 17, 23, 18}));
    CHECK(c.n_eq == 2 && c.n_x == 1 && c.n_ins == 1 && c.n_del == 2);
    CHECK((runs_of(s1, a1, b1, PBA_CIG_REVERSED, &c) == std::vector<uint32_t>{18, 23, 17, 24, 23, 18}));
    CHECK((runs_of(s1, a1, b1, PBA_CIG_B_IS_QUERY, &c) == std::vector<uint32_t>{17, 23, 24, 18, 23, 17}));
    CHECK(c.n_eq == 2 && c.n_x == 1 && c.n_ins == 2 && c.n_del == 1);
    CHECK((runs_of(s1, a1, b1, PBA_CIG_REVERSED | PBA_CIG_B_IS_QUERY, &c) == std::vector<uint32_t>{17, 23, 18, 24, 23, 17}));
    // runs longer than one op: a = AAAT, b = AAATT as 3 MATCH, 2 INSERT, 1 DELETE
    const std::vector<uint8_t> s2{1, 1, 1, 2, 2, 3};
    const std::vector<char> a2{'A', 'A', 'A', 'T'}, b2{'A', 'A', 'A', 'T', 'T'};
    CHECK((runs_of(s2, a2, b2, 0u, &c) == std::vector<uint32_t>{55, 34, 17}));
    CHECK(c.n_eq == 3 && c.n_x == 0 && c.n_ins == 1 && c.n_del == 2);
    CHECK((runs_of(s2, a2, b2, PBA_CIG_REVERSED, &c) == std::vector<uint32_t>{17, 34, 55}));
    CHECK((runs_of(s2, a2, b2, PBA_CIG_B_IS_QUERY, &c) == std::vector<uint32_t>{55, 33, 18}));
    CHECK((runs_of(s2, a2, b2, PBA_CIG_REVERSED | PBA_CIG_B_IS_QUERY, &c) == std::vector<uint32_t>{18, 33, 55}));
    m = walk(s2, a2, b2, false, &ok);
    CHECK(ok && same(m[3], PBA_CIG_DEL, 2, 3, 3) && same(m[4], PBA_CIG_DEL, 2, 3, 4) && same(m[5], PBA_CIG_INS, 3, 3, 5));
    // a script of INSERTs only reads no a-element, one of DELETEs only no b-element
    m = walk({2, 2}, {}, {'A', 'C'}, false, &ok);
    CHECK(ok && m.size() == 2 && same(m[1], PBA_CIG_DEL, 2, 0, 1));
    m = walk({3, 3}, {'A', 'C'}, {}, false, &ok);
    CHECK(ok && m.size() == 2 && same(m[1], PBA_CIG_INS, 3, 1, 0));
    // a byte that is no op ends the walk with false, after the ops before it
    m = walk({1, 0, 1}, {'A', 'C'}, {'A', 'C'}, false, &ok);
    CHECK(!ok && m.size() == 1);
    m = walk({4}, {'A'}, {'A'}, false, &ok);
    CHECK(!ok && m.empty());
    // ... and so does the callee
    m = walk(s1, a1, b1, false, &ok, 3);
    CHECK(!ok && m.size() == 3);
}

// rows_layout into an exact-size array of `cap` elements filled with -1
static std::vector<int> laid(const std::vector<std::vector<int>> &of, const std::vector<uint64_t> &row_of, uint64_t n_rows, uint64_t cap,
                             std::vector<uint64_t> *off, uint64_t *n_slots) {
    std::vector<int> dst((size_t)cap, -1);
    off->assign((size_t)n_rows + 1, ~0ull);
    rows_layout(of, row_of, n_rows, cap ? dst.data() : nullptr, cap, off->data(), n_slots);
    return dst;
}

static void layout() {
    // six rows, jobs for rows 0, 2, 3 (nothing to show) and 5
    const std::vector<std::vector<int>> of{{1, 2}, {3}, {}, {4, 5, 6}};
    const std::vector<uint64_t> row_of{0, 2, 3, 5}, want_off{0, 2, 2, 3, 3, 3, 6};
    std::vector<uint64_t> off;
    uint64_t n_slots = 99;
    CHECK((laid(of, row_of, 6, 6, &off, &n_slots) == std::vector<int>{1, 2, 3, 4, 5, 6}));          // cut at no row
    CHECK(off == want_off && n_slots == 6);
    CHECK((laid(of, row_of, 6, 8, &off, &n_slots) == std::vector<int>{1, 2, 3, 4, 5, 6, -1, -1}));  // room to spare
    CHECK(off == want_off && n_slots == 6);
    CHECK((laid(of, row_of, 6, 5, &off, &n_slots) == std::vector<int>{1, 2, 3, -1, -1}));           // cut at the last row: whole rows only
    CHECK(off == want_off && n_slots == 6);
    CHECK((laid(of, row_of, 6, 2, &off, &n_slots) == std::vector<int>{1, 2}));                      // cut at a middle row
    CHECK(off == want_off && n_slots == 6);
    CHECK((laid(of, row_of, 6, 1, &off, &n_slots) == std::vector<int>{-1}));                        // cut at the first row
    CHECK(off == want_off && n_slots == 6);
    CHECK(laid(of, row_of, 6, 0, &off, &n_slots).empty());                                          // no array at all
    CHECK(off == want_off && n_slots == 6);
    // a row that fits behind one that did not stays out: the rows are whole and in order
    CHECK((laid({{1, 2}, {3, 4, 5}, {6}}, {0, 1, 2}, 3, 3, &off, &n_slots) == std::vector<int>{1, 2, -1}));
    CHECK((off == std::vector<uint64_t>{0, 2, 5, 6}) && n_slots == 6);
    // no rows, and rows without any job
    CHECK(laid({}, {}, 0, 0, &off, &n_slots).empty() && off == std::vector<uint64_t>{0} && n_slots == 0);
    CHECK((laid({}, {}, 2, 4, &off, &n_slots) == std::vector<int>{-1, -1, -1, -1}) && (off == std::vector<uint64_t>{0, 0, 0}) && n_slots == 0);
}

int main() {
    walker();
    layout();
    printf("ok %d\n", n_checks);
    return 0;
}
