"""What every input of prefilter_inputs.py is, from two references and no GPU: the oracle (Oracle.align's fail_row, Oracle.cell)
and the plain unbanded edit-distance matrix over the first 64 x 64 square (prefilter_inputs.plain_diag).  prefilter.h's
exactness claim -- on cell (i, i) the banded and the plain matrix agree while the check passes -- is stated here by requiring
both to give the same first failing row for every generated pair: a pair that drifted fails, it is not dropped."""
import itertools

import numpy as np
import pytest

import prefilter_inputs as pi
from conftest import MASK_PAT

ROWS = set(range(11, 65))


def both_fail_rows(oracle, x, y, R):
    res = oracle.align(x, y, R)
    return res, res["fail_row"] if res["rc"] == -1 else 0, pi.plain_fail_row(x, y, R)


def test_plain_matrix_is_the_edit_distance():
    """the second reference against the textbook recurrence, cell by cell along the diagonal"""
    rng = np.random.RandomState(1)
    for _ in range(20):
        a, b = pi.ar.rand_seq(rng, 40), pi.ar.rand_seq(rng, 37)
        D = np.zeros((38, 38), int)
        D[:, 0] = D[0, :] = np.arange(38)
        for i, j in itertools.product(range(1, 38), range(1, 38)):
            D[i, j] = min(D[i - 1, j] + 1, D[i, j - 1] + 1, D[i - 1, j - 1] + (a[i - 1] != b[j - 1]))
        assert (pi.plain_diag(a, b) == np.diagonal(D)).all()


@pytest.mark.parametrize("R", pi.RS)
def test_thresholds_and_stretch_ends_in_fp64(R):
    T = [int(np.floor(np.float64(i) * np.float64(R))) for i in range(67)]
    assert list(pi.thresholds(R, 66)) == T
    ends = [i for i in range(11, 65) if T[i + 1] != T[i]]
    assert pi.stretch_ends(R) == ends and all(0 <= b - a <= 1 for a, b in zip(T, T[1:]))
    if R == 0.07:
        assert T[11:15] == [0, 0, 0, 0] and T[15] == 1
    if R == 0.25:
        assert [i for i in range(11, 65) if np.float64(i) * np.float64(R) == T[i]] == list(range(12, 65, 4))    # on integers
    if R == 0.9:
        assert max(T[:33]) == 28 and max(T[:65]) == 57 and len([e for e in ends if e <= 32]) >= 19


@pytest.mark.parametrize("entry", list(pi.ENTRIES))
@pytest.mark.parametrize("R", pi.RS)
def test_reachable_first_failing_rows(oracle, entry, R):
    """The set the recurrence gives is the set a search over every placement gives (rows up to 24, where the seed constrains),
    every row in it is built -- as a lasting failure and as a blip -- and both references name that row; no other row builds."""
    pat, fwd = pi.ENTRIES[entry]
    reach = pi.reachable(R, pat, fwd)
    T, wild = pi.thresholds(R), pi.seed_rows(pat, fwd)
    free = [i for i in range(1, 25) if pi.is_free(i, wild)]
    brute = set()
    for k in range(len(free) + 1):
        for S in itertools.combinations(free, k):
            c = np.searchsorted(np.array(S, int), np.arange(25), side="right")
            bad = [i for i in range(11, 25) if c[i] > T[i]]
            if bad:
                brute.add(bad[0])
    assert brute == {f for f in reach if f <= 24}
    rng = np.random.RandomState(7000 + int(R * 100))
    for f in range(11, 65):
        for build in (pi.fail_first_at, pi.blip_at):
            if f not in reach:
                with pytest.raises(pi.Unreachable):
                    build(rng, f, R, pat, fwd)
                continue
            x, y = build(rng, f, R, pat, fwd)
            res, fo, fp = both_fail_rows(oracle, x, y, R)
            assert fo == fp == f, (entry, R, build.__name__, f, fo, fp)
            assert all(x[i] == y[i] for i in range(16) if i + 1 not in wild)        # the seed's care positions agree
            if build is pi.blip_at:                                                   # ... and only f's stretch fails
                d = pi.plain_diag(x, y)
                end = min(e for e in pi.stretch_ends(R) + [64] if e >= f)
                assert [i for i in range(11, 65) if d[i] > T[i]] == list(range(f, end + 1)), (entry, R, f)


def test_reachable_rows_cover_11_to_64_and_the_facts_the_docstring_names():
    union = set()
    for entry, (pat, fwd) in pi.ENTRIES.items():
        for R in pi.RS:
            union |= set(pi.reachable(R, pat, fwd))
    assert union == ROWS
    fwd_main = set().union(*(pi.reachable(R, MASK_PAT, True) for R in np.arange(0.01, 1.0, 0.01)))
    assert not fwd_main & {13, 14, 15, 16}                                # no forward MASK_PAT pair fails first there, whatever R
    assert {13, 14, 15, 16} <= set().union(*(pi.reachable(R, pi.ALT_PAT, True) for R in pi.RS))
    assert 13 in pi.reachable(0.30, MASK_PAT, False)                      # backward: the wildcards sit at rows 5, 7, 10, 13
    assert 11 in pi.reachable(0.25, MASK_PAT) and 11 not in pi.reachable(0.28, MASK_PAT)     # three wildcards by row 10: 3 > 2.75, 3 <= 3.08
    assert 17 not in pi.reachable(0.30, MASK_PAT)
    for pat, fwd in pi.ENTRIES.values():
        assert pi.reachable(0.9, pat, fwd) == []
    assert pi.seed_rows(MASK_PAT) == {4, 7, 10, 12} and pi.seed_rows(MASK_PAT, False) == {5, 7, 10, 13}


@pytest.mark.parametrize("fwd", [True, False])
@pytest.mark.parametrize("R", pi.TIGHT_RS)
def test_tightrope_touches_every_stretch_end(oracle, R, fwd):
    """cost(i, i) = floor((double) i R) at every stretch end of 11 .. 64 in both references, every row passes, and the whole
    alignment is accepted.  Behind MASK_PAT one stretch end is out of any pair's reach: row 16 at R = 0.30 (T = 4, and a pair
    that passed row 12 or 13 with T = 3 has no free row left before 17)."""
    T, ends = pi.thresholds(R), pi.stretch_ends(R)
    mc = pi.max_costs(R, MASK_PAT, fwd)
    out_of_reach = [e for e in ends if mc[e] < T[e]]
    assert out_of_reach == ([16] if R == 0.30 else [])
    rng = np.random.RandomState(7100 + int(R * 100) + fwd)
    for m in (64, 65, 96, 200):
        x, y = pi.tightrope(rng, R, m, MASK_PAT, fwd)
        res, fo, fp = both_fail_rows(oracle, x, y, R)
        assert res["rc"] > 0 and fo == fp == 0 and res["cost"] == mc[64]
        d = pi.plain_diag(x, y)
        for e in ends:
            assert oracle.cell(e, e)[0] == d[e] == mc[e], (R, fwd, m, e)
            assert e in out_of_reach or d[e] == T[e]
        assert x[64:] == y[64:]


def test_dearest_seeded_pair_passes_at_R_09(oracle):
    """R = 0.9: every free row differs, cost(i, i) = i - 12 from row 16 on, every row up to 120 passes and row 121 fails"""
    rng = np.random.RandomState(7200)
    x = pi.base_side(rng, 64) + np.frombuffer(b"AC", np.uint8)[rng.randint(0, 2, 96)].tobytes()
    y = pi.other_side(rng, x, (), junk_from=1, wild=pi.seed_rows(MASK_PAT))
    res, fo, fp = both_fail_rows(oracle, x, y, 0.9)
    assert fo == 121 and fp == 0 and list(pi.plain_diag(x, y)[16:65]) == list(range(4, 53))
    assert (pi.plain_diag(x, y)[11:] <= pi.thresholds(0.9)[11:65]).all()


def test_row_10_is_not_checked(oracle):
    rng = np.random.RandomState(7300)
    x, y = pi.edge10_pair(rng, 96)
    res, fo, fp = both_fail_rows(oracle, x, y, pi.EDGE10_R)
    assert res["rc"] > 0 and fo == fp == 0
    assert oracle.cell(10, 10)[0] == pi.plain_diag(x, y)[10] == 3 > 10 * pi.EDGE10_R and oracle.cell(11, 11)[0] == 3 <= 11 * pi.EDGE10_R


@pytest.mark.parametrize("m", [31, 32, 33, 63, 64, 65])
def test_short_sides(oracle, m):
    """the lengths around the prefilters' 32 and 64 rows: a pair of m elements that fails first at a row within them"""
    rng = np.random.RandomState(7400 + m)
    for R in (0.15, 0.30):
        f = max(r for r in pi.reachable(R, MASK_PAT) if r <= m)
        x, y = pi.fail_first_at(rng, f, R, m=m)
        res, fo, fp = both_fail_rows(oracle, x, y, R)
        assert len(x) == len(y) == m == res["len_a"] and fo == fp == f


@pytest.mark.parametrize("R", pi.RS)
def test_overlap_case_candidates_agree_in_both_references(oracle, R):
    """Every candidate of the all-vs-all case -- the indel pairs among them, whose cheapest path leaves the diagonal -- gets the
    same verdict on rows 11 .. 64 from the oracle and from the plain matrix."""
    texts, designed, nq, wt = pi.overlap_case(R)
    kinds = {d[:4]: d[4] for d in designed}
    cands, _ = pi.overlap_candidates(texts, MASK_PAT)
    assert {d[:4] for d in designed} <= {c[:4] for c in cands}
    n_indel = 0
    for t, q, fwd, p, a, b in cands:
        res = oracle.align(a, b, R)
        n = min(res["len_a"], res["len_b"], 64)
        fo = res["fail_row"] if res["rc"] == -1 and 0 < res["fail_row"] <= n else 0
        assert fo == pi.plain_fail_row(a[:res["len_a"]], b[:res["len_b"]], R, n), (R, kinds.get((t, q, fwd, p)), res)
        if kinds.get((t, q, fwd, p)) == "indel":
            n_indel += 1
            assert R < 0.15 or fo == 0
            assert max(pi.plain_diag(a, b)[25:33]) == 2 < sum(x != y for x, y in zip(a[:32], b[:32]))      # the diagonal alone counts more
    assert n_indel == 2 * len(pi.OVL_INDEL_ROWS)


@pytest.mark.parametrize("view", ["forward", "rc"])
@pytest.mark.parametrize("R", [0.15, 0.30])
def test_straddle_case_shows_the_walks_group_edges(oracle, R, view):
    """The three targets of straddle_case, as enumeration and the oracle see them (both ways the GPU test runs them): each
    has 65 .. 192 listed candidates and shows its situation at slots 63 | 64 of the sorted slice -- (a) a run that crosses the
    edge, fails in the second group at rows 33 .. 64 and succeeds behind that; (b) a run that crosses it with its first success
    before and another success behind; (c) a run that starts at slot 64.  And a plain walk of the enumeration in slice order
    gives the oracle's rows and pair count: the order is the one the reference tries candidates in."""
    views, nq = pi.straddle_views(R)
    texts, qtexts = views[view]
    W = pi.walk_composition(oracle, texts, qtexts, R)
    assert pi.straddle_situations(W["slices"]) == {nq: "a", nq + 1: "b", nq + 2: "c"}
    for t in range(nq, nq + 3):
        L = W["slices"][t]
        assert [c["q"] for c in L] == sorted(c["q"] for c in L)
        runs = [sum(c["q"] == q for c in L) for q in sorted({c["q"] for c in L})]
        assert min(runs) >= 10 and max(runs) <= 30 and {c["fwd"] for c in L} == {True, False}
        assert all(c["ok"] or (c["x"]["rc"] == -1 and 33 <= c["x"]["fail_row"] <= 64) for c in L)       # nothing the scan would stop
    assert W["n_pre"] == 0
    want, pairs = pi.oracle_composition(oracle, texts, qtexts, R)
    assert (W["rows"], W["pairs"]) == (want, pairs)
    hit = {(t, q) for t, q, *_ in want}
    assert len({(t, q) for t, q in hit if t >= nq}) == 5 and len(want) >= 10             # (b)'s two successes are one row; and the mirrors
