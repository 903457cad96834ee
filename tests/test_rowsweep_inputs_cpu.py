"""The inputs of tests/test_gpu_rowsweep.py are what they are named for: proven here from the oracle alone, so that no GPU
test can pass vacuously.  No GPU."""
import collections

import pytest

import rowsweep_inputs as ri


@pytest.fixture(scope="module")
def cases_exp(oracle):
    cs = ri.all_cases()
    return cs, ri.expected(oracle, cs)


def test_classes_and_proportions(cases_exp):
    cs, exp = cases_exp
    n = collections.Counter(c.cls for c in cs)
    assert set(n) == {f"group:W{w}" for w in (63, 65, 127, 129, 191, 193)} | {"small", "check_eq", "accept_eq", "tie_row", "tie_col"}
    assert all(v >= 6 for v in n.values()), n
    assert 3 * sum(x["rc"] >= 0 for x in exp) >= len(cs)
    assert 5 * sum(x["fail_row"] > 0 for x in exp) >= len(cs)
    # rejected by the acceptance alone, on a path that costs something
    assert sum(x["rc"] < 0 and x["fail_row"] == 0 and x["cost"] > 0 for x in exp) >= 4
    assert {(c.fa, c.fb) for c in cs} == {(False, False), (False, True), (True, False), (True, True)}
    assert all(len(c.a) < 600 and len(c.b) < 600 for c in cs)


def test_group_edges(cases_exp):
    cs, exp = cases_exp
    seen = collections.defaultdict(set)
    for c, x in zip(cs, exp):
        if not c.cls.startswith("group"):
            continue
        md = c.meta["md"]
        assert x["max_dst"] == md and c.cls == f"group:W{2 * md + 1}", c.tag
        assert (x["len_a"] > x["len_b"]) == (c.meta["a_longer"] and c.meta["delta"] > 0), c.tag
        # the clip: the longer side is cut to the shorter one + max_dst (deltas max_dst + 1 and max_dst + 40)
        assert max(x["len_a"], x["len_b"]) == c.meta["m"] + min(c.meta["delta"], md), c.tag
        seen[md].add((c.meta["m"], c.meta["delta"], c.meta["kind"], c.meta["a_longer"], (c.fa, c.fb)))
    assert sorted(seen) == list(ri.GROUP_MD)
    for md, s in seen.items():
        assert {t[0] for t in s} == set(ri.GROUP_M[md])
        for m in ri.GROUP_M[md]:
            assert {t[1] for t in s if t[0] == m} == {0, 1, md - 1, md, md + 1, md + 40}
        assert {(t[2], t[3]) for t in s} == {("true", False), ("true", True), ("unrel", False), ("unrel", True)}
        assert {t[4] for t in s} == {(False, False), (False, True), (True, False), (True, True)}, md
    grp = [(c, x) for c, x in zip(cs, exp) if c.cls.startswith("group")]
    for md in ri.GROUP_MD:                  # both outcomes at every width, with either side the longer one
        for a_longer in (False, True):
            sub = [x for c, x in grp if c.meta["md"] == md and c.meta["a_longer"] == a_longer]
            assert sum(x["rc"] >= 0 for x in sub) >= 6 and sum(x["fail_row"] > 0 for x in sub) >= 6, (md, a_longer)
    # accepted pairs whose goal is not the end of the diagonal: the goal row's / column's minimum is somewhere in the band
    assert sum(x["rc"] >= 0 and x["matlen_b"] > x["len_a"] for c, x in grp) >= 20
    assert sum(x["rc"] >= 0 and x["matlen_a"] > x["len_b"] for c, x in grp) >= 20


def test_small_sizes(cases_exp):
    cs, exp = cases_exp
    small = [(c, x) for c, x in zip(cs, exp) if c.cls == "small"]
    assert {c.meta["m"] for c, _ in small} == set(ri.SMALL_M)
    for m in ri.SMALL_M:
        md = 1 + int(m * ri.R_EDGE)
        assert {c.meta["delta"] for c, _ in small if c.meta["m"] == m} == {0, 1, md, md + 5}
    for c, x in small:
        assert min(x["len_a"], x["len_b"]) == c.meta["m"] and x["max_dst"] == c.meta["md"], c.tag
        if c.meta["m"] <= 10:               # rows 1 .. 10 carry no check
            assert x["fail_row"] == 0, c.tag
        if c.meta["kind"] == "unrel":
            if c.meta["m"] == 10:
                assert x["fail_row"] == 0 and x["cost"] >= 10, c.tag
            if c.meta["m"] >= 11:           # row 11 is the first with a check: met once, failed
                assert x["rc"] == -1 and x["fail_row"] == 11, c.tag
    assert any(x["rc"] >= 0 and min(x["len_a"], x["len_b"]) >= 11 for c, x in small)
    assert any(x["rc"] == 0 for c, x in small) and any(x["len_a"] == 0 for c, x in small) and any(x["len_b"] == 0 for c, x in small)


def test_check_at_equality(oracle):
    """D(12,12) = 3 = 12 R and D(16,16) = 4 = 16 R pass; one more substitution right behind fails at rows 13 and 17.  (A
    failure AT row 12 or 16 cannot exist: rowsweep_inputs' docstring.)"""
    cs = ri.of_class("check_eq")
    assert {c.meta["name"] for c in cs} == set(ri.CHECK_SUBS) and {c.meta["shape"] for c in cs} == {"eq", "blong", "along"}
    for c in cs:
        x = oracle.align(c.a, c.b, c.R)
        row, d, fail = ri.CHECK_ROW[c.meta["name"]]
        assert float(d) == row * c.R and oracle.cell(row, row)[0] == d, c.tag
        assert x["fail_row"] == fail and (x["rc"] >= 0) == (fail == 0), c.tag
        if fail:
            assert oracle.cell(fail, fail)[0] == d + 1 == int(fail * c.R) + 1, c.tag


def test_acceptance_at_equality(oracle):
    cs = ri.of_class("accept_eq")
    eq = 0
    for c in cs:
        x = oracle.align(c.a, c.b, c.R)
        assert (x["len_b"], x["matlen_b"], x["rc"]) == (c.meta["len_b"], c.meta["matlen_b"], c.meta["rc"]), c.tag
        assert x["fail_row"] == 0 and x["cost"] > 0, c.tag
        thr = x["len_b"] * (1.0 - c.R)
        assert (x["rc"] >= 0) == (x["matlen_b"] >= thr), c.tag
        eq += x["matlen_b"] == thr
        if x["rc"] < 0:                     # the largest matlen_b the acceptance turns down
            assert x["matlen_b"] < thr <= x["matlen_b"] + 1, c.tag
    assert eq >= 4 and sum(c.meta["rc"] < 0 for c in cs) >= 4


def test_goal_ties(oracle):
    """Both named offsets hold the minimum of the goal row (column), nothing in it is lower, nothing before the first of them
    is as low, and the oracle answers the first."""
    for cls in ("tie_row", "tie_col"):
        cs = ri.of_class(cls)
        want = {(0, 1), (31, 32), (63, 64), (0, 64)} if cls == "tie_row" else {(0, 1), (9, 10), (31, 32)}
        assert {c.meta["offs"] for c in cs} == want
        for c in cs:
            x = oracle.align(c.a, c.b, c.R)
            assert x["rc"] >= 0 and x["fail_row"] == 0, c.tag
            if cls == "tie_row":
                assert x["len_a"] <= x["len_b"]
                line = [oracle.cell(x["len_a"], j)[0] for j in range(x["len_a"], x["len_b"] + 1)]
                got = x["matlen_b"] - x["len_a"]
            else:
                assert x["len_a"] > x["len_b"]
                line = [oracle.cell(i, x["len_b"])[0] for i in range(x["len_b"], x["len_a"] + 1)]
                got = x["matlen_a"] - x["len_b"]
            k0, k1 = c.meta["offs"]
            assert len(line) > k1 and line[k0] == line[k1] == min(line) == c.meta["cost"] == x["cost"], (c.tag, line)
            assert min(line[:k0], default=1 << 30) > line[k0] and got == k0, (c.tag, got)
        # each tie with the line ending right behind it and running on
        assert {c.meta["offs"] for c in cs if c.tag.endswith("tail0")} == want == {c.meta["offs"] for c in cs if c.tag.endswith("tail40")}


def test_translation_keeps_every_answer(cases_exp, oracle):
    cs, exp = cases_exp
    seen = set()
    for c, x in zip(cs, exp):
        t = c.translated()
        assert len(t.a) == len(c.a) and not set(t.a + t.b) & set(b"ACGT")
        seen |= set(t.a + t.b)
        y = oracle.align(t.a, t.b, t.R, want_ops=True)
        assert all(y[k] == x[k] for k in y if k != "ops"), c.tag
        assert y["ops"].tolist() == x["ops"].tolist(), c.tag
    assert seen == {ord("N"), ord("a"), 0x00, 0xFF}


def test_batch_of_places_every_case():
    cs = ri.of_class("small") + ri.of_class("tie_row")
    B = ri.batch_of(cs)
    assert len(B.pairs) == len(cs)
    for q, c in enumerate(cs):
        assert B.elems(q) == (c.a, c.b) and B.pairs[q][6] == (1 if c.fa else 0) | (2 if c.fb else 0), c.tag
