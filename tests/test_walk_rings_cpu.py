"""What every input of walk_ring_inputs.py is, from overlap_ref.walk_composition, the oracle and the constants of
align_bitvec.h, no GPU: the ring of the call, the row, block and position of every planted failure, the planted costs, where
the narrow sweep is given up, how many runs every stage of the walk takes, and the slot of every parked candidate.  The model
with a target range is held to Oracle.spaced_round target by target."""
import os
import re

import pytest

import align_rings as ar
import diag_collect_inputs as dc
import index_ref as ir
import overlap_ref as orf
import walk_ring_inputs as wi
from conftest import ROOT


def between(W, t, q):
    return [c for c in W["cands"] if c["t"] == t and c["q"] == q]


def equals_the_oracle_round(oracle, W):
    rows, pairs_by = orf.oracle_composition(oracle, W["texts"], W["qtexts"], W["R"], W["mask"], W["max_trial"], W["overlap_min"],
                                            oracle.text2bin, W["t_lo"], W["t_hi"])
    assert W["rows"] == rows and W["pairs_by"] == pairs_by
    assert all(W["t_lo"] <= c["t"] < W["t_hi"] and c["t"] != c["q"] for c in W["cands"])


def test_constants_restate_the_sources():
    src = open(os.path.join(ROOT, "pacbioassembly_amd", "csrc", "pba_overlap.hip")).read()
    m = re.search(r"for \(int nb : \{([\d, ]+)\}\)\s*if \(nb > pl.nb1 && nb < pl.nb2\) c.nb_mid = nb;", src)
    assert m and [int(v) for v in m.group(1).split(",")] == [nb for nb in ar.RINGS if nb < ar.MAX_NB]
    assert [(r[2], r[3]) for r in ar.plan_rows()] == list(wi.STAGE_ROWS)
    assert {row: wi.nb_mid_of(*row) for row in wi.STAGE_ROWS if wi.nb_mid_of(*row)} == {(2, 4): 3, (3, 6): 4, (4, 8): 6}
    hdr = open(ar.HDR).read()
    assert "i >= 1024 && fr == 0" in hdr and "((float)end - 4.0f * __builtin_sqrtf((float)end)) * (float)m > (float)i * (float)bail_w" in hdr


# ----------------------------------------------------------------------------- A
def test_collect_inputs_cover_every_block_edge():
    """the (superblock, block, position) of every failing row, from the ring's geometry alone"""
    for NB in wi.COLLECT_NBS:
        RB = 32 * NB
        rows = sorted(f for R, fs in wi.collect_groups(NB) for f in fs)
        assert rows == wi.collect_rows(NB) and all(dc.can_fail_first(f, R) for R, fs in wi.collect_groups(NB) for f in fs)
        got = {((f - 1) // RB, ((f - 1) % RB) >> 5, (f - 1) % 32 + 1) for f in rows}
        sbs = wi.RING6_SUPERBLOCKS if NB == 6 else dc.SUPERBLOCKS[NB]
        assert got == {(s, b, p) for s in sbs for b in range(NB) for p in dc.POS if s * RB + 32 * b + p > 64}
        assert {b for _, b, _ in got} == set(range(NB)) and min(rows) > 64
        planted = [(p["f"], p["m"] == p["f"]) for g in range(len(wi.collect_groups(NB))) for p in wi.collect_set(NB, g)["planted"] if p["kind"] == "fail"]
        assert sorted(planted) == sorted((f, last) for f in rows for last in (True, False))


@pytest.mark.parametrize("case", wi.COLLECT_CASES, ids=lambda c: f"ring{c[0]}.{c[1]}")
def test_collect_pairs_are_what_they_are_named_for(oracle, case):
    NB, g = case
    C = wi.collect_set(NB, g)
    W = wi.model(oracle, C)
    R, md = C["R"], wi.call_md(C)
    assert (ar.nb1(md), ar.nb2(md)) == wi.ROW_OF_RING[NB] and (NB == 1 or md == ar.row_of(*wi.ROW_OF_RING[NB])[0])
    assert C["t_hi"] == len(C["texts"]) - (NB >= 2) and max(len(t) for t in C["texts"][:C["t_hi"]]) <= 12000
    a_rows = set()
    for p in C["planted"]:
        for t, q in ((p["x"], p["y"]), (p["y"], p["x"])):
            cs = between(W, t, q)
            head = cs[0]
            assert (head["jd"], head["p"], head["tried"], head["pre"]) == (0, 0, True, False), (p, t, q)
            x = head["x"]
            assert min(x["len_a"], x["len_b"]) == p["m"] and x["max_dst"] <= ar.bv_pass1_w(x["max_dst"], NB)   # its window is its band
            a_rows.add(x["len_a"] > x["len_b"])
            if p["kind"] == "fail":
                assert x["rc"] == -1 and x["fail_row"] == p["f"] and not head["ok"], (p, x)
            else:
                assert head["ok"] and x["matlen_a"] >= wi.COLLECT_MIN, (p, x)
            # what the tails did: the copy's tail is unrelated, the read's own last 16 bases are the copy's where the pair
            # is clean behind the failing row -- a backward candidate of (copy, read), which the model decides
            back = [c for c in cs[1:]]
            assert all(c["jd"] == 1 for c in back) and len(back) <= 1
            xt, yt, m = W["texts"][p["x"]], W["texts"][p["y"]], p["m"]
            same_tail = int(ir.np_keys(xt[m - 16:])[0]) & W["mask"] == int(ir.np_keys(yt[m - 16:m])[0]) & W["mask"]
            assert bool(back) == (t == p["y"] and same_tail), (p, t, q, back)
            assert p["kind"] == "true" or same_tail == (m > p["f"])
        if p["kind"] == "true":
            a, b = orf.sides(W["texts"][p["x"]], W["texts"][p["y"]], 0, 0)
            assert oracle.align(a, b, R)["rc"] >= 0 and dc.touches_bound(oracle, a, b, p["m"], R, 32 * NB), p
    assert a_rows == {False, True}
    assert g != 0 or len([p for p in C["planted"] if p["kind"] == "true"]) >= 3
    equals_the_oracle_round(oracle, W)
    st = wi.stages(W)
    assert st["launches"] == [(NB, "first", len(wi.items_of(W)))] and st["parked"] == 0 and st["rows"] == sorted(W["rows"])


# ----------------------------------------------------------------------------- B
def stage_expectation(W, env):
    """must_redo-style arithmetic: the launches of a plan row's call from the planted costs alone (every planted read is an
    item of its own: one candidate per target)"""
    row, R, L = W["row"], W["R"], W["L"]
    md = ar.max_dst_of(L, L, R)
    mid = wi.nb_mid_of(*row)
    w1, w_mid = ar.bv_pass1_w(md, row[0]), ar.bv_pass1_w(md, mid) if mid else 0
    costs = wi.planted_costs(row)
    n_up = sum(k.startswith("given_up") for k in W["long"])
    n_items = len(wi.items_of(W))
    over1 = sum(c > w1 for c in costs.values()) + n_up              # parked by a first launch in the narrow ring
    over_mid = sum(c > w_mid for c in costs.values())                # parked by the middle ring (it fails the given-up pairs)
    out = []
    if env == "wide":
        if mid:
            out = [(mid, "first", n_items)] + ([(row[1], "redo_band", over_mid)] if over_mid else [])
            return out, over_mid
        return [(row[1], "band", n_items)], 0
    assert env is None
    out = [(row[0], "first", n_items)]
    if over1 and mid:
        out.append((mid, "redo", over1))
        if over_mid:
            out.append((row[1], "redo_band", over_mid))
    elif over1:
        out.append((row[1], "redo_band", over1))
    return out, over1


@pytest.mark.parametrize("row", list(wi.STAGE_ROWS), ids=str)
def test_stage_sets_are_in_their_row_and_park_where_planted(oracle, row):
    C = wi.stage_set(row)
    W = wi.model(oracle, C)
    R, L = C["R"], C["L"]
    md = wi.call_md(C)
    lo, hi = ar.row_of(*row)
    assert lo <= md <= hi and (ar.nb1(md), ar.nb2(md)) == row and md == ar.max_dst_of(L, L, R) and L <= 12000
    mid = wi.nb_mid_of(*row)
    w1 = ar.bv_pass1_w(md, row[0])
    w_mid = ar.bv_pass1_w(md, mid) if mid else 0
    costs = wi.planted_costs(row)
    near_budget = 0
    for name, (tx, qy) in C["long"].items():
        cs = [c for c in W["cands"] if c["t"] == tx]
        assert [(c["q"], c["jd"], c["p"], c["pre"], c["tried"]) for c in cs] == [(qy, 0, 0, False, True)], name   # its copy's head probe, nothing else
        assert not [c for c in W["cands"] if c["q"] == qy and c["t"] != tx]
        x = cs[0]["x"]
        xt, yt = W["texts"][tx], W["texts"][qy]
        assert (x["len_a"], x["len_b"], x["max_dst"]) == (L, L, md)
        planted = [sum(a != b for a, b in zip(xt[:i], yt[:i])) for i in sorted(x["diag"])]
        assert [x["diag"][i] for i in sorted(x["diag"])] == planted, name             # the diagonal carries the planted count, row by row
        if name.startswith("given_up"):
            assert x["rc"] == -1 and x["fail_row"] == 1601 and x["diag"][1600] == 1600 - wi.STAGE_HEAD
            assert 1024 in wi.gives_up(x["diag"], L, w1, 1600, margin=1.05)           # given up at row 1 024, with 5 % to spare
            assert wi.outcome(cs[0], row[0], False, R) == "park"
            nxt, full = (mid, False) if mid else (row[1], True)
            if mid:                                                                    # the middle ring is not, and certifies the failure
                assert wi.gives_up(x["diag"], L, w_mid, 1600, margin=0.98) == [] and 1601 * R < 2 * ar.bv_pass1_wl(md, mid) + 2
            assert wi.outcome(cs[0], nxt, full, R) == "no"
            continue
        near_budget += 1
        assert (L + 1) * (2 * md + 1) <= ar.ORACLE_CELL_BUDGET
        assert cs[0]["ok"] and x["cost"] == costs[name] == planted[-1] and x["matlen_a"] == L, (name, x["cost"])
        # never given up where it is to be certified: the condition fails by 2 % at every row it is looked at (float32
        # rounds at 1e-7; the four standard deviations are 4.4 % of the densest pair's count)
        if name == "w1" and w1 < md:
            assert wi.gives_up(x["diag"], L, w1, L, margin=0.98) == []
        if name in ("w1+1", "w_mid") and mid and w_mid < md:
            assert wi.gives_up(x["diag"], L, w_mid, L, margin=0.98) == []
        want = ["ok" if costs[name] <= w1 else "park"] + (["ok" if costs[name] <= w_mid else "park"] if mid else []) + ["ok"]
        got = [wi.outcome(cs[0], row[0], False, R)] + ([wi.outcome(cs[0], mid, False, R)] if mid else []) + [wi.outcome(cs[0], row[1], True, R)]
        assert got == want, name
    assert near_budget <= 8
    assert row == (6, 8) or costs["w1"] <= w1
    if row == (6, 8):
        assert not costs and len(C["long"]) == 2
    else:
        assert ("w1+1" in costs) == (w1 < md - 1) and ("w_mid" in costs) == ("w_mid+1" in costs) == bool(mid)
    if row == (6, 8):
        assert (ar.row_of(6, 8)[0] - 1) / 0.9999 * (2 * ar.row_of(6, 8)[0] + 1) > ar.ORACLE_CELL_BUDGET      # no accepted pair of this row fits
    for tx, qy in C["short"]:                                                         # never leave the first launch
        for c in between(W, tx, qy) + between(W, qy, tx):
            assert c["x"]["max_dst"] <= 600 and wi.outcome(c, row[0], False, R) in ("ok", "no")
    assert sum(c["ok"] for tx, qy in C["short"] for c in between(W, tx, qy)) >= 3
    if row[1] <= 3:
        equals_the_oracle_round(oracle, W)
    for env in (None, "wide"):
        st = wi.stages(W, env)
        want, parked = stage_expectation(W, env)
        assert st["launches"] == want and st["parked"] == parked and st["rows"] == sorted(W["rows"]), (env, st["launches"], want)
        assert st["wide_first"] == (env == "wide")
    st = wi.stages(W, "sample")                                                        # one item sampled, the rest decided by it
    first = wi.items_of(W)[0][0]
    name = [k for k, v in C["long"].items() if v[0] == first][0]
    assert st["launches"][0] == (row[0], "first", 1) and st["rows"] == sorted(W["rows"])
    assert st["wide_first"] == int(name.startswith("given_up") or costs.get(name, 0) > w1)
    assert st["parked"] >= stage_expectation(W, "wide")[1] and (name == "w1+1") == (row in wi.PARKS_FIRST)
    if row in wi.PARKS_FIRST:                                                         # ... the rest starts in the middle ring
        assert st["launches"][:3] == [(row[0], "first", 1), (mid, "redo", 1), (mid, "first", len(wi.items_of(W)) - 1)]


def test_stage_sets_cover_every_ring_in_every_form(oracle):
    """first launch in rings 1, 2, 3, 4, 6; resumed runs short of the band in 3, 4, 6 and at the band in 2, 3, 4, 6, 8; the
    first-launch form at the band in 2, 4 and 8 at the least; a run parked twice in every row with a middle ring"""
    seen = {}
    for row in wi.STAGE_ROWS:
        W = wi.model(oracle, wi.stage_set(row))
        for env in (None, "wide", "sample"):
            launches = wi.stages(W, env)["launches"]
            for nb, form, n in launches:
                seen.setdefault(form, set()).add(nb)
            if env is None and wi.nb_mid_of(*row):
                assert [f for _, f, _ in launches] == ["first", "redo", "redo_band"]
    assert seen["first"] >= {1, 2, 3, 4, 6} and seen["redo"] == {3, 4, 6} and seen["redo_band"] == {2, 3, 4, 6, 8}
    assert seen["band"] >= {2, 4, 8}


@pytest.mark.parametrize("row", wi.RC_ROWS, ids=str)
def test_stage_sets_on_the_other_strand(oracle, row):
    """the reverse-complement pass over the set with its queries flipped aligns the designed bases: same planted runs"""
    C = wi.stage_set(row)
    W, V = wi.model(oracle, C), wi.model(oracle, C, "rc")
    long = {tx for tx, _ in C["long"].values()}
    assert [r for r in V["rows"] if r[0] in long] == [r for r in W["rows"] if r[0] in long] and len(long) == 5
    launches = wi.stages(V)["launches"]
    assert [(nb, f) for nb, f, _ in launches] == [(row[0], "first"), (wi.nb_mid_of(*row), "redo"), (row[1], "redo_band")]
    assert [n for _, _, n in launches[1:]] == [n for _, _, n in wi.stages(W)["launches"][1:]]


# ----------------------------------------------------------------------------- C
PARK_SLOTS = {"slot0": [0], "slot63": [63], "slot64": [64], "straddle": [64], "second_narrow": [63], "two_in_item": [10, 40]}


@pytest.mark.parametrize("view", ["forward", "rc"])
@pytest.mark.parametrize("name", wi.PARK_CASES)
def test_parked_candidates_sit_where_they_are_named_for(oracle, name, view):
    C = wi.parked_set(name)
    W = wi.model(oracle, C, view)
    R, md = C["R"], wi.call_md(C)
    assert (ar.nb1(md), ar.nb2(md)) == (1, 2) and wi.nb_mid_of(1, 2) == 0 and (C["t_lo"], C["t_hi"]) == (0, 1)
    if name in ("slot0", "straddle"):
        equals_the_oracle_round(oracle, W)
    L = wi.listed(W)[0]
    assert len(L) == W["n_listed"] and len(wi.items_of(W)) == (len(L) + 63) // 64
    parks = [s for s, c in enumerate(L) if c["tried"] and wi.outcome(c, 1, False, R) == "park"]
    assert parks == PARK_SLOTS[name] and [L[s]["q"] for s in parks] == C["parked"]
    for s in parks:
        x = L[s]["x"]
        assert L[s]["ok"] and L[s]["tried"] and x["cost"] == wi.park_cost() + parks.index(s) > ar.bv_pass1_w(x["max_dst"], 1)
        assert x["cost"] == sum(a != b for a, b in zip(*orf.sides(W["texts"][0], W["qtexts"][L[s]["q"]], L[s]["jd"], L[s]["p"])))
        assert wi.outcome(L[s], 2, True, R) == "ok"
    # the short queries: runs of one (with two trials: of two, the second never tried), every one a success in the narrow ring
    others = [c for c in L if c["q"] not in C["parked"]]
    per_q = {}
    for c in others:
        per_q.setdefault(c["q"], []).append(c)
    assert all(cs[0]["ok"] and cs[0]["tried"] and not any(c["tried"] for c in cs[1:]) for cs in per_q.values())
    assert {len(cs) for cs in per_q.values()} == ({1, 2} if name == "straddle" else {1})
    assert [c["q"] for c in L] == sorted(c["q"] for c in L)                            # slots in query order
    if name == "slot63":                                                              # directly followed by a run that succeeds narrowly
        assert L[64]["q"] != L[63]["q"] and wi.outcome(L[64], 1, False, R) == "ok" and L[64]["tried"]
    if name == "straddle":                                                            # slot 63: the run's first candidate, 20 rows, decided,
        a, b = L[63], L[64]                                                           # no success; the parked one is past the item's end
        assert a["q"] == b["q"] and (a["jd"], b["jd"]) == (0, 2) and a["tried"] and not a["ok"] and min(a["x"]["len_a"], a["x"]["len_b"]) == 20
        assert wi.outcome(a, 1, False, R) == "no" and W["pairs_by"][(0, a["q"])] == 2
    if name == "second_narrow":                                                       # the candidate behind the parked one would succeed
        a, b = L[63], L[64]                                                           # in the narrow ring, and is never tried
        assert a["q"] == b["q"] and b["ok"] and wi.outcome(b, 1, False, R) == "ok" and not b["tried"] and W["pairs_by"][(0, a["q"])] == 1
        assert [r[4] for r in W["rows"] if r[1] == a["q"]] == [0]
    st = wi.stages(W)
    n_items = (len(L) + 63) // 64
    assert st["launches"] == [(1, "first", n_items), (2, "redo_band", len(parks))] and st["parked"] == len(parks)
    assert st["rows"] == sorted(W["rows"]) and n_items == (2 if len(L) > 64 else 1)
    if name == "two_in_item":
        assert n_items == 1
