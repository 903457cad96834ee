"""What every input of overlap_edge_inputs.py is, from overlap_ref.py (a plain model of the all-vs-all loop), index_ref.py and the
oracle, no GPU: the model equals Oracle.spaced_round target by target on every input (rows, j, pairs per query) and
prefilter_inputs' one-trial enumerator on that file's cases; every input holds exact copies of probe windows and no chance hit;
and every edge test_gpu_overlap_edges.py is there to reach -- the shape of a round's run lists, the bucket sizes, the positions on
either side of the head / tail order, what lies behind a success, the census that misses -- is asserted present."""
import os
import re

import pytest

import align_rings as ar
import index_ref as ir
import overlap_edge_inputs as oi
import overlap_ref as orf
import prefilter_inputs as pi
from conftest import MASK_PAT, ROOT

PATS = (MASK_PAT, pi.HEAVY_PAT)


def on(W, name, q=None):
    t = W["S"].idx[name]
    return [c for c in W["cands"] if c["t"] == t and (q is None or c["q"] == q)]


def table(W):
    return orf.ProbeTable(W["qtexts"], W["mask"], W["max_trial"])


def test_mask_and_rounds_restate_the_sources(oracle):
    for pat in (MASK_PAT, pi.HEAVY_PAT, pi.ALT_PAT):
        assert orf.mask_of(pat) == oracle.mask_from_pattern(pat)
    assert orf.hashed(orf.mask_of(pi.HEAVY_PAT)) and not orf.hashed(orf.mask_of(MASK_PAT))
    src = open(os.path.join(ROOT, "pacbioassembly_amd", "csrc", "overlap.h")).read()
    for name, v in (("PBA_OVL_PPT", orf.PPT), ("PBA_OVL_HALF", orf.HALF), ("PBA_OVL_WAVES", orf.WAVES), ("PBA_PT_MAX_BITS", orf.PT_MAX_BITS)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == v
    # the walk of k_ovl_scan, thread by thread: chunk c = 256 st + x, 16 positions, halves of 8, wavefronts of 64 threads
    for tlen in (17, 200, 4185, 4112, 9000):
        seen = {}
        steps = (orf.n_chunks(tlen) + 255) // 256
        for st in range(steps):
            for x in range(256):
                c = st * 256 + x
                if c < orf.n_chunks(tlen):
                    for k in range(16):
                        seen[16 * c + k] = (st, x // 64, k // 8)
        assert set(range(tlen - 16)) <= set(seen) and max(seen) < tlen + 15
        assert all(orf.round_of(p) == r for p, r in seen.items())


@pytest.mark.parametrize("which", ["overlap_case", "straddle_forward", "straddle_rc"])
def test_model_reproduces_the_one_trial_enumerator(oracle, which):
    if which == "overlap_case":
        texts = qtexts = pi.overlap_case(0.30, MASK_PAT)[0]
    else:
        texts, qtexts = pi.straddle_views(0.30)[0][which.split("_")[1]]
    mask = orf.mask_of(MASK_PAT)
    old_c, old_match = pi.overlap_candidates(texts, MASK_PAT, pi.OVL_MIN, qtexts)
    new_c, new_match = orf.candidates(texts, qtexts, mask, 1, pi.OVL_MIN)
    assert new_match == old_match and sorted((t, q, not (jd & 1), p) for t, q, jd, _, p in new_c) == sorted(c[:4] for c in old_c)
    old = pi.walk_composition(oracle, texts, qtexts, 0.30)
    new = orf.walk_composition(oracle, texts, qtexts, 0.30, mask, 1, pi.OVL_MIN)
    assert [r[:2] + r[3:] for r in new["rows"]] == old["rows"] and not any(r[2] for r in new["rows"])
    assert (new["pairs"], new["n_match"], new["n_pre"], new["n_listed"]) == (old["pairs"], old["n_match"], old["n_pre"], old["n_listed"])
    listed = [(c["t"], c["q"], not (c["jd"] & 1), c["p"]) for c in new["cands"] if not c["pre"]]
    assert listed == [(t, c["q"], c["fwd"], c["p"]) for t in sorted(old["slices"]) for c in old["slices"][t]]


@pytest.mark.parametrize("case,view", [(c, "forward") for c in oi.CASES + [("census",)]] + [(c, "rc") for c in oi.VIEW_CASES],
                         ids=lambda v: v if isinstance(v, str) else oi.case_id(v))
def test_model_equals_the_oracle_round_by_round(oracle, case, view):
    """rows (with j), and the pairs tried per (target, query), of the locked spaced_seed round of every target; and no chance
    hit in any input, under the trial count and in the view it is run in"""
    W = oi.expected(oracle, case, view)
    assert oi.is_clean(W["texts"], W["qtexts"], W["mask"], W["max_trial"], W["overlap_min"])
    rows, pairs_by = orf.oracle_composition(oracle, W["texts"], W["qtexts"], W["R"], W["mask"], W["max_trial"], W["overlap_min"], oracle.text2bin)
    assert W["rows"] == rows
    assert W["pairs_by"] == pairs_by
    assert len(orf.probe_entries(W["qtexts"], W["mask"], W["max_trial"])) == W["n_probe_entries"]


@pytest.mark.parametrize("case", oi.SHORT_CASES, ids=oi.case_id)
def test_short_masks_model_equals_the_oracle_on_either_side_of_the_small_scan(oracle, case):
    """masks of six and seven care bases: a direct-address probe table of 4 096 buckets (scanned by one workgroup) and of 16 384
    (tiled); chance hits everywhere, overlaps found, and the model is still the oracle's round target by target"""
    small_max = ir.define("PBA_SCAN_SMALL_MAX", "seed_index.h")
    W = oi.expected(oracle, case)
    buckets = 1 << bin(W["mask"]).count("1")
    assert W["mask"] == oracle.mask_from_pattern(case[1]) and not orf.hashed(W["mask"])
    assert (buckets <= small_max) == (case == oi.SHORT_CASES[0]) and [2 * p.count("1") for p in oi.SHORT_PATS] == [12, 14]
    rows, pairs_by = orf.oracle_composition(oracle, W["texts"], W["qtexts"], W["R"], W["mask"], W["max_trial"], W["overlap_min"], oracle.text2bin)
    assert W["rows"] == rows and W["pairs_by"] == pairs_by
    assert len(rows) >= 20 and not oi.is_clean(W["texts"], W["qtexts"], W["mask"], W["max_trial"], W["overlap_min"])
    assert W["n_pre"] > 0 and W["n_listed"] > len(rows) and W["n_probe_entries"] > 60


# ----------------------------------------------------------------------------- the run lists
@pytest.mark.parametrize("pat", PATS)
def test_bucket_sizes(oracle, pat):
    sizes = []
    for name in ("b_small", "b128", "b200", "b520"):
        W = oi.expected(oracle, ("run", name, pat))
        tab = table(W)
        for N in oi.BUCKETS[name]:
            T = W["texts"][W["S"].idx[f"b{N}"]]
            assert orf.rounds(T, tab) == {(0, 0, 1): [(40, N)]}                       # one run of N: R = 1, Tot = N
            c = on(W, f"b{N}")
            assert len(c) == N and {x["p"] for x in c} == {40} and len({x["q"] for x in c}) == N
            assert sum(not x["pre"] for x in c) >= min(N, 3) and sum(x["ok"] for x in c) >= min(N, 3)
            sizes.append(N)
            if N < 512:                                                               # ... and every member holds the bucket at its head,
                m = c[0]["q"]                                                         # its own entry inside the run
                assert orf.rounds(W["texts"][m], tab)[(0, 0, 0)][0] == (0, N)
                assert len([x for x in W["cands"] if x["t"] == m and x["p"] == 0]) == N - 1
    assert sizes == [1, 63, 64, 65, 128, 129, 200, 520]


@pytest.mark.parametrize("pat", PATS)
def test_round_shapes(oracle, pat):
    W = oi.expected(oracle, ("run", "shapes", pat))
    tab = table(W)
    shape = {}
    for name, runs in oi.SHAPES.items():
        r = orf.rounds(W["texts"][W["S"].idx[name]], tab)
        assert r == {(0, 0, 0): runs}, name
        shape[name] = (len(runs), orf.run_starts(runs))
        assert [(c["p"]) for c in on(W, name)].count(runs[-1][0]) == runs[-1][1]
    assert shape["r64_5"] == (2, [0, 64, 69])                    # a run starts at slot 64 behind one long run
    assert shape["r60_4_5"] == (3, [0, 60, 64, 69])              # a run ends at slot 63, the next starts at 64
    assert shape["ones64_5"][1][:66] == list(range(65)) + [69]   # ... behind 64 runs of one
    assert shape["ones65"] == (65, list(range(66)))              # Tot = 65: one slot in the second iteration
    assert shape["tot_small"] == (3, [0, 3, 4, 6])               # Tot < 64: 58 lanes without a slot
    W64 = oi.expected(oracle, ("run", "b_small", pat))
    assert orf.rounds(W64["texts"][W64["S"].idx["b64"]], table(W64)) == {(0, 0, 1): [(40, 64)]}       # Tot = 64 exactly
    W200 = oi.expected(oracle, ("run", "b200", pat))
    assert orf.rounds(W200["texts"][W200["S"].idx["b200"]], table(W200)) == {(0, 0, 1): [(40, 200)]}  # one run of 200


@pytest.mark.parametrize("pat", PATS)
def test_slot_groups_and_full_round(oracle, pat):
    W = oi.expected(oracle, ("run", "groups", pat))
    S = W["S"]
    assert orf.rounds(W["texts"][S.idx["groups"]], table(W)) == {(0, 0, 0): [(p, 1) for p in oi.GROUP_POS]} and len(oi.GROUP_POS) == 192
    by_q = {c["q"]: c for c in on(W, "groups")}
    assert len(by_q) == len(on(W, "groups")) == 192
    for q, (s, p) in S.facts.items():
        assert by_q[q]["p"] == p and by_q[q]["jd"] == s % 2                          # slot s: forward and backward alternate
        if s % 64 in oi.GROUP_LANES:
            assert not by_q[q]["pre"], s                                              # a survivor at lanes 0, 31, 32, 63 of every group
    assert sum(c["pre"] for c in by_q.values()) >= 100
    W = oi.expected(oracle, ("run", "full", pat))
    r = orf.rounds(W["texts"][W["S"].idx["full"]], table(W))
    assert r[(0, 0, 1)] == [(p, 1) for p in oi.FULL_POS] and len(oi.FULL_POS) == 512       # every position of the round
    assert (len(r[(0, 0, 0)]), len(r[(0, 1, 0)])) == (496, 16) and len(r) == 3            # (the tails: half 0 from lane 2 on, into wavefront 1)
    assert len(on(W, "full")) == 1024 and all(c["ok"] for c in on(W, "full"))


@pytest.mark.parametrize("pat", PATS)
def test_layout_last_window_short_reads_own_probes_and_collision(oracle, pat):
    W = oi.expected(oracle, ("run", "misc", pat))
    S, tab = W["S"], table(W)
    # layout
    T = W["texts"][S.idx["layout"]]
    r = orf.rounds(T, tab)
    assert set(r) == {(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 2, 1), (0, 3, 0), (1, 0, 0)}
    assert len(T) > 4096 and orf.n_chunks(len(T)) == 261 and oi.LAYOUT_LAST >> 4 == 260 and oi.LAYOUT_LAST <= len(T) - 17
    assert [r[(0, 0, 0)], r[(0, 0, 1)]] == [[(p, 1)] for p in oi.LAYOUT_LANE] and len({p >> 4 for p in oi.LAYOUT_LANE}) == 1   # both halves of one lane
    assert r[(1, 0, 0)] == [(oi.LAYOUT_POS[-1], 3), (oi.LAYOUT_LAST, 2)]
    assert sorted({c["p"] for c in on(W, "layout")}) == sorted(oi.LAYOUT_POS + oi.LAYOUT_LANE + [oi.LAYOUT_LAST])
    # the last window
    for m in oi.LAST_MODS:
        L = 160 + m
        assert len(W["texts"][S.idx[f"last16_{m}"]]) == L and L % 16 == m
        assert on(W, f"last16_{m}") == [] and on(W, f"cut_{m}") == [] and on(W, f"cutnext_{m}") == []
        c17 = on(W, f"last17_{m}")                                                     # the two members; and last16's own backward probe,
        assert [c["p"] for c in c17] == [L - 17] * 3 and S.idx[f"last16_{m}"] in {c["q"] for c in c17 if c["jd"] == 1}   # which IS that window
        a, b = W["texts"][S.idx[f"cut_{m}"]], W["texts"][S.idx[f"cutnext_{m}"]]
        assert (a[-9:] + b[:7]) == W["texts"][S.idx[f"last16_{m}"]][-16:]              # the window continues in the next read
    # short reads
    assert [len(W["texts"][S.idx[f"short{L}"]]) for L in oi.SHORT_LENS] == list(oi.SHORT_LENS)
    gated, _ = orf.candidates(W["texts"], W["qtexts"], W["mask"], 1, 0)
    every = {(t, q) for t, q, *_ in gated}
    st = S.idx["short_t"]
    for L in oi.SHORT_LENS:
        i = S.idx[f"short{L}"]
        assert ((st, i) in every) == (L >= 16) and bool(on(W, "short_t", i)) == (L >= oi.RUN_MIN)      # matched from 16, past the gate from 20
        assert bool(on(W, f"short{L}")) == (L >= 17)                                                    # a target of 17 visits position 0
    # the target's own probes
    t, twin = S.idx["own_t"], S.idx["own_twin"]
    assert orf.rounds(W["texts"][t], tab)[(0, 0, 0)] == [(0, 5), (80, 5)]             # 3 members, the twin, the target itself
    assert len(on(W, "own_t")) == 2 * 4 and W["texts"][t] == W["texts"][twin]         # never the target itself
    assert [r for r in W["rows"] if r[:2] == (t, twin)] == [(t, twin, 0, 1, 0, 0, 200, 200)]
    # two keys, one bucket of the hashed table
    w1, w2 = S.facts["collide"]
    k1, k2 = (int(ir.np_keys(w)[0]) & orf.mask_of(pi.HEAVY_PAT) for w in (w1, w2))
    assert k1 != k2 and orf.bucket_of(k1, orf.mask_of(pi.HEAVY_PAT)) == orf.bucket_of(k2, orf.mask_of(pi.HEAVY_PAT))
    want = [(40, 5), (104, 5)] if pat == pi.HEAVY_PAT else [(40, 3), (104, 2)]
    assert orf.rounds(W["texts"][S.idx["col_t"]], tab) == {(0, 0, 1): want}
    assert sorted(c["p"] for c in on(W, "col_t")) == [40] * 3 + [104] * 2


# ----------------------------------------------------------------------------- head and tail
def test_head_tail_positions(oracle):
    cap = int(re.search(r"kRowSweepLdsCap = (\d+) \* 1024", open(os.path.join(ROOT, "pacbioassembly_amd", "csrc", "pba_host.h")).read()).group(1)) * 1024
    seen = set()
    for L in oi.HT_LENS:
        W = oi.expected(oracle, ("ht", L))
        S = W["S"]
        md = 1 + int(max(len(t) for t in W["texts"]) * oi.HT_R)
        assert oi.HT_R in pi.RS and ar.bitvec_supports(md) and ((2 * md + 1) * 2 + 15) // 16 * 16 <= cap         # both plans accept it
        nh, lo, top = oi.head_tail(L)
        order, _ = ir.visit_order(L, "head_tail")
        assert list(order) == list(range(nh)) + list(range(top, lo - 1, -1))
        visited = set(order.tolist())
        T = S.idx["T"]
        for p, (qf, qb) in S.facts["q"].items():
            f, b = on(W, "T", qf), on(W, "T", qb)
            assert bool([c for c in b if c["p"] == p]) == (p in visited), (L, p)
            assert bool([c for c in f if c["p"] == p]) == (p in visited and L - p >= oi.HT_MIN), (L, p)
            if p in visited:
                assert (T, qb, 0, -1, p) in [r[:5] for r in W["rows"]]                  # backward from p + 15, wherever p lies
            seen.add(("head" if p < nh else "tail" if lo <= p <= top else "gap", p in visited, p == L - 16))
        assert on(W, "next") == [] and not [c for c in W["cands"] if c["q"] == S.idx["next"]]
        od = oi.ht_order(L)
        if od:
            a, b = ([c for c in on(W, "T", S.facts[k]) if c["jd"] == 0] for k in ("qa", "qb"))
            assert [c["p"] for c in a] == od["a"][:2] + od["a"][:1:-1] and [c["p"] for c in b] == od["b"][:2] + od["b"][:1:-1]
            assert [c["ok"] for c in a] == [True] * 4 and [c["ok"] for c in b] == [False, False, True, True]
            assert [r[4] for r in W["rows"] if r[:2] in ((T, S.facts["qa"]), (T, S.facts["qb"]))] == [od["a"][0], od["b"][3]]
    # visited head and tail positions, the gap, and len - 16 both ways: not visited in a short read, visited as tail_top
    assert {("head", True, False), ("tail", True, False), ("tail", True, True), ("gap", False, False), ("gap", False, True)} <= seen
    assert [oi.head_tail(L)[1:] for L in (20017, 40016, 40017)] == [(20001, 20001), (20001, 40000), (20002, 40001)]


# ----------------------------------------------------------------------------- behind a success
def test_after_count_situations(oracle):
    seen = set()
    for name in oi.AFTER_SETS:
        for mt in oi.AFTER_TRIALS:
            for om in oi.AFTER_MINS:
                W = oi.expected(oracle, ("after", name, mt, om))
                sit = oi.after_situations(W, W["qtexts"], W["mask"], mt, om)
                named = {W["S"].idx.get(k): k for k in W["S"].idx}
                for (t, q), names in sit.items():
                    seen |= {(n, mt) for n in names}
                    if named.get(q) == "own_first":
                        assert "own_key_head_and_tail_behind" in names and "first" in names
                    if named.get(q) == "own_second":
                        assert "own_key_before" in names
                behind = sum(not c["tried"] for c in W["cands"])
                assert behind == W["n_gate"] - W["pairs"] and (behind > 0 or mt == 1)
    assert {n for n, _ in seen} == oi.AFTER_NAMES
    for n in ("nonexistent_past_gate", "zero_key", "gate_minus_1", "own_key_repeats", "multiplicity_3"):
        assert {mt for k, mt in seen if k == n} & {33, 63}, n                         # ... where t2 = 66 or 126: the second ballot round
    assert {mt for k, mt in seen if k == "last"} == {1} and (("middle", 63) in seen)


# ----------------------------------------------------------------------------- the census that misses
def test_census_misses_the_dense_target(oracle):
    W = oi.expected(oracle, ("census",))
    n = len(W["texts"])
    n_s = min(n, max(64, n // 16))
    assert n == oi.CENSUS_READS >= 1024 and n // n_s == 16                            # ovl_size_fused: every 16th target is sampled
    per_t = {}
    for c in W["cands"]:
        per_t.setdefault(c["t"], []).append(c)
    assert not any(t % 16 == 0 for t in per_t)                                        # no sampled target has a candidate
    room = 0 + 0 // 2 + 64                                                            # the sample's largest need, half as much again, + 64
    assert sum(not c["pre"] for c in per_t[oi.CENSUS_TARGET]) >= 70 > room
