"""The planted inputs of cons_round_inputs.py are what they are named for -- shown on the serial oracle alone (no GPU):
the rows of a pool and of its reversal differ where meta says, the flip reads are found or not as named, the chains need
their three steps, the threshold trio sits at thr - 1, thr, thr + 1 by the oracle's own clip, the vote cases leave
contested boxes at the seam, the hit lists are as long as named, and no probe that ss_try's first gate skips would have hit.

must_rewalk() is the sequential restatement the GPU suite takes its bounds on the round's stats from: which reads of a
pool cannot keep a row computed against the round's first text.  It is pinned here against the oracle's extents."""
import ctypes as C

import numpy as np
import pytest

import cons_round_inputs as ci

COLS = ("read", "found", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b", "n_trials", "n_pairs")
DUMP_CAP = 40000

_CACHE = {}


def oracle_round(oracle, case, pool=None):
    """The serial oracle on a case: dict(rows, ext, sel, sup, tot, text, evolved, rows2, ext2, sel2, sup2, tot2, text2,
    evolved2) -- one round over case.pool, evolve, a second round over meta['pool2'], evolve.  Computed once per case."""
    key = (case.meta["name"], tuple(pool if pool is not None else case.pool))
    if key in _CACHE:
        return _CACHE[key]
    mask = oracle.mask_from_pattern(ci.PATTERN)
    file, offs = ci.records(case.reads)
    oc = oracle.consensus(case.text, case.weight, overlap_min=case.overlap_min)
    out = {}
    for tag, pl in (("", pool if pool is not None else case.pool), ("2", case.meta["pool2"])):
        rows, nm = oc.round(mask, ci.R, case.max_trial, file, offs, pl, buggy=False)
        sel, sup, tot, ext = oc.dump(DUMP_CAP)
        assert nm == int(rows["found"].sum())
        out.update({"rows" + tag: rows, "ext" + tag: ext, "sel" + tag: sel, "sup" + tag: sup, "tot" + tag: tot,
                    "text" + tag: oc.text(DUMP_CAP)})
        oc.evolve()
        out["evolved" + tag] = oc.text(DUMP_CAP)
    _CACHE[key] = out
    return out


def must_rewalk(case, rows, pool=None, text_len=None):
    """Walk the oracle's rows in pool order, keeping the extent as ref_seq::try_align grows it (ref_seq.h:268-275).
    A found read must be re-walked when an earlier pool read has grown the end its candidate's accessor runs to while
    that accessor was shorter than thr = s_len + 1 + int(s_len * R): its clipped len_a (seq_aligner.h:94-102) then depends
    on the growth.  (An accessor only gets longer, so it is shortest against the round's first text.)  Returns
    dict(n_rewalk, depth, ext, n_grown_fwd, n_grown_bwd): depth is the longest chain of such dependencies, counted in
    batches, since a growth is applied only after its batch."""
    pool = case.pool if pool is None else pool
    ln = len(case.text) if text_len is None else text_len
    pre, post = 0, ln
    growers = {1: [], -1: []}          # (accessor end before the growth is irrelevant: depth only)
    n_rewalk, depth, nf, nb = 0, 1 if len(pool) else 0, 0, 0
    for k, r in enumerate(pool):
        w = rows[k]
        if not w["found"]:
            continue
        d = int(w["dir"])
        s_len = len(case.reads[r]) - int(w["j"])
        thr = ci.thr_of(s_len, case.meta["R"])
        la0 = ln - int(w["ref_pos"]) if d == 1 else int(w["ref_pos"]) + 16
        la = post - int(w["ref_pos"]) if d == 1 else int(w["ref_pos"]) + 16 - pre
        mine = 1
        if growers[d] and la0 < thr:
            n_rewalk += 1
            # the accessor before grower g was la0 + (what the growers before g added); it matters while below thr
            added = 0
            for g_depth, g_add in growers[d]:
                if la0 + added < thr:
                    mine = max(mine, g_depth + 1)
                added += g_add
        depth = max(depth, mine)
        if int(w["matlen_a"]) == la:
            add = s_len - int(w["matlen_b"])
            growers[d].append((mine, add))
            if d == 1:
                post += add; nf += 1
            else:
                pre -= add; nb += 1
    return dict(n_rewalk=n_rewalk, depth=depth, ext=[pre, post, ln], n_grown_fwd=nf, n_grown_bwd=nb)


UNLOCKED = ci.unlocked_cases()
BY_NAME = {c.meta["name"]: c for c in UNLOCKED}
IDS = [c.meta["name"] for c in UNLOCKED]


def test_case_names_are_unique_and_documented():
    assert len(BY_NAME) == len(UNLOCKED)
    for c in UNLOCKED + ci.toolong_cases():
        assert "ss_try" in c.meta["line"] or "pba_cons" in c.meta["line"] or "spaced_round_subset" in c.meta["line"], c.meta["name"]
        assert len(c) == 7 and set(c.pool) <= set(range(len(c.reads)))


@pytest.mark.parametrize("case", UNLOCKED, ids=IDS)
def test_restatement_follows_the_oracles_extents(oracle, case):
    """must_rewalk keeps the oracle's extent in both rounds, and gives the counts each case is named for."""
    o = oracle_round(oracle, case)
    m = must_rewalk(case, o["rows"])
    assert m["ext"] == o["ext"], (m, o["ext"])
    m2 = must_rewalk(case, o["rows2"], case.meta["pool2"], len(o["evolved"]))
    assert m2["ext"] == o["ext2"], (m2, o["ext2"])
    meta = case.meta
    if meta.get("one_batch"):
        assert m["n_rewalk"] == 0 and m["depth"] <= 1
    if "depth" in meta:
        assert m["depth"] == meta["depth"]
    if meta.get("thr_delta") == -1 or meta["name"] in ("follower_post_01", "follower_pre_01", "ring2_post_01", "ring2_pre_01"):
        assert m["n_rewalk"] == 1 and m["depth"] == 2
    if meta.get("thr_delta", -1) >= 0:
        assert m["n_rewalk"] == 0
    if meta["name"] == "both_fwd":
        assert (m["n_rewalk"], m["depth"], m["n_grown_fwd"], m["n_grown_bwd"]) == (2, 2, 2, 2)
    if meta["name"] == "interior_interleaved":
        assert m["n_rewalk"] == 2 and m["depth"] == 2


def test_pool_and_reversal_differ_in_the_named_columns(oracle):
    n = 0
    for case in UNLOCKED:
        if "twin" not in case.meta:
            continue
        a = oracle_round(oracle, case)["rows"]
        twin = BY_NAME[case.meta["twin"]]
        b = oracle_round(oracle, twin)["rows"]
        for k, r in enumerate(case.pool):
            kb = twin.pool.index(r)
            diff = tuple(c for c in COLS if a[c][k] != b[c][kb])
            assert diff == tuple(case.meta["differs"]), (case.meta["name"], r, diff)
            assert a["found"][k] and b["found"][kb]
        n += 1
    assert n == 8


def test_flip_reads_are_found_as_named(oracle):
    for case in UNLOCKED:
        if "follower_found" not in case.meta:
            continue
        rows = oracle_round(oracle, case)["rows"]
        k = case.pool.index(1)
        assert bool(rows["found"][k]) == case.meta["follower_found"], case.meta["name"]
        if not rows["found"][k]:                  # every probe met its one candidate, which aligned one base short of the gate
            assert rows["n_trials"][k] == rows["n_pairs"][k] == case.max_trial
        assert rows["found"][case.pool.index(0)]


def test_chains_need_three_steps(oracle):
    for side in ci.SIDES:
        for name in ("chain", "gatechain"):
            case = BY_NAME[f"{name}_{side}_fwd"]
            o = oracle_round(oracle, case)
            assert o["rows"]["found"].all() and must_rewalk(case, o["rows"])["depth"] == 3
            for k in (1, 2):                      # run first, each later read gets less: a shorter matlen, or nothing
                alone = oracle_round(oracle, case, pool=[k])["rows"]
                if name == "chain":
                    assert alone["found"][0] and alone["matlen_a"][0] == case.meta["ds"][k] < o["rows"]["matlen_a"][k]
                else:
                    assert not alone["found"][0]
            # ... and C behind A alone is still not what it is behind A and B
            ac = oracle_round(oracle, case, pool=[0, 2])["rows"]
            assert (ac["found"][1], ac["matlen_a"][1]) != (o["rows"]["found"][2], o["rows"]["matlen_a"][2])
            rev = oracle_round(oracle, BY_NAME[f"{name}_{side}_rev"])
            assert must_rewalk(BY_NAME[f"{name}_{side}_rev"], rev["rows"])["n_rewalk"] == (2 if name == "chain" else 0)


def test_threshold_trio_by_the_oracles_own_clip(oracle):
    """The follower's accessor is thr - 1, thr, thr + 1 long, where thr is the len_b + max_dst the oracle's aligner
    itself reports (seq_aligner.h:94-102); only below thr does the clipped len_a change with the grower's 250 bases."""
    g = ci.genome()
    for side in ci.SIDES:
        for d in (-1, 0, 1):
            case = BY_NAME[f"thr_{side}_{'m1' if d < 0 else 'p%d' % d}"]
            w = oracle_round(oracle, case)["rows"][1]
            rd = case.reads[1]
            assert w["found"] and w["j"] == 0 and w["dir"] == (1 if side == "post" else -1)
            if side == "post":
                la = ci.L - int(w["ref_pos"])
                a0, a1 = case.text[ci.L - la:], g[ci.P0 + ci.L - la:ci.P0 + ci.L + 250]
            else:
                la = int(w["ref_pos"]) + 16
                a0, a1 = case.text[:la], g[ci.P0 - 250:ci.P0 + la]
            fwd = side == "post"
            r0 = oracle.align(a0, rd, ci.R, a_fwd=fwd, b_fwd=fwd)
            r1 = oracle.align(a1, rd, ci.R, a_fwd=fwd, b_fwd=fwd)
            thr = r1["len_b"] + r1["max_dst"]
            assert thr == ci.thr_of(len(rd)) and la == thr + d
            assert (r0["len_a"] != r1["len_a"]) == (d < 0), (side, d, r0, r1)
            assert (r0["cost"], r0["matlen_a"], r0["matlen_b"]) == (r1["cost"], r1["matlen_a"], r1["matlen_b"])


def test_interior_reads_touch_neither_end(oracle):
    for name, ids in (("interior_growers", [0, 2, 4]), ("interior_interleaved", [0, 2, 4, 6])):
        case = BY_NAME[name]
        rows = oracle_round(oracle, case)["rows"]
        for r in ids:
            w = rows[case.pool.index(r)]
            assert w["found"] and w["dir"] == 1 and w["j"] == 0 and w["matlen_a"] == ci.N
            assert ci.L - w["ref_pos"] > ci.thr_of(ci.N) and w["ref_pos"] + ci.N > ci.thr_of(ci.N)


def test_other_end_and_short_text_cases(oracle):
    for side in ci.SIDES:
        rows = oracle_round(oracle, BY_NAME[f"other_end_{side}"])["rows"]
        assert rows["found"].all() and rows["dir"][0] == -rows["dir"][1]      # the follower runs to the other end
        case = BY_NAME[f"short_text_{side}"]
        assert len(case.text) < ci.N + ci.thr_of(ci.N)
        w = oracle_round(oracle, case)["rows"][1]
        assert w["found"] and w["dir"] == -1 and w["n_pairs"] == 2            # a failed forward candidate, then the backward one
        assert len(case.text) - case.text.find(case.reads[1][:16]) <= ci.thr_of(ci.N) and w["ref_pos"] + 16 <= ci.thr_of(ci.N)
    rows = oracle_round(oracle, BY_NAME["fwd_after_prepend"])
    assert rows["rows"]["dir"].tolist() == [-1, -1, 1, 1] and rows["ext"][0] < 0 and rows["rows"]["ref_pos"][2] == ci.L - ci.D_FOLLOW


def test_vote_cases_leave_contested_boxes_at_the_seam(oracle):
    for case in UNLOCKED:
        if not case.meta["name"].startswith("vote_"):
            continue
        o = oracle_round(oracle, case)
        pre, post, end = o["ext"]
        w = np.ones(post - pre, np.int64); w[-pre:-pre + end] = case.weight           # what cons_fill / append put into sel
        ignored = o["tot"] - 1 > o["sel"].sum(axis=1) - w                               # a DELETE vote: tot without sel
        two = ((o["sel"] > 0).sum(axis=1) >= 2) | (o["sup"] > 0).any(axis=1) | ignored     # two alleles, the gap among them
        seam = slice(-pre + end - 3, -pre + end + 3) if "post" in case.meta["name"] else slice(-pre - 3, -pre + 3)
        assert two[seam].any(), case.meta["name"]
        grown = o["tot"][-pre + end:] if "post" in case.meta["name"] else o["tot"][:-pre]
        assert grown.size >= 250 and (grown >= 2).sum() >= 100, case.meta["name"]
        assert o["rows"]["found"].all() and must_rewalk(case, o["rows"])["n_rewalk"] >= 1


def test_pool_forms(oracle):
    case = BY_NAME["subset_pool"]
    assert sorted(case.pool) != case.pool and set(case.meta["outside"]).isdisjoint(case.pool)
    assert oracle_round(oracle, case)["rows"]["read"].tolist() == case.pool
    for n in (0, 10, 15):
        o = oracle_round(oracle, BY_NAME[f"tiny_text_{n}"])
        assert not o["rows"]["found"].any() and not o["rows"]["n_trials"].any() and o["ext"] == [0, n, n]
    for case in ci.toolong_cases():               # on a buffer that is large enough the growth passes 2 * max_len
        ext = oracle_round(oracle, case)["ext"]
        assert ext[1] > 2 * case.meta["max_len"] or -ext[0] > case.meta["max_len"]


def test_ring_lengths_come_from_the_plan():
    import align_rings as ar
    n2 = ci.ring_read_len(2)
    assert ar.nb1(1 + int(n2 * ci.R)) == 2 and ar.nb1(1 + int((n2 - 1) * ci.R)) == 1 and ar.nb1(1 + int(ci.N * ci.R)) == 1
    for case in UNLOCKED:
        md = 1 + int(max(len(r) for r in case.reads) * ci.R)
        assert ar.nb1(md) == case.meta.get("ring", 1), case.meta["name"]
    for ring in (1, 2):
        reads, _, _ = ci.locked_reads(ring)
        assert ar.nb1(1 + int(max(len(r) for r in reads) * ci.R)) == ring


# ------------------------------------------------------------------------------------------------ locked-round gates
def locked_rows(oracle, ring, buggy, max_trial=ci.LOCK_MAX_TRIAL):
    key = ("locked", ring, buggy, max_trial)
    if key not in _CACHE:
        reads, names, nc = ci.locked_reads(ring)
        file, offs = ci.records(reads)
        _CACHE[key] = oracle.spaced_round(ci.locked_ref(), oracle.mask_from_pattern(ci.PATTERN), ci.R, file, offs, max_trial,
                                          ci.LOCK_OVERLAP_MIN, buggy=buggy, nthreads=4)
    return _CACHE[key]


def test_locked_gate_reads_are_what_they_are_named_for(oracle):
    reads, names, nc = ci.locked_reads(1)
    rows = locked_rows(oracle, 1, False)
    at = {n: k for k, n in enumerate(names)}
    for n, want in ci.PLANT_PAIRS.items():        # hit lists that end before, at and behind a 64-lane batch of candidates
        assert rows["found"][at[n]] and rows["n_pairs"][at[n]] == want and rows["j"][at[n]] == 0
    assert sorted(ci.PLANT_PAIRS.values()) == [1, 64, 65, 66, 129, 130]
    w = rows[at["poly_a"]]                        # key 0: the forward probe j = 0 is no trial; found backward at j = 0
    assert w["found"] and w["dir"] == -1 and w["j"] == 0 and w["n_trials"] == 2 * (w["j"] + 1) - 1
    w = rows[at["short_first_hit"]]               # position 47 aligns with matlen_a = overlap_min - 1, then 8000 passes
    assert w["found"] and w["dir"] == -1 and w["n_pairs"] == 2 and w["ref_pos"] == ci.SHORT_HIT_END - 16
    rd, ref = reads[at["short_first_hit"]], ci.locked_ref()
    first = oracle.align(ref[:63], rd, ci.R, a_fwd=False, b_fwd=False)
    assert first["rc"] >= 0 and first["matlen_a"] == ci.LOCK_OVERLAP_MIN - 1
    assert rows["dir"][at["both_dirs"]] == 1 and rows["dir"][at["both_dirs_bwd"]] == -1       # found either way at j = 0: forward wins
    assert rows["j"][at["both_dirs"]] == 0 and rows["j"][at["both_dirs_bwd"]] == 0
    for n in ci.SHORT_LENS:                       # exact copies: every probe the gate lets through is a trial
        w = rows[at[f"short_{n}"]]
        assert bool(w["found"]) == (n >= ci.LOCK_OVERLAP_MIN)
        if not w["found"]:
            assert w["n_trials"] == 2 * ci.LOCK_MAX_TRIAL - len(ci.skipped_probes(n)) and w["n_pairs"] == 0
        t = rows[at[f"short_tail_{n}"]]
        assert bool(t["found"]) == (n >= ci.LOCK_OVERLAP_MIN) and (not t["found"] or t["dir"] == -1)
    for mt in (0, 1):
        r = locked_rows(oracle, 1, False, mt)
        assert (r["j"] < mt).all() and r["found"].sum() == (0 if mt == 0 else rows["found"][rows["j"] == 0].sum())


@pytest.mark.parametrize("ring", (1, 2))
def test_no_skipped_probe_would_have_hit(oracle, ring):
    """ss_try skips a probe with pos < 0 or pos + 16 > slen; the oracle (like the reference, which never meets such a read)
    reads the neighbouring records there.  For the short reads of the set none of those windows is a key of the index, in
    either seed placement: the rows cannot depend on anything but the gate."""
    reads, names, nc = ci.locked_reads(ring)
    file, offs = ci.records(reads)
    mask = oracle.mask_from_pattern(ci.PATTERN)
    keys = set(oracle.index(ci.locked_ref(), mask, "head_tail")[0].tolist())
    buf = np.frombuffer(file + b"\0" * 64, np.uint8)
    n = 0
    for r, (nm, rd) in enumerate(zip(names, reads)):
        if not nm.startswith("short_") or nm == "short_first_hit":
            continue
        assert int(offs[r]) >= 64 and names[r - 1].startswith("spacer") and len(rd) in ci.SHORT_LENS
        for pos, _ in ci.skipped_probes(len(rd)):
            for fn in (oracle.lib.orc_seed_at, oracle.lib.orc_seed_at_fixed):
                assert fn(C.c_void_p(buf.ctypes.data + int(offs[r])), pos) & mask not in keys, (nm, pos)
                n += 1
    assert n == 2 * sum(len(ci.skipped_probes(k)) for k in ci.SHORT_LENS) * 2 > 500
