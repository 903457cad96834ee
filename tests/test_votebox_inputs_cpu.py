"""What the inputs of tests/votebox_inputs.py are, proved on the CPU from the oracle (oracle/pba_oracle.c) and from the
module's own plain model of elect and evolve: every named state is in the regime it is named for -- the yield class at the
named boxes, which output absorbs which deleted box, 2 * max against tot at the tie boxes, the advancing ops per 64-op chunk
of the elect scripts, the votes that fall outside the range, the vote count at which the sweep's single op falls, the boxes
of the pile-up case that yield 2, 0 or 1.  tests/test_gpu_votebox.py runs the kernels on the same inputs."""
import numpy as np
import pytest

import votebox_inputs as vb
from polish_helpers import EDGE_DEL, EDGE_INS, TILE, edge_case, oracle_boxes, oracle_evolve, oracle_vote, yields

EVOLVE = {s.name: s for s in vb.evolve_states()}
ELECT = {s.name: s for s in vb.elect_states()}


def oracle_stages(oracle, st):
    c = vb.build(oracle.consensus, st)
    vb.elect_loop(c, st)
    return vb.stages(c, st)


def model_stages(st, rounds=2):
    """the stages of vb.stages from the plain model: ((sel, sup, tot, extent, text), ...), src and absorbed per evolve"""
    sel, sup, tot = vb.model_boxes(st)
    out = [(sel, sup, tot, [-len(st.pre), len(st.base) + len(st.app), len(st.base)], st.text)]
    maps = []
    for _ in range(rounds):
        sel, sup, tot, text, src, absorbed = vb.model_evolve(sel, sup, tot)
        out.append((sel, sup, tot, [0, len(tot), len(tot)], text))
        maps.append((src, absorbed))
    return out, maps


def test_the_states_the_issue_names_are_all_there():
    names = set(EVOLVE)
    for form in vb.FORMS:
        for n in (1023, 1024, 1025, 2048, vb.BIG):
            assert f"len_{n}/{form}" in names
        for want in ["split_at_1022", "split_at_1023", "split_at_1024", "split_at_2047", "del_behind_kept", "del_behind_split",
                     "del_with_supply_at_0", "del_with_supply_at_1023", "del_with_supply_at_1024", "del_run_across_edge",
                     "del_run_at_start", "chunk_all_deleted", "chunk0_all_deleted", "ties_w1", "ties_w3", "weight_0",
                     "winner_ties_w3", "two_evolves"]:
            assert f"{want}/{form}" in names
    assert "len_1/plain" in names and "len_1_deleted/plain" in names
    assert len(names) == len(vb.evolve_states())                       # no two states share a name
    assert set(ELECT) == {"elect/" + k for k in ("chunks", "tails", "insert_dropped", "insert_kept", "slots", "hammer",
                                                 "fuzz_inside", "fuzz_any", "limits")}
    for s in vb.evolve_states():
        assert s.n <= s.max_len and s.ref_safe, s.name
        assert (len(s.pre) == vb.PRE) == s.name.endswith("/prepended") and not s.app
        assert all(sc.nedit == 1 for sc in s.scripts)                   # planted with one-op scripts only
    assert {s.name for s in vb.elect_states() if not s.ref_safe} == {"elect/tails", "elect/insert_dropped", "elect/fuzz_any"}
    for s in vb.elect_states()[:-1]:
        assert s.n == vb.ELECT_N and len(s.pre) == vb.ELECT_PRE and len(s.app) == vb.ELECT_APP


@pytest.mark.parametrize("name", sorted(EVOLVE) + sorted(ELECT))
def test_oracle_equals_the_plain_model(oracle, name):
    """elect, evolve and a second evolve: boxes, extent and text of the oracle are those of the model"""
    st = vb.state(name)
    want, _ = model_stages(st)
    got = oracle_stages(oracle, st)
    assert len(got) == len(want) == 3
    for k, (g, w) in enumerate(zip(got, want)):
        assert vb.same_stage(g, w), (name, k)


@pytest.mark.parametrize("name", sorted(EVOLVE))
def test_evolve_state_is_in_its_regime(oracle, name):
    st = vb.state(name)
    sel, sup, tot, ext, text = oracle_stages(oracle, st)[0]
    assert ext == [-len(st.pre), st.n - len(st.pre), st.n - len(st.pre)] and text == st.text
    assert int(sel.max()) <= 65535 and int(sup.max()) <= 65535
    y = yields(sel, sup, tot)
    V, S = 2 * sel.max(axis=1).astype(int) > tot, 2 * sup.max(axis=1).astype(int) > tot
    for box, cls in st.marks.get("yield", {}).items():
        if cls == "split_only":
            assert not V[box] and S[box] and y[box] == 1, (name, box)
        else:
            assert y[box] == cls and (cls != 1 or V[box]), (name, box, int(y[box]))
    for box, (which, rel) in st.marks.get("tie", {}).items():
        mx = int((sel if which == "sel" else sup)[box].max())
        assert 2 * mx == int(tot[box]) + rel, (name, box)
        assert bool((V if which == "sel" else S)[box]) == bool(rel)
    for box, (which, win) in st.marks.get("winner", {}).items():
        v = (sel if which == "sel" else sup)[box]
        assert b"ACGT"[int(np.argmax(v))] == win[0], (name, box)
        assert (int((v == v.max()).sum()) == 1) == (win == b"T"), (name, box)     # a tie everywhere but where T wins
    # which output absorbs what: the model's map of the first evolve, the oracle's boxes being the model's (test above)
    stages, maps = model_stages(st)
    src, absorbed = maps[0]
    for box, into in st.marks.get("absorb", {}).items():
        assert box in absorbed, (name, box)
        if into is None:
            assert absorbed[box] == -1, (name, box)
        else:
            assert src[absorbed[box]] == into, (name, box, src[absorbed[box]])
            assert (stages[1][1][absorbed[box]] >= stages[0][0][box]).all()          # its suppliment holds that selection
    for box, base in st.marks.get("second_split", {}).items():
        k = src.index((box, 0))
        src2 = maps[1][0]
        assert src2.count((k, 1)) == 1 and stages[2][4][src2.index((k, 1))] == base[0]
        assert stages[0][1][box].sum() == 0                                       # nothing was supplied: absorbed counts only
    for box in st.marks.get("second_kept_whole", {}):
        assert maps[1][0].count((src.index((box, 0)), 1)) == 0


def test_regimes_across_the_chunk_grid():
    """What the names promise about the 1 024-box chunks counted from pre."""
    for form in vb.FORMS:
        st = vb.state(f"chunk_all_deleted/{form}")
        stages, maps = model_stages(st)
        y = yields(*stages[0][:3])
        assert not y[vb.CHUNK:2 * vb.CHUNK].any() and y[2 * vb.CHUNK] == 0 and y[:vb.CHUNK].all()
        k = maps[0][0].index((vb.CHUNK - 1, 0))
        assert int(stages[1][1][k].sum()) == vb.CHUNK + 1 and int(stages[1][1][k].max()) < 65535
        st = vb.state(f"chunk0_all_deleted/{form}")
        stages, maps = model_stages(st)
        assert not yields(*stages[0][:3])[:vb.CHUNK + 1].any() and not stages[1][1].any()
        st = vb.state(f"del_run_across_edge/{form}")
        stages, maps = model_stages(st)
        k = maps[0][0].index((1018, 0))
        assert (stages[1][1][k] > 0).all() and int(stages[1][1][k].sum()) == 12   # all four counters, both dwords
        st = vb.state(f"weight_0/{form}")
        stages, _ = model_stages(st)
        voted = bytes(st.text[b] for b in (40, 1023, 1024, 1099))
        assert stages[1][4] == st.pre + voted[:1] + b"A" + voted[1:]              # (the prepended boxes have weight 1)
    assert vb.state("len_1_deleted/plain").n == 1 and model_stages(vb.state("len_1_deleted/plain"))[0][1][4] == b""


@pytest.mark.parametrize("name", sorted(ELECT))
def test_elect_scripts_are_where_they_are_meant_to_be(name):
    st = vb.state(name)
    targets = [vb.vote_targets(st, sc) for sc in st.scripts]
    inside = [bool(((t >= 0) & (t < st.n)).all()) for t in targets]
    if name == "elect/chunks":
        assert sorted({sc.nedit for sc in st.scripts}) == list(vb.ELECT_LENS) and len(st.scripts) == 2 * 3 * len(vb.ELECT_LENS)
        heads = set()
        for sc in st.scripts:
            per = vb.advancing_per_chunk(sc)
            assert len(per) == -(-sc.nedit // vb.WAVE) and all(0 < a < vb.WAVE for a in per[:sc.nedit // vb.WAVE])   # every full chunk
            assert sc.ops[0] == vb.MATCH
            for k in (vb.WAVE, 2 * vb.WAVE):
                if k < sc.nedit:
                    heads.add((k, int(sc.ops[k]), sc.fwd))
        assert heads == {(k, op, f) for k in (64, 128) for op in (1, 2, 3) for f in (True, False)}
        assert all(inside)
    elif name == "elect/tails":
        assert not any(inside)
        assert any((t >= st.n).any() for t in targets) and any((t < 0).any() for t in targets)
        assert all(((t >= 0) & (t < st.n)).any() for t in targets)              # every script also votes inside
    elif name == "elect/insert_dropped":
        assert [int(t[0]) for t in targets] == [-1, -1] and all(sc.ops[0] == vb.INSERT and sc.fwd for sc in st.scripts)
    elif name == "elect/insert_kept":
        assert all(inside)
        assert [int(t[int(np.flatnonzero(sc.ops == vb.INSERT)[0])]) for t, sc in zip(targets, st.scripts)] == [st.n - 1, 0, 0, st.n - 1]
    elif name == "elect/slots":
        assert sum(sc.nedit == 0 for sc in st.scripts) == 4 and all(sc.ops.size >= sc.nedit for sc in st.scripts)
        long_slots = [sc for sc in st.scripts if sc.ops.size > sc.nedit]
        assert len(long_slots) == 12 and all((sc.ops[sc.nedit:] != 0).all() for sc in long_slots)   # the tail would vote
        assert all(inside)
    elif name == "elect/hammer":
        assert len(st.scripts) == 500 and {int(x) for t in targets for x in t} == {200, 201, 202}
    elif name == "elect/fuzz_inside":
        assert len(st.scripts) == 200 and all(inside) and max(sc.nedit for sc in st.scripts) > 256
        assert any(sc.ops[0] == vb.INSERT and sc.fwd for sc in st.scripts if sc.nedit)
    elif name == "elect/fuzz_any":
        assert len(st.scripts) == 200 and 20 < sum(inside) < 180
    else:
        assert name == "elect/limits" and st.weight == 65534
        sel, sup, tot = vb.model_boxes(st)
        for c, b in enumerate(vb.LIMIT_BOXES):
            assert sel[b].tolist() == [65535 if k == c else 0 for k in range(4)] and tot[b] == 2
        others = [b for b in range(st.n) if b not in vb.LIMIT_BOXES]
        assert (sel[others].max(axis=1) == 65534).all() and (tot[others] == 1).all() and not sup.any()
        assert int(sel.max()) == 65535


def test_sweep_covers_every_phase_of_the_gather(oracle):
    """The walk hands its ops to VoteSink from the alignment's end: the op of index k of an n-op script is vote n - 1 - k.
    Per kind and direction the single planted op falls on every lane of the gather, and the run behind it is cut at every
    vote count mod 64."""
    text, reads, pairs, meta = vb.sweep_case()
    cons, res = vb.sweep_expectation(oracle)
    assert len(pairs) == len(meta) == 2 * (3 * len(vb.SWEEP_D) + 8) and len(vb.SWEEP_D) == 130
    phases = {}
    voted = 0
    for pr, (kind, d, fwd), out in zip(pairs, meta, res):
        seg = reads[int(pr["b_seq"])]
        a = text[int(pr["a_pos"]):] if fwd else text[:int(pr["a_pos"]) + 1][::-1]
        b = seg if fwd else seg[::-1]
        assert out["rc"] >= 0, (kind, d, fwd)
        voted += out["matlen_a"] >= vb.OVERLAP_MIN
        edits = vb.edit_phase(a, b, out["ops"])
        if kind == "run":
            assert out["cost"] == 0 and not edits and (out["ops"] == vb.MATCH).all()
            continue
        n_ops = len(out["ops"])
        if kind == "ins":       # the read is one base longer than its slice: the aligner ends a base further and pays a DELETE
            assert out["cost"] == len(edits) <= 2, (kind, d, fwd)          # for it among the last ops, behind the planted one
            assert all(out["ops"][k] == vb.DELETE and n_ops - 1 - k < 8 for k in edits[1:]), (kind, d, fwd)
        else:
            assert out["cost"] == 1 and len(edits) == 1, (kind, d, fwd)
        assert int(out["ops"][edits[0]]) == {"sub": vb.MATCH, "ins": vb.INSERT, "del": vb.DELETE}[kind]
        phases.setdefault((kind, fwd), set()).add((n_ops - 1 - edits[0]) % vb.WAVE)
    assert voted == len(pairs) - 6                                      # the three 50-base reads are gated out, both ways
    assert set(phases) == {(k, f) for k in vb.SWEEP_KINDS for f in (True, False)}
    for key, seen in phases.items():
        assert seen == set(range(vb.WAVE)), key
    assert {(vb.SWEEP_L - d) % vb.WAVE for d in vb.SWEEP_D} == set(range(vb.WAVE))
    sel, sup, tot, _ = cons.dump(len(text) + 8)
    assert int(tot.max()) > 100 and int(sup.sum()) == 2 * len(vb.SWEEP_D)


def test_pile_case_yields_what_was_planted(oracle):
    contigs, reads, rows = vb.pile_case()
    assert [len(c) for c in contigs] == list(vb.PILE_LENS) and max(vb.PILE_LENS) <= 65536
    sites = sorted(vb.PILE_INS + tuple(d[0] for d in vb.PILE_DEL) + (vb.PILE_TIE,))
    assert all(b - a >= 1500 for a, b in zip(sites, sites[1:]))
    assert [s % vb.STEP for s in vb.PILE_INS] == [vb.STEP - 1, vb.WAVE - 1]
    assert [tuple(b % vb.STEP for b in d) for d in vb.PILE_DEL] == [(vb.STEP - 1, 0), (vb.WAVE,)]
    for r, s in zip(reads, rows["pos"]):
        assert sum(int(s) <= x < int(s) + len(r) + 2 for x in sites) == 1         # no read covers two sites
    cons, res, voted = oracle_vote(oracle, contigs, reads, rows, vb.PILE_C)
    assert voted == len(reads) == 4 * vb.PILE_VOTERS + 7
    n = len(contigs[vb.PILE_C])
    sel, sup, tot = oracle_boxes(cons, n)
    y = yields(sel, sup, tot)
    assert np.flatnonzero(y == 2).tolist() == sorted(vb.PILE_INS + vb.PILE_EXTRA_TWO)
    assert np.flatnonzero(y == 0).tolist() == sorted(tuple(b for d in vb.PILE_DEL for b in d) + vb.PILE_EXTRA_NONE)
    assert len(vb.PILE_EXTRA_TWO) + len(vb.PILE_EXTRA_NONE) <= 4
    for site in vb.PILE_INS:
        assert int(tot[site]) == 1 + vb.PILE_VOTERS and sup[site].tolist() == [0, 0, 0, vb.PILE_VOTERS]
    for b in (b for d in vb.PILE_DEL for b in d):
        assert int(tot[b]) == 1 + vb.PILE_VOTERS and int(sel[b].max()) == 1
    assert int(tot[vb.PILE_TIE]) == 8 and sup[vb.PILE_TIE].tolist() == [0, 0, 0, 4] and y[vb.PILE_TIE] == 1   # 2 * 4 == tot
    want = oracle_evolve(cons, n)
    assert len(want) == int(y.sum()) == n + len(vb.PILE_INS) - 3 - len(vb.PILE_EXTRA_NONE)


def test_novote_lengths_straddle_wave_step_and_chunk():
    assert set(vb.NOVOTE_LENS) == {k + e for k in (64, 256, 512, 1024) for e in (-1, 0, 1)}
    assert [len(t) for t in vb.novote_texts()] == list(vb.NOVOTE_LENS) and vb.NOVOTE_WEIGHTS == (1, 65535)


def test_form_sets_sit_on_either_side_of_the_switch():
    """What test_gpu_qual.py's comparison of the two kernel forms relies on: every original target is served by the per-target
    kernels, the appended sequence is the shortest that is not, and the 20 000-base edge case carries its plants where
    EDGE_INS and EDGE_DEL say, in the text and in its reads."""
    assert vb.FORM_LONG_SEG == 65536 and vb.FORM_SWITCH_LEN == len(vb.form_switch_text()) == 65537
    assert set(vb.form_switch_text()) <= set(b"ACGT")
    T, reads = edge_case(711, vb.FORM_EDGE_LEN)
    originals = list(vb.pile_case()[0]) + list(vb.novote_texts()) + [T]
    assert max(len(t) for t in originals) <= vb.FORM_LONG_SEG
    assert len(T) == vb.FORM_EDGE_LEN == 20000 and len(edge_case(711)[0]) == 70001
    plants = [(s, 0) for s in EDGE_INS] + [(d[0], len(d)) for d in EDGE_DEL]
    assert [s % TILE for s in EDGE_INS] == [TILE - 1] * 2 and [tuple(b % TILE for b in d) for d in EDGE_DEL] == [(TILE - 1, 0), (0,)]
    assert len(reads) == 6 * len(plants)
    for p, (site, lost) in enumerate(plants):
        assert T[site - 1:site + 3] == (b"ACGA" if lost == 1 else b"ACGT")
        for k, r in enumerate(reads[6 * p:6 * p + 6]):
            s = site - 400 - 17 * k
            at = site - s
            assert 0 <= s and s + 900 < 16900 <= len(T)
            if lost:
                assert len(r) == 900 - lost and r[:at] == T[s:site] and r[at:] == T[site + lost:s + 900]
            else:
                assert len(r) == 901 and r[:at + 1] == T[s:site + 1] and r[at + 1:at + 2] == b"T" and r[at + 2:] == T[site + 1:s + 900]
