"""The vote-box core on the device, pinned at its own boundaries (csrc/consensus.h: k_cons_elect, VoteSink, cons_yield,
cons_bump, k_cons_evolve; csrc/pba_pileup.hip: k_pile_fill / count / write) on the hand-built inputs of
tests/votebox_inputs.py, which tests/test_votebox_inputs_cpu.py proves to sit on those boundaries.  Held to the CPU oracle
box for box, extent for extent and byte for byte, and to what the reference itself gave (tests/golden/votebox.json) where
the reference is defined.  All comparisons are exact.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import votebox_inputs as vb
from conftest import gold_json
from pacbioassembly_amd import Pileup
from pacbioassembly_amd import engine as eng
from polish_helpers import check_result, oracle_boxes, oracle_evolve, oracle_vote

pytestmark = pytest.mark.gpu

EVOLVE = sorted(s.name for s in vb.evolve_states())
ELECT = sorted(s.name for s in vb.elect_states())


@pytest.fixture(scope="module")
def gold():
    return gold_json("votebox.json")["states"]


def oracle_stages(oracle, st):
    c = vb.build(oracle.consensus, st)
    vb.elect_loop(c, st)
    return vb.stages(c, st)


def device_cons(ctx, st):
    return vb.build(lambda base, weight, max_len: eng.Consensus(ctx, base, weight, max_len), st)


def assert_stages(got, want, tag):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for x, y, what in zip(g[:3], w[:3], ("sel", "sup", "tot")):
            assert x.shape == y.shape and (x == y).all(), (tag, k, what, np.flatnonzero((x != y).reshape(len(x), -1).any(axis=1))[:8])
        assert g[3] == w[3], (tag, k, "extent", g[3], w[3])
        assert g[4] == w[4], (tag, k, "text")


@pytest.mark.parametrize("name", ELECT)
def test_elect(ctx, oracle, gold, name):
    """One pba_cons_elect call over all scripts of the family (each in its own slot, some slots longer than their nedit),
    and the same scripts one call each: the dump is the oracle's, and so is what two evolves make of it."""
    st = vb.state(name)
    want = oracle_stages(oracle, st)
    many = device_cons(ctx, st)
    vb.elect_batch(many, st.scripts)
    got = vb.stages(many, st)
    assert_stages(got, want, name)
    one = device_cons(ctx, st)
    for sc in st.scripts:
        one.elect([sc.pos], [sc.fwd], [sc.ops[:sc.nedit]], [sc.vals[:sc.nedit]])
    assert_stages([vb.snap(one, 0)], want[:1], name + " one by one")
    assert (name in gold) == st.ref_safe
    if name in gold:
        assert vb.record(got) == gold[name], name
    if name == "elect/limits":
        sel = got[0][0]
        for c, b in enumerate(vb.LIMIT_BOXES):
            assert sel[b].tolist() == [65535 if k == c else 0 for k in range(4)]


@pytest.mark.parametrize("name", EVOLVE)
def test_evolve(ctx, oracle, gold, name):
    """Text, extent and every counter -- the absorbed suppliments among them -- after the votes, after evolve and after a
    second evolve on what the first one left."""
    st = vb.state(name)
    want = oracle_stages(oracle, st)
    c = device_cons(ctx, st)
    vb.elect_batch(c, st.scripts)
    got = [vb.snap(c, 0)]
    for k in (1, 2):
        text = c.evolve()
        got.append(vb.snap(c, 0))
        assert text == got[k][4] and got[k][3] == [0, len(text), len(text)], (name, k)
    assert_stages(got, want, name)
    assert vb.record(got) == gold[name], name


def test_vote_pairs_phase_sweep(ctx, oracle):
    """One pba_cons_vote_pairs call over the sweep: a single substitution, insertion or deletion at every vote count mod 64
    of VoteSink's gather, forward and backward, and pure runs of 300 and 650 matches that put_run cuts at every count."""
    text, reads, pairs, meta = vb.sweep_case()
    cons, want_res = vb.sweep_expectation(oracle)
    A = ctx.seqs_from_list([b"ACGT" * 10, text], strict_acgt=True)       # the reference is sequence 1 of its set
    B = ctx.seqs_from_list(list(reads), strict_acgt=True)
    c = eng.Consensus(ctx, text, 1, vb.MAX_LEN)
    res = c.vote_pairs(A, 1, B, pairs, vb.R, vb.OVERLAP_MIN)
    for q, (g, w) in enumerate(zip(res, want_res)):
        assert int(g["rc"]) == w["rc"], (q, meta[q])
        for k in ("cost", "matlen_a", "matlen_b"):
            assert int(g[k]) == w[k], (q, meta[q], k)
    got = vb.snap(c, 0)
    want = vb.snap(cons, len(text) + 8)
    assert_stages([got], [want], "sweep")
    cons2 = oracle.consensus(text, 1, vb.MAX_LEN)                         # (the shared expectation stays as it is)
    for pr, w in zip(pairs, want_res):
        if w["rc"] >= 0 and w["matlen_a"] >= vb.OVERLAP_MIN:
            fwd = int(pr["flags"]) == 0
            cons2.elect(int(pr["a_pos"]), fwd, w["ops"], eng.script_vals(w["ops"], reads[int(pr["b_seq"])], fwd))
    cons2.evolve()
    assert c.evolve() == cons2.text(2 * len(text) + 8)
    assert_stages([vb.snap(c, 0)], [vb.snap(cons2, 2 * len(text) + 8)], "sweep evolved")


def test_pileup_per_target_edges(ctx, oracle):
    """The per-target pile-up kernels on a contig that is the second of three: an inserted base after thread 255 of a step
    and after lane 63 of wave 0, lost bases on both sides of a step edge and at lane 0 of wave 1, a tie that does not
    split."""
    contigs, reads, rows = vb.pile_case()
    assert max(len(c) for c in contigs) <= 65536                         # the per-target kernels serve, not the tiled ones
    cons, want_res, want_voted = oracle_vote(oracle, contigs, reads, rows, vb.PILE_C)
    n = len(contigs[vb.PILE_C])
    boxes = oracle_boxes(cons, n)
    S = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    pile = Pileup(ctx, S)
    res, n_voted = pile.vote_mapped(Rd, rows, vb.R, vb.OVERLAP_MIN)
    assert n_voted == want_voted == len(reads)
    for k, o in want_res.items():
        check_result(res[k], o, k)
    for x, w, name in zip(pile.dump(vb.PILE_C), boxes, ("sel", "sup", "tot")):
        assert x.shape == w.shape and (x == w).all(), (name, np.flatnonzero((x != w).reshape(n, -1).any(axis=1))[:8])
    for t in (0, 2):                                                     # the neighbours' boxes are as they were filled
        sel, sup, tot = pile.dump(t)
        assert (sel.sum(axis=1) == 1).all() and not sup.any() and (tot == 1).all()
        assert bytes(b"ACGT"[k] for k in sel.argmax(axis=1)) == contigs[t]
    out, crows = pile.evolve()
    want = oracle_evolve(cons, n)
    assert [out.get_text(t) for t in range(3)] == [contigs[0], want, contigs[2]]
    assert [int(x) for x in crows["len_out"]] == [len(contigs[0]), len(want), len(contigs[2])]
    assert [int(x) for x in crows["n_rows"]] == [0, len(reads), 0]


@pytest.mark.parametrize("weight", vb.NOVOTE_WEIGHTS)
def test_pileup_without_votes_returns_the_texts(ctx, weight):
    """Lengths on both sides of a wave, a step, two steps and four, at the smallest and the largest weight."""
    texts = list(vb.novote_texts())
    assert max(len(t) for t in texts) <= 65536
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    pile = Pileup(ctx, S, weight=weight)
    for t, text in enumerate(texts):
        sel, sup, tot = pile.dump(t)
        assert (sel.max(axis=1) == weight).all() and (sel.astype(np.int64).sum(axis=1) == weight).all()
        assert bytes(b"ACGT"[k] for k in sel.argmax(axis=1)) == text and not sup.any() and (tot == 1).all()
    out, crows = pile.evolve()
    assert [out.get_text(t) for t in range(len(texts))] == texts
    assert [int(x) for x in crows["len_out"]] == [len(t) for t in texts] and not crows["n_rows"].any()
