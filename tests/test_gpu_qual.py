"""Per-base evidence, Phred qualities and FASTQ out on the device (pba_qual_*, pba_pileup_evolve_qual, the *_qual drivers,
pba_seqs_write_fastq), held to tests/qual_ref.py -- the rule in plain numpy, pinned by hand in
tests/test_qual_cpu.py -- over the dumps of twin pile-ups.  All comparisons are exact.  Needs a real MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

import qual_ref as qr
import votebox_inputs as vb
from conftest import MASK_PAT
from correct_helpers import mixed_reads
from pacbioassembly_amd import Pileup, Qual
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PbaError
from place_ref import NOISY_SEED, noisy_reads
from polish_helpers import EDGE_DEL, EDGE_INS, OVERLAP_MIN, POLISH_LENS, R, TILE, edge_case, polish_case

pytestmark = pytest.mark.gpu
MASK = eng.mask_from_pattern(MASK_PAT)
KEYS = ("qv", "depth", "agree", "src")


def texts_of(S):
    return [S.get_text(i) for i in range(S.count)]


def status(call):
    with pytest.raises(PbaError) as e:
        call()
    return e.value.status


def map_rows(ctx, T, Rd, strands=3, reads_rc=None):
    ix = ctx.index_build_set(T, MASK)
    rows, _ = ctx.map_reads(ix, T, Rd, R, strands=strands, reads_rc=reads_rc)
    ix.close()
    return rows


def dumps_evidence(pile, n, weight, qmax=60):
    """qual_ref.evidence of every target's dump, as it stands"""
    return [qr.evidence(*pile.dump(t), weight, qmax) for t in range(pile.t_lo, pile.t_lo + n)]


def assert_evidence(out, qual, want, tag=""):
    """The set and its Qual against per-target expectations: texts, lengths, and the four arrays target by target and whole."""
    n = len(want)
    assert out.count == qual.count == n
    lens = [len(w["text"]) for w in want]
    assert qual.lengths().tolist() == out.lengths().tolist() == lens, tag
    assert texts_of(out) == [w["text"] for w in want], tag
    whole = qual.get()
    for k in KEYS:
        cat = np.concatenate([w[k] for w in want]) if n else np.zeros(0, whole[k].dtype)
        assert whole[k].dtype == cat.dtype and whole[k].shape == cat.shape, (tag, k)
        bad = np.flatnonzero(whole[k] != cat)
        assert bad.size == 0, (tag, k, bad[:8], whole[k][bad[:8]], cat[bad[:8]])
    for t in {0, n // 2, n - 1} if n else ():
        got = qual.get(t, t + 1)
        assert all((got[k] == want[t][k]).all() and len(got[k]) == lens[t] for k in KEYS), (tag, t)


# ----------------------------------------------------------------------------- 1: the rule on the device
def phred_device(ctx, agree, n, qmax):
    agree, n = np.ascontiguousarray(agree, np.uint32), np.ascontiguousarray(n, np.uint64)
    qv = np.full(max(agree.size, 1), 255, np.uint8)
    ctx.check(ctx.lib.pba_qual_phred_device(ctx.h, C.c_void_p(agree.ctypes.data), C.c_void_p(n.ctypes.data), agree.size, qmax,
                                            C.c_void_p(qv.ctypes.data)), "qual_phred_device")
    return qv[:agree.size]


@pytest.mark.parametrize("qmax", [0, 1, 10, 60])
def test_phred_on_the_device(ctx, qmax):
    agree, n = qr.phred_grid()
    assert (phred_device(ctx, agree, n, qmax) == qr.phred_array(agree, n, qmax)).all()
    rng = np.random.default_rng(9000 + qmax)
    n = np.concatenate([rng.integers(0, 200, 50000), rng.integers(0, 2 ** 31 + 65535, 50000)]).astype(np.uint64)
    agree = np.minimum(rng.integers(0, 2 ** 32, 100000).astype(np.uint64) % (n + np.uint64(3)), np.uint64(2 ** 32 - 1)).astype(np.uint32)
    got, want = phred_device(ctx, agree, n, qmax), qr.phred_array(agree, n, qmax)
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    assert len(set(want.tolist())) >= min(qmax, 20)                              # the fuzz spreads over the scale
    host = [ctx.lib.pba_qual_phred(int(a), int(x), qmax) for a, x in zip(agree[:2000], n[:2000])]
    assert host == got[:2000].tolist()                                           # one body, host and device
    assert ctx.lib.pba_qual_phred_device(ctx.h, C.c_void_p(agree.ctypes.data), C.c_void_p(n.ctypes.data), 4, 61, C.c_void_p(got.ctypes.data)) == -1


# ----------------------------------------------------------------------------- 2, 3: the two write passes at their edges
def twin_piles(ctx, S, vote, weight=1):
    """Two pile-ups voted identically: (the one left for evolve(), the one for dump() then evolve_qual())"""
    a, b = Pileup(ctx, S, weight=weight), Pileup(ctx, S, weight=weight)
    vote(a); vote(b)
    return a, b


def run_pile_case(ctx):
    contigs, reads, rows = vb.pile_case()
    assert max(len(c) for c in contigs) <= 65536                                 # the per-target kernels serve
    S = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    plain, twin = twin_piles(ctx, S, lambda p: p.vote_mapped(Rd, rows, vb.R, vb.OVERLAP_MIN))
    out, crows = plain.evolve()
    want = dumps_evidence(twin, 3, 1)
    out_q, crows_q, qual = twin.evolve_qual()
    assert texts_of(out_q) == texts_of(out) and crows_q.tobytes() == crows.tobytes()
    assert_evidence(out_q, qual, want, "pile_case")
    src = qual.get(vb.PILE_C, vb.PILE_C + 1)["src"]
    sup_at = (src[src >= qr.SUP] & 0x7FFFFFFF).tolist()
    assert sup_at == sorted(vb.PILE_INS)                                         # the SUP characters sit where planted
    kept = set((src & 0x7FFFFFFF).tolist())
    assert all(b not in kept for d in vb.PILE_DEL for b in d) and vb.PILE_TIE in kept and vb.PILE_TIE not in sup_at
    for t in (0, 2):                                                             # the neighbours: nobody voted
        g = qual.get(t, t + 1)
        assert (g["qv"] == 4).all() and not g["depth"].any() and (g["agree"] == 1).all() and (g["src"] == np.arange(len(contigs[t]))).all()
    return qual


def test_per_target_kernels_at_their_edges(ctx):
    run_pile_case(ctx)


def test_tiled_kernels_at_tile_edges(ctx):
    T, reads = edge_case(711)
    assert len(T) > 65536                                                        # the tiled kernels serve
    S = ctx.seqs_from_list([T], strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    rows = map_rows(ctx, S, Rd, strands=1)
    assert rows["found"].all()
    plain, twin = twin_piles(ctx, S, lambda p: p.vote_mapped(Rd, rows, R, OVERLAP_MIN))
    out, crows = plain.evolve()
    want = dumps_evidence(twin, 1, 1)
    out_q, crows_q, qual = twin.evolve_qual()
    assert texts_of(out_q) == texts_of(out) and crows_q.tobytes() == crows.tobytes()
    assert_evidence(out_q, qual, want, "edge_case")
    src = qual.get()["src"]
    sup_at = (src[src >= qr.SUP] & 0x7FFFFFFF).tolist()
    assert sup_at == list(EDGE_INS) and all(b % TILE == TILE - 1 for b in sup_at)   # two characters at a tile's end
    for b in EDGE_INS:
        k = int(np.flatnonzero(src == b)[0])
        assert int(src[k + 1]) == b | qr.SUP                                        # side by side across the tile's end
    kept = set((src & 0x7FFFFFFF).tolist())
    assert all(b not in kept for d in EDGE_DEL for b in d)
    assert (np.diff((src & 0x7FFFFFFF).astype(np.int64)) >= 0).all() and int(src[-1]) == len(T) - 1


# ----------------------------------------------------------------------------- 3b: the two forms held to each other
@pytest.fixture(scope="module")
def form_sets(ctx):
    """name -> (targets, weight, vote): the pile case (plants at a step's last thread, at lane 63, at lane 0 of wave 1, the
    tie), the unvoted texts of 63 ... 1 025 bases at both weights, and the tile-edge plants in a contig short enough for the
    per-target kernels -- there a box's two characters lie inside a step, and straddle a tile's end in the tiled form.  Its
    rows come from the mapper once, on the short set; the contig's index is the same in both."""
    contigs, reads, rows = vb.pile_case()
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    sets = {"pile_case": (list(contigs), 1, lambda p: p.vote_mapped(Rd, rows, vb.R, vb.OVERLAP_MIN))}
    for w in vb.NOVOTE_WEIGHTS:
        sets[f"novote_w{w}"] = (list(vb.novote_texts()), w, lambda p: None)
    T, ereads = edge_case(711, vb.FORM_EDGE_LEN)
    Re = ctx.seqs_from_list(ereads, strict_acgt=True)
    erows = map_rows(ctx, ctx.seqs_from_list([T], strict_acgt=True), Re, strands=1)
    assert erows["found"].all()
    sets["tile_edges"] = ([T], 1, lambda p: p.vote_mapped(Re, erows, R, OVERLAP_MIN))
    return sets


@pytest.mark.parametrize("name", ["pile_case", "novote_w1", "novote_w65535", "tile_edges"])
def test_per_target_and_tiled_forms_agree(ctx, form_sets, name):
    """A set runs the per-target kernels when it stands alone and the tiled ones, for every segment, once one unvoted sequence
    of 65 537 bases -- the shortest that switches the form -- stands behind it.  Same rows voted into both: the original
    targets' texts, rows and evidence are equal byte for byte, plainly evolved and with evidence, and the appended target
    comes back as its own text.  (The threshold is the library's PBA_PILE_LONG_SEG, 65 536 unless a tuning build sets another;
    nothing exposes it, so vb.FORM_LONG_SEG restates the default.  Against a build with a threshold above 65 537 both pile-ups
    would run the per-target kernels and this test would compare that form with itself.)"""
    targets, weight, vote = form_sets[name]
    extra = vb.form_switch_text()
    n = len(targets)
    assert max(len(t) for t in targets) <= 65536 < len(extra) == vb.FORM_SWITCH_LEN == 65537
    short = ctx.seqs_from_list(targets, strict_acgt=True)
    long_ = ctx.seqs_from_list(targets + [extra], strict_acgt=True)

    def piles():
        a, b = Pileup(ctx, short, weight=weight), Pileup(ctx, long_, weight=weight)
        vote(a); vote(b)
        return a, b

    a, b = piles()
    (out_a, crows_a), (out_b, crows_b) = a.evolve(), b.evolve()
    assert texts_of(out_b) == texts_of(out_a) + [extra]
    assert crows_b[:n].tobytes() == crows_a.tobytes()
    assert int(crows_b[n]["n_rows"]) == 0 and int(crows_b[n]["len_out"]) == len(extra)
    a, b = piles()
    (qout_a, qrows_a, qual_a), (qout_b, qrows_b, qual_b) = a.evolve_qual(), b.evolve_qual()
    assert texts_of(qout_a) == texts_of(out_a) and texts_of(qout_b) == texts_of(out_b)
    assert qrows_a.tobytes() == crows_a.tobytes() and qrows_b.tobytes() == crows_b.tobytes()
    assert qual_b.lengths().tolist() == qual_a.lengths().tolist() + [len(extra)]
    got, want = qual_b.get(0, n), qual_a.get()
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (name, k)
    g = qual_b.get(n, n + 1)
    assert not g["depth"].any() and (g["agree"] == weight).all() and (g["src"] == np.arange(len(extra))).all()
    if name == "tile_edges":                                                     # the input is what it is named for
        src = want["src"]
        assert (src[src >= qr.SUP] & 0x7FFFFFFF).tolist() == list(EDGE_INS)
        kept = set((src & 0x7FFFFFFF).tolist())
        assert all(x not in kept for d in EDGE_DEL for x in d)
    elif name == "pile_case":
        src = qual_a.get(vb.PILE_C, vb.PILE_C + 1)["src"]
        assert (src[src >= qr.SUP] & 0x7FFFFFFF).tolist() == sorted(vb.PILE_INS)


# ----------------------------------------------------------------------------- 4: no votes
@pytest.mark.parametrize("weight", vb.NOVOTE_WEIGHTS)
def test_no_votes(ctx, weight):
    texts = list(vb.novote_texts())
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    out, crows, qual = Pileup(ctx, S, weight=weight).evolve_qual()
    assert texts_of(out) == texts and qual.lengths().tolist() == [len(t) for t in texts]
    g = qual.get()
    assert (g["qv"] == {1: 4, 65535: 48}[weight]).all() and not g["depth"].any() and (g["agree"] == weight).all()
    assert (g["src"] == np.concatenate([np.arange(len(t)) for t in texts])).all()
    rows = qual.summary(10)
    assert rows["n_unvoted"].tolist() == rows["len"].tolist() == [len(t) for t in texts] and not rows["n_sup"].any()
    assert rows["n_below"].tolist() == ([len(t) for t in texts] if weight == 1 else [0] * len(texts))


# ----------------------------------------------------------------------------- 5: real pile-ups
@pytest.fixture(scope="module")
def reads_case(ctx):
    texts, _, _ = mixed_reads(401, 402, 250, 3000, 31000, rl_min=2000, extra=2)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, MASK, R, 32, 64, strands=3, reads_rc=Src)
    return dict(texts=texts, S=S, Src=Src, rows=rows)


@pytest.fixture(scope="module")
def reads_evidence(ctx, reads_case):
    """Per weight: the text evolve() gives and qual_ref.evidence of every target's dump at qmax 60, computed once."""
    c, out = reads_case, {}
    for weight in (1, 3):
        plain, twin = twin_piles(ctx, c["S"], lambda p: p.vote(c["rows"], R, reads_rc=c["Src"]), weight)
        got, crows = plain.evolve()
        out[weight] = dict(texts=texts_of(got), crows=crows, want=dumps_evidence(twin, len(c["texts"]), weight), twin=twin)
    return out


@pytest.mark.parametrize("weight", [1, 3])
def test_real_pileups_every_target(ctx, reads_case, reads_evidence, weight):
    e = reads_evidence[weight]
    twin = e["twin"]
    before = twin.dump(7)
    assert status(lambda: twin.evolve_qual(61)) == -1 and status(lambda: twin.evolve_qual(-1)) == -1
    for x, y in zip(before, twin.dump(7)):
        assert (x == y).all()                                                    # refused: the pile-up stays usable
    out, crows, qual = twin.evolve_qual(60)
    assert texts_of(out) == e["texts"] and crows.tobytes() == e["crows"].tobytes()
    assert_evidence(out, qual, e["want"], f"weight {weight}")
    g = qual.get()
    assert (g["src"] >= qr.SUP).any() and g["depth"].max() >= 5 and len(set(g["qv"].tolist())) >= 5    # the input exercises the rule
    assert status(lambda: twin.evolve_qual(60)) == -1                            # spent


@pytest.mark.parametrize("qmax", [0, 10])
def test_real_pileups_at_lower_caps(ctx, reads_case, reads_evidence, qmax):
    c = reads_case
    pile = Pileup(ctx, c["S"], weight=3)
    pile.vote(c["rows"], R, reads_rc=c["Src"])
    want = dumps_evidence(pile, len(c["texts"]), 3, qmax)
    out, _, qual = pile.evolve_qual(qmax)
    assert_evidence(out, qual, want, f"qmax {qmax}")
    full = np.concatenate([w["qv"] for w in reads_evidence[3]["want"]])
    assert (qual.get()["qv"] == np.minimum(full, qmax)).all() and (full > qmax).any()      # the cap bites


# ----------------------------------------------------------------------------- 6: the drivers
def test_correct_reads_qual(ctx, reads_case, reads_evidence):
    c, e = reads_case, reads_evidence[1]
    plain, prow, pst = ctx.correct_reads(c["S"], MASK, R, 32, 64, reads_rc=c["Src"])
    out, rows, st, qual = ctx.correct_reads_qual(c["S"], MASK, R, 32, 64, reads_rc=c["Src"])
    assert texts_of(out) == texts_of(plain) == e["texts"] and rows.tobytes() == prow.tobytes()
    assert [s["n_overlaps"] for s in st] == [s["n_overlaps"] for s in pst]
    assert_evidence(out, qual, e["want"], "default budget")
    lo, hi = 3, 60
    part, prow2, _, pq = ctx.correct_reads_qual(c["S"], MASK, R, 32, 64, t_lo=lo, t_hi=hi, reads_rc=c["Src"], max_boxes=1)
    assert ctx.last_correct_profile()["n_chunks"] == hi - lo                     # one read per chunk
    assert prow2.tobytes() == rows[lo:hi].tobytes()
    assert_evidence(part, pq, e["want"][lo:hi], "one read per chunk")
    whole = qual.get(lo, hi)
    assert all((whole[k] == pq.get()[k]).all() for k in KEYS)
    assert status(lambda: ctx.correct_reads_qual(c["S"], MASK, R, 32, 64, reads_rc=c["Src"], qmax=61)) == -1


@pytest.fixture(scope="module")
def polish_expect(ctx):
    """polish_case: the text of polish_contigs at rounds = 2 and the last round made by hand -- rounds = 1, then map -> Pileup
    -> vote_mapped -> dump."""
    contigs, reads = polish_case(701)
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    Rc = ctx.seqs_revcomp(Rd)
    two, rows2, log2 = ctx.polish_contigs(T, Rd, MASK, R, overlap_min=OVERLAP_MIN, rounds=2, reads_rc=Rc)
    one, _, _ = ctx.polish_contigs(T, Rd, MASK, R, overlap_min=OVERLAP_MIN, rounds=1, reads_rc=Rc)
    pile = Pileup(ctx, one)
    pile.vote_mapped(Rd, map_rows(ctx, one, Rd, reads_rc=Rc), R, OVERLAP_MIN, reads_rc=Rc)
    want = dumps_evidence(pile, len(contigs), 1)
    return dict(T=T, Rd=Rd, Rc=Rc, texts=texts_of(two), rows=rows2, log=log2, want=want)


@pytest.mark.parametrize("max_boxes", [0, 1])
def test_polish_contigs_qual(ctx, polish_expect, max_boxes):
    p = polish_expect
    out, rows, log, qual = ctx.polish_contigs_qual(p["T"], p["Rd"], MASK, R, overlap_min=OVERLAP_MIN, rounds=2, reads_rc=p["Rc"],
                                                   max_boxes=max_boxes)
    assert texts_of(out) == p["texts"] == [w["text"] for w in p["want"]] and rows.tobytes() == p["rows"].tobytes()
    for k in ("round", "n_mapped", "n_voted", "n_bases_in", "n_bases_out"):
        assert log[k].tolist() == p["log"][k].tolist(), k
    assert (log["n_chunks"] == (sum(1 for n in POLISH_LENS) if max_boxes else 1)).all()    # one contig per range
    assert_evidence(out, qual, p["want"], f"max_boxes {max_boxes}")
    assert qual.lengths().tolist()[0] == 0 and (qual.get(1, 2)["depth"] == 0).all()         # the empty contig; the one without rows


def test_layout_consensus_qual(ctx):
    texts = noisy_reads(NOISY_SEED)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, MASK, R, 32, 64, reads_rc=Src)
    lay = ctx.layout(S, rows, 64, 2)
    plain, prow, pst = ctx.layout_consensus(lay, S, rows, R, OVERLAP_MIN, 1, 0)
    contigs = lay.stitch(S)
    pile = Pileup(ctx, contigs)
    pile.vote_placed(S, lay.place(S, rows), R, OVERLAP_MIN, reads_rc=Src)
    want = dumps_evidence(pile, contigs.count, 1)
    assert contigs.count >= 2
    for max_boxes in (0, 1):
        out, rows_out, st, qual = ctx.layout_consensus_qual(lay, S, rows, R, OVERLAP_MIN, 1, max_boxes)
        assert texts_of(out) == texts_of(plain) and rows_out.tobytes() == prow.tobytes()
        assert st["n_voted"] == pst["n_voted"] and st["n_chunks"] == (contigs.count if max_boxes else 1)
        assert_evidence(out, qual, want, f"layout max_boxes {max_boxes}")


# ----------------------------------------------------------------------------- 7: summary and spans
def runs_to_qv(length, runs, rng, qmin=20):
    """qv of one sequence: below qmin exactly on the runs [beg, end)"""
    q = rng.integers(qmin, 94, length).astype(np.uint8)
    for b, e in runs:
        q[b:e] = rng.integers(0, qmin, e - b)
    return q


def span_case(seed=77):
    """(lengths, qv, depth, src): runs of 7 bases that begin and that end at 63 / 64 / 65, 255 / 256 / 257 and 4 095 / 4 096 /
    4 097, one run across three tiles, a run through a sequence's last base with the next sequence starting low, empty
    sequences in between, all low, none low, a 70 001-base sequence and 300 fuzzed ones."""
    rng = np.random.default_rng(seed)
    seqs = []
    for e in (63, 64, 65, 255, 256, 257, 4095, 4096, 4097):
        seqs.append((4500, [(e, e + 7)]))
        seqs.append((4500, [(e - 7, e)]))
        seqs.append((0, []))
    seqs.append((13000, [(4000, 8300)]))                                         # tiles 0, 1 and 2
    seqs.append((300, [(290, 300)]))
    seqs.append((200, [(0, 12)]))                                                # two spans, not one
    seqs.append((0, []))
    seqs.append((5000, [(0, 5000)]))
    seqs.append((5000, []))
    seqs.append((1, [(0, 1)]))
    long_runs, at = [], 3
    while at < 69900:
        ln = int(rng.integers(1, 40))
        long_runs.append((at, min(at + ln, 70001)))
        at += ln + int(rng.integers(1, 300))
    long_runs.append((69995, 70001))
    seqs.append((70001, long_runs))
    for _ in range(300):
        ln = int(rng.integers(0, 3000))
        runs, at = [], int(rng.integers(0, 50))
        while at < ln:
            w = int(rng.integers(1, 30))
            runs.append((at, min(at + w, ln)))
            at += w + int(rng.integers(1, 200))
        seqs.append((ln, runs))
    lengths = np.array([s[0] for s in seqs], np.uint32)
    qv = np.concatenate([runs_to_qv(n, runs, rng) for n, runs in seqs])
    total = int(lengths.sum())
    depth = np.where(rng.random(total) < 0.1, 0, rng.integers(0, 65536, total)).astype(np.uint16)
    src = (rng.integers(0, 2 ** 31, total) | np.where(rng.random(total) < 0.05, qr.SUP, 0)).astype(np.uint32)
    n_runs = sum(len(s[1]) for s in seqs)
    return lengths, qv, depth, src, n_runs


def run_span_case(ctx):
    lengths, qv, depth, src, n_runs = span_case()
    agree = (depth // 2).astype(np.uint16)
    q = Qual.from_arrays(ctx, lengths, qv, depth, agree, src)
    assert q.count == len(lengths) and q.lengths().tolist() == lengths.tolist()
    g = q.get()
    assert all((g[k] == w).all() for k, w in zip(KEYS, (qv, depth, agree, src)))
    for qmin in (20, 0, 94, 5):
        got, want = q.summary(qmin), qr.summary(lengths, qv, depth, src, qmin)
        for f in qr.ROW_DTYPE.names:
            assert got[f].tolist() == want[f].tolist(), (qmin, f)
    want = qr.low_spans(lengths, qv, 20, 1)
    assert len(want) == n_runs                                                   # the runs as planted: none merged, none split
    for qmin, min_run in ((20, 1), (20, 7), (20, 8), (20, 4301), (5, 1), (94, 1), (94, 5001), (0, 1)):
        got, want = q.low_spans(qmin, min_run), qr.low_spans(lengths, qv, qmin, min_run)
        assert got.tobytes() == want.tobytes(), (qmin, min_run, len(got), len(want))
    seven, eight = qr.low_spans(lengths, qv, 20, 7), qr.low_spans(lengths, qv, 20, 8)
    edges = [r for r in seven.tolist() if r[0] < 27]
    assert len(edges) == 18 and not [r for r in eight.tolist() if r[0] < 27]    # min_run met, and missed by one
    assert q.summary(20)["n_low_runs"].sum() == n_runs
    want = qr.low_spans(lengths, qv, 20, 1)
    short = q.low_spans(20, 1, cap=5)                                            # cap below n_out: the count still comes back
    assert q.n_low_spans == len(want) and short.tobytes() == want[:5].tobytes()
    none = q.low_spans(20, 1, cap=0)
    assert q.n_low_spans == len(want) and len(none) == 0
    return q


def test_summary_and_low_spans(ctx):
    q = run_span_case(ctx)
    assert status(lambda: q.summary(95)) == -1 and status(lambda: q.summary(-1)) == -1
    assert status(lambda: q.low_spans(95)) == -1 and status(lambda: q.low_spans(20, 0)) == -1
    empty = Qual.from_arrays(ctx, np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    assert empty.count == 0 and len(empty.summary(20)) == 0 and len(empty.low_spans(20)) == 0 and len(empty.get()["qv"]) == 0
    blank = Qual.from_arrays(ctx, np.zeros(3, np.uint32), np.zeros(0, np.uint8))
    assert blank.summary(20)["min_qv"].tolist() == [-1, -1, -1] and len(blank.low_spans(94)) == 0
    dflt = Qual.from_arrays(ctx, [3, 2], [1, 2, 3, 4, 5])                        # depth, agree: 0; src: the position in its sequence
    g = dflt.get()
    assert g["src"].tolist() == [0, 1, 2, 0, 1] and not g["depth"].any() and not g["agree"].any()
    assert status(lambda: Qual.from_arrays(ctx, [2], [93, 94])) == -1


# ----------------------------------------------------------------------------- 8: FASTQ
FQ_LENS = (5, 0, 63, 64, 65, 1, 200, 129)


def fastq_case(ctx, seed=88):
    rng = np.random.default_rng(seed)
    texts = [rng.choice(np.frombuffer(b"ACGT", np.uint8), n).tobytes() for n in FQ_LENS]
    quals = [rng.integers(0, 94, n).astype(np.uint8) for n in FQ_LENS]
    quals[0][:] = (0, 93, 31, 26, 10)                                            # '!', '~', '@', ';', '+': what a parser could trip on
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    q = Qual.from_arrays(ctx, [len(t) for t in texts], np.concatenate(quals))
    return texts, quals, S, q


def run_fastq_case(ctx):
    texts, quals, S, q = fastq_case(ctx)
    names = [f"read{k} len={len(t)}" for k, t in enumerate(texts)]
    img = S.write_fastq(q)
    assert img == qr.fastq_image(texts, quals)
    assert S.write_fastq(q, names=names) == qr.fastq_image(texts, quals, names)
    assert S.write_fastq(q, lo=1, hi=5) == qr.fastq_image(texts[1:5], quals[1:5], first_id=1)           # begins with the empty one
    assert S.write_fastq(q, names=names[6:], lo=6) == qr.fastq_image(texts[6:], quals[6:], names[6:])
    assert S.write_fastq(q, lo=3, hi=3) == b""
    back, index = ctx.seqs_from_fastx(S.write_fastq(q, names=names))
    assert texts_of(back) == texts and index.names(S.write_fastq(q, names=names)) == [n.split()[0] for n in names]
    assert back.write_fasta(width=0) == S.write_fasta(width=0)
    named = S.write_fastq(q, names=names)
    for r, ql in zip(index.recs(), quals):
        assert named[int(r["qual_off"]):int(r["qual_off"]) + len(ql)] == bytes(int(x) + 33 for x in ql)
    return img


def test_fastq(ctx):
    img = run_fastq_case(ctx)
    texts, quals, S, q = fastq_case(ctx)
    size = C.c_uint64()
    assert ctx.lib.pba_seqs_write_fastq(ctx.h, S.h, q.h, 0, S.count, None, None, None, 0, C.byref(size)) == 0 and size.value == len(img)
    buf = np.full(len(img) + 8, 0xEE, np.uint8)
    size = C.c_uint64()
    assert ctx.lib.pba_seqs_write_fastq(ctx.h, S.h, q.h, 0, S.count, None, None, C.c_void_p(buf.ctypes.data), len(img) - 1, C.byref(size)) == -1
    assert size.value == len(img) and (buf == 0xEE).all()                       # one short: the size, and nothing written
    assert ctx.lib.pba_seqs_write_fastq(ctx.h, S.h, q.h, 0, S.count, None, None, C.c_void_p(buf.ctypes.data), len(img), C.byref(size)) == 0
    assert buf[:len(img)].tobytes() == img and (buf[len(img):] == 0xEE).all()
    lens = [len(t) for t in texts]
    other = Qual.from_arrays(ctx, lens[:-1] + [lens[-1] + 1], np.zeros(sum(lens) + 1, np.uint8))
    fewer = Qual.from_arrays(ctx, lens[:-1], np.zeros(sum(lens[:-1]), np.uint8))
    assert status(lambda: S.write_fastq(other)) == -1 and status(lambda: S.write_fastq(fewer)) == -1


def test_fastq_of_an_evolved_set(ctx):
    """The product end to end: the pile case's contigs with their own evidence, out as FASTQ and read back."""
    contigs, reads, rows = vb.pile_case()
    S = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    pile = Pileup(ctx, S)
    pile.vote_mapped(Rd, rows, vb.R, vb.OVERLAP_MIN)
    out, _, qual = pile.evolve_qual()
    img = out.write_fastq(qual, names=["a", "b", "c"])
    g = [qual.get(t, t + 1)["qv"] for t in range(3)]
    assert img == qr.fastq_image(texts_of(out), g, ["a", "b", "c"])
    back, _ = ctx.seqs_from_fastx(img)
    assert texts_of(back) == texts_of(out)


# ----------------------------------------------------------------------------- 9: scribbled work buffers
@pytest.mark.parametrize("byte", [0x00, 0xFF])
def test_over_scribbled_buffers(ctx, byte):
    """One case each of the write pass, summary / spans and FASTQ with every kept buffer of the ctx overwritten first: what a
    new entry point finds in a kept buffer is undefined."""
    for run in (run_pile_case, run_span_case, run_fastq_case):
        run(ctx)                                                                 # (the buffers exist and have their sizes)
        ctx.scribble(byte)
        run(ctx)
