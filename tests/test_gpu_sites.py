"""Variant sites from pile-ups and every row's allele at each site, on the device: the scan (k_sites_flag, k_sites_write) against
tests/sites_ref.py over Pileup.dump on hand-built states at the edges of its bitmap words; the AlleleSink of the traced
bit-vector pass (k_allele_pairs) against sites_ref over the scripts pba_align_batch_trace gives for the same pairs, at the
edges of its 64-op groups; the invariant that ties the two together (the allele records of all rows plus the target's own
weight ARE the boxes); the refusals; caller-owned streams and scribbled kept buffers; the planted diploid end to end.  Every
comparison is exact.  The inputs are held to their conditions without a GPU in tests/test_sites_cpu.py.  Needs a real MI355X
(-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cigar_ref as cr
import sites_inputs as si
import sites_ref as sr
from conftest import MASK_PAT, ROOT
from correct_helpers import mixed_reads, rc
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import ALLELE_DTYPE, PAIR_DTYPE, SITE_DTYPE, PbaError, Pileup
from polish_helpers import polish_case

pytestmark = pytest.mark.gpu
FIELDS = SITE_DTYPE.names
R = si.R


def status(call):
    with pytest.raises(PbaError) as e:
        call()
    return e.value.status


def texts_of(S):
    return [S.get_text(k) for k in range(S.count)]


def ref_sites(pile, texts, th, weight=1):
    """sites_ref over the dump of every target of a live pile-up"""
    parts = [sr.sites_of(*pile.dump(t), texts[t], weight, th, t) for t in range(pile.t_lo, pile.t_hi)]
    return np.concatenate(parts) if parts else np.zeros(0, sr.SITE)


def same_sites(got, want):
    assert got.size == want.size, (got.size, want.size)
    for f in FIELDS:
        assert (got[f] == want[f]).all(), (f, np.flatnonzero(got[f] != want[f])[:5])


def check_object(sites, want, t_lo, t_hi):
    """count, the records, every target's range, a partial get"""
    assert sites.count == want.size
    got = sites.get()
    same_sites(got, want)
    for t in range(t_lo, t_hi):
        lo, hi = sites.target_range(t)
        assert (lo, hi) == (int(np.searchsorted(want["target"], t, "left")), int(np.searchsorted(want["target"], t, "right"))), t
    if want.size >= 3:
        same_sites(sites.get(1, want.size - 1), want[1:-1])
    return got


# ----------------------------------------------------------------------------- the scan
@pytest.fixture(scope="module")
def scan_world(ctx):
    targets, reads, rows, want_sel, want_sup = si.scan_case()
    S, Rd = ctx.seqs_from_list(targets, strict_acgt=True), ctx.seqs_from_list(reads, strict_acgt=True)
    return dict(targets=targets, reads=reads, rows=rows, S=S, Rd=Rd, sel=want_sel, sup=want_sup)


def voted_pile(ctx, w, weight=1, t_lo=0, t_hi=None):
    pile = Pileup(ctx, w["S"], t_lo, t_hi, weight=weight)
    rows = w["rows"][(w["rows"]["contig"] >= pile.t_lo) & (w["rows"]["contig"] < pile.t_hi)]
    _, n = pile.vote_placed(w["Rd"], rows, R, 64)
    assert n == rows.size
    return pile


@pytest.mark.parametrize("weight", (1, 3))
def test_scan_hand_built_states(ctx, scan_world, weight):
    """sites at a target's first and last box, at arena offsets 63 / 64 / 65 mod 64 where a bitmap word straddles two targets, a
    target with none, an empty target, 200 consecutive sites, both kinds on one box, a DEL allele -- under three threshold sets;
    the scanned pile-up dumps and evolves to what a twin that was never scanned gives; the object outlives the pile-up"""
    w = scan_world
    pile, twin = voted_pile(ctx, w, weight), voted_pile(ctx, w, weight)
    nt = len(w["targets"])
    kept = None
    for th in (si.STRICT, si.LOOSE, (8, 3, 200), (11 + weight, 1, 0), (1, 1, 1000)):
        want = ref_sites(twin, w["targets"], th, weight)
        sites = pile.sites(*th)
        got = check_object(sites, want, 0, nt)
        if th == si.STRICT:                                      # (weight 3: 3 of N = 12, the share at equality)
            for t in range(nt):
                assert [int(s["pos"]) for s in got if s["target"] == t and s["kind"] == sr.SEL] == w["sel"][t]
                assert [int(s["pos"]) for s in got if s["target"] == t and s["kind"] == sr.SUP] == w["sup"][t]
            kept = (sites, want)
        elif th == si.LOOSE:
            t, lo, hi = si.SCAN_RUN
            run = [int(s["pos"]) for s in got if s["target"] == t and s["kind"] == sr.SEL]
            assert run == list(range(lo, hi)) and got.size > 200
            sites.close()
        else:
            assert (got.size > 0) == (th == (8, 3, 200))         # deeper than any box; a second allele cannot hold all of N
            sites.close()
    for t in range(nt):                                          # the pile-up was only read
        for x, y in zip(pile.dump(t), twin.dump(t)):
            assert (x == y).all(), t
    out, crows = pile.evolve()
    out2, crows2 = twin.evolve()
    assert texts_of(out) == texts_of(out2) and (crows == crows2).all()
    pile.close()
    same_sites(kept[0].get(), kept[1])                           # after the pile-up's evolve and destroy
    kept[0].close()


def test_scan_target_subrange(ctx, scan_world):
    """a pile-up of targets [1, 5): the arena starts at target 1, the records name the set's own target ids"""
    w = scan_world
    pile = voted_pile(ctx, w, 1, 1, 5)
    want = ref_sites(pile, w["targets"], si.STRICT)
    sites = pile.sites(*si.STRICT)
    got = check_object(sites, want, 1, 5)
    assert sorted(set(got["target"].tolist())) == [1, 3]
    with pytest.raises(PbaError):
        sites.target_range(0)
    with pytest.raises(PbaError):
        sites.target_range(5)


def test_scan_long_contig(ctx):
    """one contig of 70 001 bases, its boxes filled tile by tile: sites at 4 095 / 4 096 and 65 535 / 65 536"""
    T, reads, rows = si.long_case()
    S, Rd = ctx.seqs_from_list([T], strict_acgt=True), ctx.seqs_from_list(reads, strict_acgt=True)
    pile = Pileup(ctx, S)
    _, n = pile.vote_placed(Rd, rows, R, 64)
    assert n == len(reads)
    sites = pile.sites(*si.STRICT)
    got = check_object(sites, ref_sites(pile, [T], si.STRICT), 0, 1)
    assert got["pos"].tolist() == list(si.LONG_SITES) and (got["kind"] == sr.SEL).all()


# ----------------------------------------------------------------------------- the sink
def sel_tables(recs):
    """{target: (its SEL positions, their record indices)}"""
    out = {}
    for x, s in enumerate(recs):
        if int(s["kind"]) == sr.SEL:
            p, i = out.setdefault(int(s["target"]), ([], []))
            p.append(int(s["pos"])); i.append(x)
    return out


def want_records(ops, b, a_pos, back, tab):
    pos, idx = tab if tab else ([], [])
    return [(idx[k], a) for k, a in sr.alleles_from_script(ops, b, a_pos, back, pos)]


@pytest.fixture(scope="module")
def sink_world(ctx):
    """the rows of sites_inputs.sink_case with the cost and matlens of their traces, the scripts, the sites chosen from them"""
    texts, rows, tags = si.sink_case()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    pairs = [si.row_pair(r, texts) for r in rows]
    res, ops = [None] * rows.size, [None] * rows.size
    for strand, B in ((1, S), (-1, Src)):
        ks = [k for k in range(rows.size) if int(rows[k]["strand"]) == strand]
        out, scripts = ctx.align_batch_trace(S, B, np.array([pairs[k][0] for k in ks], PAIR_DTYPE), R)
        for k, o, sc in zip(ks, out, scripts):
            res[k], ops[k] = o, sc
    assert all(int(o["rc"]) >= 0 for o in res)
    rows = si.fill_rows(rows, res)
    positions = {}
    for k, (pr, a, b, a_pos, back) in enumerate(pairs):
        la = cr.clip(int(pr["a_len"]), int(pr["b_len"]), R)[0]
        positions[int(rows[k]["target"])] = si.choose_sites(tags[k], ops[k], a_pos, back, int(res[k]["matlen_a"]), la, len(texts[int(rows[k]["target"])]))
    recs = si.site_list(texts, positions)
    sites = ctx.sites_create(S, recs.astype(SITE_DTYPE))
    tab = sel_tables(recs)
    want = [want_records(ops[k], pairs[k][2], pairs[k][3], pairs[k][4], tab.get(int(rows[k]["target"]))) for k in range(rows.size)]
    return dict(texts=texts, rows=rows, tags=tags, S=S, Src=Src, res=res, recs=recs, sites=sites, want=want, positions=positions)


def check_rows(got, rows, want, recs, res=None):
    """records, offsets, totals and results of a whole call against the expectation row by row"""
    out, off, sums, gres = got
    assert off.size == rows.size + 1 and int(off[0]) == 0
    for k in range(rows.size):
        o0, o1 = int(off[k]), int(off[k + 1])
        assert [(int(x["site"]), int(x["allele"])) for x in out[o0:o1]] == want[k], (k, want[k][:4])
        t = sr.row_totals(want[k], recs)
        assert {f: int(sums[k][f]) for f in sr.SUM_FIELDS} == t, (k, t)
        if res is not None:
            for f in ("rc", "cost", "matlen_a", "matlen_b"):
                assert int(gres[k][f]) == int(res[k][f]), (k, f)
    assert int(off[-1]) == sum(len(x) for x in want) == out.size


def test_sink_at_the_edges_of_the_walk(ctx, sink_world):
    """sites at a-elements 0 and matlen_a - 1, one past the covered span, at the 63rd / 64th / 65th op from the goal, two and
    sixty-four in one op group and a group with none, on DELETEs, on dir -1 and strand -1 rows, the row-sweep corner, a row
    whose target has no site (bound 0): records in ascending site order, totals, results"""
    w = sink_world
    check_object(w["sites"], w["recs"], 0, len(w["texts"]))
    got = ctx.overlap_alleles(w["S"], w["rows"], R, w["sites"], reads_rc=w["Src"])
    check_rows(got, w["rows"], w["want"], w["recs"], w["res"])
    by_tag = dict(zip(w["tags"], w["want"]))
    assert len(by_tag["copy"]) == 64 and len(by_tag["nosite"]) == 0 and len(by_tag["two"]) == 2 and len(by_tag["tiny"]) == 2
    assert sum(1 for _, a in by_tag["del"] if a == sr.DEL) == 4
    for k, tag in enumerate(w["tags"]):                          # ascending site order whatever the direction
        assert [s for s, _ in w["want"][k]] == sorted(s for s, _ in w["want"][k])
        if tag in ("edges", "back", "minus", "back-minus", "tiny"):
            assert len(w["want"][k]) == len(w["positions"][int(w["rows"][k]["target"])]) - 1      # the one past the span
    # the reversed row order gives the same rows
    back = ctx.overlap_alleles(w["S"], w["rows"][::-1].copy(), R, w["sites"], reads_rc=w["Src"])
    check_rows(back, w["rows"][::-1], w["want"][::-1], w["recs"], w["res"][::-1])


def test_sink_cap_and_budget(ctx, sink_world):
    """cap too small: off complete, the records cut at a row boundary and nothing behind them written; the _budget form at
    one row per chunk gives the same bytes"""
    w = sink_world
    rows, n = w["rows"], w["rows"].size
    whole = ctx.overlap_alleles(w["S"], rows, R, w["sites"], reads_rc=w["Src"])
    one = ctx.overlap_alleles(w["S"], rows, R, w["sites"], reads_rc=w["Src"], max_slots=1)
    for x, y in zip(whole, one):
        assert x.tobytes() == y.tobytes()
    off = whole[1]
    cut = next(k for k in range(n) if int(off[k + 1]) > int(off[k]) and k >= 3)      # the first row that does not fit
    cap = int(off[cut + 1]) - 1
    out = np.zeros(cap + 1, ALLELE_DTYPE)
    out["site"], out["allele"] = 0xDEADBEEF, 0xDEADBEEF
    off2, total = np.zeros(n + 1, np.uint64), eng.C.c_uint64()
    sums, res = np.zeros(n, eng.ALLELE_COUNTS_DTYPE), np.zeros(n, eng.RESULT_DTYPE)
    st = ctx.lib.pba_overlap_rows_alleles(ctx.h, w["S"].h, w["Src"].h, rows.ctypes.data, n, R, w["sites"].h, out.ctypes.data, cap,
                                          off2.ctypes.data, eng.C.byref(total), sums.ctypes.data, res.ctypes.data)
    assert st == 0 and (off2 == off).all() and total.value == int(off[-1])
    fit = int(off[cut])
    assert out[:fit].tobytes() == whole[0][:fit].tobytes() and (out["site"][fit:] == 0xDEADBEEF).all()
    assert sums.tobytes() == whole[2].tobytes()
    got = ctx.overlap_alleles(w["S"], rows, R, w["sites"], reads_rc=w["Src"], cap=cap)
    assert got[0].tobytes() == whole[0][:fit].tobytes() and (got[1] == off).all()


# ----------------------------------------------------------------------------- the two sinks tied together
def check_invariant(pile, sites, recs, texts, out, off, sums, weight):
    """for every SEL site, the histogram of the allele records over all rows plus `weight` on own equals the five counts of the
    dumped box; every row's n_sites is its record count"""
    assert (sums["n_sites"] == np.diff(off.astype(np.int64))).all()
    assert (sums["n_major"] + sums["n_minor"] + sums["n_other"] == sums["n_sites"]).all()
    h = sr.histogram(recs.size, [(int(x["site"]), int(x["allele"])) for x in out])
    boxes = {}
    n_sel = 0
    for x, s in enumerate(recs):
        if int(s["kind"]) != sr.SEL:
            assert not h[x].any()                                # SUP sites get no per-row record
            continue
        t = int(s["target"])
        if t not in boxes:
            sel, _, tot = pile.dump(t)
            boxes[t] = sr.box_counts(sel, tot, weight)
        h[x, int(s["own"])] += weight
        assert h[x].tolist() == boxes[t][int(s["pos"])].tolist(), (x, s)
        n_sel += 1
    return n_sel


def test_invariant_overlap_pileup(ctx):
    """a both-strand all-vs-all pile-up under weight 2: the rows that voted, walked again by the allele sink"""
    texts, _, flip = mixed_reads(431, 432, 70, 1200, 7000, rl_min=800, extra=1)
    assert flip.any() and not flip.all()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, eng.mask_from_pattern(MASK_PAT), R, 32, 64, strands=3, reads_rc=Src)
    assert rows.size >= 100 and {1, -1} <= set(rows["strand"].tolist())
    pile = Pileup(ctx, S, weight=2)
    pile.vote(rows, R, Src)
    sites = pile.sites(4, 2, 200)
    recs = check_object(sites, ref_sites(pile, texts, (4, 2, 200), 2), 0, len(texts))
    out, off, sums, res = ctx.overlap_alleles(S, rows, R, sites, reads_rc=Src)
    assert (res["rc"] >= 0).all() and (res["cost"] == rows["cost"]).all()
    n_sel = check_invariant(pile, sites, recs, texts, out, off, sums, 2)
    assert n_sel >= 50 and out.size >= 200 and (recs["kind"] == sr.SUP).any()


def test_invariant_mapped_pileup(ctx):
    """a mapped pile-up: the voting roles of every row under vote_mapped's gate; rows that are not found, or miss the gate,
    leave nothing"""
    contigs, reads = polish_case(701)
    T, Rd = ctx.seqs_from_list(contigs, strict_acgt=True), ctx.seqs_from_list(reads, strict_acgt=True)
    Rc = ctx.seqs_revcomp(Rd)
    ix = ctx.index_build_set(T, eng.mask_from_pattern(MASK_PAT))
    rows, _ = ctx.map_reads(ix, T, Rd, R, strands=3, reads_rc=Rc)
    pile = Pileup(ctx, T)
    vres, n_voted = pile.vote_mapped(Rd, rows, R, 64, Rc)
    sites = pile.sites(4, 2, 200)
    recs = check_object(sites, ref_sites(pile, contigs, (4, 2, 200)), 0, len(contigs))
    out, off, sums, res = ctx.map_alleles(T, Rd, rows, R, sites, 64, reads_rc=Rc)
    assert res.tobytes() == vres.tobytes()
    gate = (rows["found"] != 0) & (res["rc"] >= 0) & (res["matlen_a"] >= 64)
    assert int(gate.sum()) == n_voted and (rows["found"] == 0).any() and ((rows["found"] != 0) & ~gate).any()
    assert not sums["n_sites"][~gate].any() and not sums["n_own"][~gate].any()
    n_sel = check_invariant(pile, sites, recs, contigs, out, off, sums, 1)
    assert n_sel >= 10 and out.size >= 50


# ----------------------------------------------------------------------------- refusals
def test_refusals(ctx, scan_world, sink_world):
    w, k = scan_world, sink_world
    pile = voted_pile(ctx, w)
    before = [pile.dump(t) for t in range(len(w["targets"]))]
    for th in ((0, 1, 0), (1, 0, 0), (1, 1, -1), (1, 1, 1001)):
        assert status(lambda: pile.sites(*th)) == -1
    other = ctx.seqs_from_list([t + b"A" for t in w["targets"]], strict_acgt=True)
    h = eng.C.c_void_p()
    assert ctx.lib.pba_pileup_sites(ctx.h, pile.h, other.h, 4, 2, 250, eng.C.byref(h)) == -1 and not h.value
    for t, b in enumerate(before):                               # nothing changed
        for x, y in zip(pile.dump(t), b):
            assert (x == y).all()
    pile.evolve()
    assert status(lambda: pile.sites(*si.STRICT)) == -1          # spent
    # pba_sites_create: unsorted, a duplicate, outside its sequence, outside the range, a bad kind, a bad code
    good = k["recs"].astype(SITE_DTYPE)
    S = k["S"]
    bad = []
    x = good.copy(); x[[0, 1]] = x[[1, 0]]; bad.append(x)
    x = good.copy(); x[1] = x[0]; bad.append(x)
    x = good.copy(); x["pos"][-1] = len(k["texts"][int(x["target"][-1])]); bad.append(x)
    x = good.copy(); x["pos"][0] = -1; bad.append(x)
    x = good.copy(); x["target"][-1] = S.count; bad.append(x)
    x = good.copy(); x["kind"][2] = 3; bad.append(x)
    x = good.copy(); x["own"][2] = 4; bad.append(x)
    x = good.copy(); x["minor"][2] = 5; bad.append(x)
    for x in bad:
        assert status(lambda: ctx.sites_create(S, x)) == -1
    assert status(lambda: ctx.sites_create(S, good[good["target"] >= 2], 2, S.count + 1)) == -1
    sub = ctx.sites_create(S, good[good["target"] >= 2], 2)     # a range of its own
    assert sub.count == int((good["target"] >= 2).sum()) and ctx.sites_create(S, good[:0]).count == 0
    # sites made from another set, and rows whose target lies outside the range of the sites
    rows = k["rows"]
    assert status(lambda: ctx.overlap_alleles(S, rows, R, pile_sites_of_other(ctx, w), reads_rc=k["Src"])) == -1
    assert status(lambda: ctx.overlap_alleles(S, rows, R, sub, reads_rc=k["Src"])) == -1
    assert ctx.overlap_alleles(S, rows[rows["target"] >= 2], R, sub, reads_rc=k["Src"])[0].size > 0
    wrong = rows.copy(); wrong["cost"][0] += 1                   # held to its row
    assert status(lambda: ctx.overlap_alleles(S, wrong, R, k["sites"], reads_rc=k["Src"])) == -1
    assert status(lambda: ctx.overlap_alleles(S, rows, R, k["sites"])) == -1      # a strand -1 row needs reads_rc
    check_rows(ctx.overlap_alleles(S, rows, R, k["sites"], reads_rc=k["Src"]), rows, k["want"], k["recs"])   # and all is as it was


def pile_sites_of_other(ctx, w):
    return ctx.sites_create(w["S"], np.zeros(0, SITE_DTYPE))


# ----------------------------------------------------------------------------- streams and stale buffers
def scan_and_alleles(ctx, w, k):
    pile = voted_pile(ctx, w)
    sites = pile.sites(*si.STRICT)
    recs = sites.get()
    got = ctx.overlap_alleles(k["S"], k["rows"], R, k["sites"], reads_rc=k["Src"], max_slots=40)
    return [recs.tobytes()] + [x.tobytes() for x in got]


def test_caller_stream_and_scribbled_buffers(ctx, scan_world, sink_world):
    """one pass of scan plus alleles on a caller-owned stream, one after every kept buffer was scribbled: the plain run's bytes"""
    import torch
    plain = scan_and_alleles(ctx, scan_world, sink_world)
    s = torch.cuda.Stream()
    try:
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            assert scan_and_alleles(ctx, scan_world, sink_world) == plain
    finally:
        ctx.set_stream(None)
    ctx.scribble(0xA5)
    assert scan_and_alleles(ctx, scan_world, sink_world) == plain


# ----------------------------------------------------------------------------- the planted diploid
def test_planted_diploid(ctx):
    """300 reads of 2 kb from two haplotypes mapped to haplotype 0: the sites found are sites_ref's and the planted ones; every
    row's records are what its voting pair's script says, and the reads carry their own haplotype's allele"""
    D = sr.DIPLOID
    h0, h1, reads, hap_of, planted = sr.planted_diploid()
    T, Rd = ctx.seqs_from_list([h0], strict_acgt=True), ctx.seqs_from_list(reads, strict_acgt=True)
    Rc = ctx.seqs_revcomp(Rd)
    ix = ctx.index_build_set(T, eng.mask_from_pattern(MASK_PAT))
    rows, _ = ctx.map_reads(ix, T, Rd, D["R"], strands=3, reads_rc=Rc)
    pile = Pileup(ctx, T, weight=D["weight"])
    _, n_voted = pile.vote_mapped(Rd, rows, D["R"], D["overlap_min"], Rc)
    assert n_voted >= 0.95 * len(reads)
    sites = pile.sites(*D["thresholds"])
    recs = check_object(sites, ref_sites(pile, [h0], D["thresholds"], D["weight"]), 0, 1)
    sr.planted_conditions(recs, planted)
    out, off, sums, res = ctx.map_alleles(T, Rd, rows, D["R"], sites, D["overlap_min"], reads_rc=Rc)
    tab = sel_tables(recs)[0]
    agree = total = 0
    for strand, B in ((1, Rd), (-1, Rc)):
        ks = [k for k in range(rows.size) if rows[k]["found"] and int(rows[k]["strand"]) == strand]
        pairs = np.array([eng.map_row_pair(rows[k], len(h0), len(reads[k]), D["R"]) for k in ks], PAIR_DTYPE)
        tres, scripts = ctx.align_batch_trace(T, B, pairs, D["R"])
        for k, pr, o, ops in zip(ks, pairs, tres, scripts):
            assert int(rows[k]["read"]) == k
            q = reads[k] if strand == 1 else rc(reads[k])
            b = q[int(pr["b_pos"]):int(pr["b_pos"]) + int(pr["b_len"])]
            voted = int(o["rc"]) >= 0 and int(o["matlen_a"]) >= D["overlap_min"]
            want = want_records(ops, b, int(pr["a_pos"]), False, tab) if voted else []
            got = [(int(x["site"]), int(x["allele"])) for x in out[int(off[k]):int(off[k + 1])]]
            assert got == want, k
            for s, a in got:
                p = int(recs[s]["pos"])
                if p in planted:
                    total += 1
                    agree += a == planted[p][1 + hap_of[k]]
    print("records at planted sites", total, "carrying their haplotype's allele", agree)
    assert total >= 10 * len(planted) and agree >= 0.9 * total
    check_invariant(pile, sites, recs, [h0], out, off, sums, D["weight"])


def test_bench_sites_tool():
    """tools/bench_sites.py on 600 reads x 3 kb: one JSON line with the scan next to evolve and the allele walk next to the window
    walk; the planted differences of the two haplotypes show as sites"""
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "bench_sites.py"), "--reads", "600", "--len",
                        "3000", "--het", "500", "--reps", "2", "--scan-reps", "2"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    print(lines[0])
    for k in ("scan_ms", "evolve_ms", "alleles_ms", "windows_ms"):
        assert 0 < out[k]["min"] <= out[k]["median"] <= out[k]["max"], k
    assert out["boxes"] == 600 * 3000 and out["rows"] > 300 and out["scan_gb_per_s"] > 0
    assert out["sel_sites"] > 0 and out["allele_records"] > out["sel_sites"] and out["alleles_rows_per_s"] > 0 < out["windows_rows_per_s"]
