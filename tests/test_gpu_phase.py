"""Overlap rows phased by their alleles, and reads corrected from their own copy, on the device: the phase kernels
(k_phase_classify, k_phase_rows, k_phase_orient) against tests/phase_ref.py on hand cases, at the edges of a wavefront's 64
records, on shared and lonely sites, interleaved targets and a seeded fuzz; pba_overlap_rows_phase against pba_overlap_rows_alleles
followed by pba_alleles_phase; pba_correct_reads_phased against the CPU oracle's composition, however the range is cut, and
against pba_correct_reads where no site is found; the refusals; caller-owned streams and scribbled kept buffers; the tool.  Every
comparison is exact.  The rule is pinned by hand without a GPU in tests/test_phase_cpu.py.  Needs a real MI355X (-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import phase_ref as pr
import sites_ref as sr
from conftest import MASK_PAT, ROOT
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import ALLELE_DTYPE, SITE_DTYPE, PbaError, Pileup

pytestmark = pytest.mark.gpu
A, C, G, T, DEL = 0, 1, 2, 3, 4
PARAM_GRID = [(n_iter, mm, w) for n_iter in (0, 1, 2, 5) for mm in (1, 3) for w in (0, 2)]
COUNTS = pr.STAT_FIELDS


def status(call):
    with pytest.raises(PbaError) as e:
        call()
    return e.value.status


def same(got, want_rows, want_sites, want_stats):
    rows, sites, st = got[:3]
    assert rows.size == want_rows.size
    for f in pr.ROW.names:
        assert (rows[f] == want_rows[f]).all(), (f, np.flatnonzero(rows[f] != want_rows[f])[:5])
    if sites is not None:
        assert sites.size == want_sites.size
        for f in pr.SITE.names:
            assert (sites[f] == want_sites[f]).all(), (f, np.flatnonzero(sites[f] != want_sites[f])[:5])
    assert {k: st[k] for k in COUNTS} == want_stats


# ----------------------------------------------------------------------------- the rule on supplied records
N_SEL = 140          # SEL sites per target: a row of 129 records fits one target


def built_sites(rng):
    """3 targets of 3 000 bases with N_SEL SEL sites each; every third has a SUP record on its box too and a SUP-only box sits
    before every fifth, so that a record index is not a SEL rank; every fourth own is neither major nor minor; DEL minors"""
    recs = []
    for t in range(3):
        for k in range(N_SEL):
            pos = 20 * k + 7
            major = int(rng.integers(0, 5))
            minor = int((major + 1 + rng.integers(0, 4)) % 5)
            own = int(rng.integers(0, 4)) if k % 4 == 3 else (major if (k % 2 == 0 and major < 4) or minor == 4 else minor)
            if k % 5 == 0:
                recs.append((t, pos - 3, sr.SUP, own if own < 4 else 0, major, int(rng.integers(0, 4)), 12, 0, 4))
            recs.append((t, pos, sr.SEL, own if own < 4 else 0, major, minor, 12, 8, 4))
            if k % 3 == 0:
                recs.append((t, pos, sr.SUP, own if own < 4 else 0, major, int(rng.integers(0, 4)), 12, 0, 4))
    return np.array(recs, sr.SITE)


def a_row(rng, sites, sel_of, t, n, must=None, avoid=None):
    """n records on target t: a sorted draw of its SEL records (with `must`, without `avoid`), alleles major / minor / another"""
    pool = [x for x in sel_of[t] if x != must and x != avoid]
    take = sorted(rng.choice(pool, n - (must is not None), replace=False).tolist() + ([must] if must is not None else []))
    out = []
    for x in take:
        u = rng.random()
        s = sites[x]
        a = int(s["major"]) if u < 0.45 else (int(s["minor"]) if u < 0.9 else int((int(s["major"]) + 2) % 5))
        out.append((x, a))
    return out


@pytest.fixture(scope="module")
def rule_world(ctx):
    rng = np.random.default_rng(20261)
    recs = built_sites(rng)
    texts = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 3000)) for _ in range(3)]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    sites = ctx.sites_create(S, recs.astype(SITE_DTYPE))
    sel_of = {t: [x for x, s in enumerate(recs) if int(s["target"]) == t and int(s["kind"]) == sr.SEL] for t in range(3)}
    assert sites.count == recs.size and sites.count_sel == 3 * N_SEL and recs.size > 3 * N_SEL
    rows = {}
    rows["edges"] = [a_row(rng, recs, sel_of, 0, n) for n in (0, 1, 63, 64, 65, 129, 2, 128, 0)]
    shared, lonely = sel_of[1][50], sel_of[1][90]
    rows["shared"] = [a_row(rng, recs, sel_of, 1, int(rng.integers(2, 9)), must=shared, avoid=lonely) for _ in range(500)] + \
                     [a_row(rng, recs, sel_of, 1, 5, must=lonely, avoid=shared)]
    rows["interleaved"] = [a_row(rng, recs, sel_of, (0, 2)[k % 2], int(rng.integers(1, 30))) for k in range(40)]
    rows["fuzz"] = [a_row(rng, recs, sel_of, int(rng.integers(0, 3)), int(rng.integers(0, 80))) for _ in range(200)]
    return dict(S=S, sites=sites, recs=recs, rows=rows, sel_of=sel_of, shared=shared, lonely=lonely)


def hand_cases():
    """the inputs tests/test_phase_cpu.py pins by hand: (site specs (own, major, minor[, kind]), records)"""
    three = [(A, A, C)] * 3
    return [([(A, A, C)], [[], [(0, A)]]),
            ([(A, A, C)], [[(0, C)]]),
            (three, [[(0, A), (1, A), (2, A)], [(0, A), (1, A), (2, T)], [(0, C), (1, C), (2, C)], [(0, C), (1, C)], [(0, A), (1, C)]]),
            (three, [[(0, C), (1, A), (2, A)]]),
            ([(G, A, C), (A, A, C)], [[(0, A), (1, A)]]),
            ([(A, A, DEL), (A, A, G, sr.SUP), (C, DEL, C)], [[(0, DEL), (2, C)], [(0, A), (2, C)], [(0, T), (2, DEL)]]),
            (three, [[(0, A), (1, A), (2, C)], [(0, T), (1, T), (2, A)]])]


def test_hand_cases(ctx, rule_world):
    from test_phase_cpu import sites_of
    S = rule_world["S"]
    for specs, records in hand_cases():
        recs = sites_of(*specs)
        sites = ctx.sites_create(S, recs.astype(SITE_DTYPE))
        for p in PARAM_GRID + [(1, 2, 1), (3, 1, 0), (4, 1, 0)]:
            same(ctx.alleles_phase(sites, records, *p), *pr.phase_ref(recs, records, *p))
        sites.close()


@pytest.mark.parametrize("which", ("edges", "shared", "interleaved", "fuzz"))
def test_rule_on_supplied_records(ctx, rule_world, which):
    """rows of 0 / 1 / 63 / 64 / 65 / 129 records; one site shared by 500 rows and one touched by a single row; rows of two targets
    interleaved; 200 fuzzed rows over 3 targets -- SUP records between the SEL ones throughout -- under n_iter 0, 1, 2, 5,
    min_margin 1, 3 and self_weight 0, 2; without sites_out the rows and stats are the same"""
    w = rule_world
    records = w["rows"][which]
    if which == "shared":
        n_at = lambda x: sum(1 for r in records for s, _ in r if s == x)
        assert n_at(w["shared"]) == 500 and n_at(w["lonely"]) == 1
    moved = 0
    for p in PARAM_GRID:
        want = pr.phase_ref(w["recs"], records, *p)
        same(ctx.alleles_phase(w["sites"], records, *p), *want)
        moved += want[2]["n_flipped_last"]
    assert moved > 0 or which == "edges"                         # the iterations do change orientations on these inputs
    p = (2, 1, 2)
    want = pr.phase_ref(w["recs"], records, *p)
    got = ctx.alleles_phase(w["sites"], records, *p, want_sites=False)
    assert got[1] is None
    same(got, *want)
    assert want[2]["n_same"] > 0 and want[2]["n_other"] > 0


def test_no_rows(ctx, rule_world):
    """n == 0 is legal: the sites keep their seed orientation, score = self_weight * o0"""
    w = rule_world
    for p in ((0, 1, 2), (3, 2, 1)):
        rows, sites, st = ctx.alleles_phase(w["sites"], [], *p)
        want = pr.phase_ref(w["recs"], [], *p)
        same((rows, sites, st), *want)
        assert rows.size == 0 and sites.size == 3 * N_SEL and st["n_flipped_last"] == 0 and not sites["n_agree"].any()
    assert ctx.lib.pba_alleles_phase(ctx.h, w["sites"].h, None, None, 0, eng._ptr(eng._phase_params(1, 1, 1)), None, None, None) == 0


# ----------------------------------------------------------------------------- the planted input
@pytest.fixture(scope="module")
def planted_world(ctx):
    D = pr.PLANTED
    h0, h1, reads, hap_of, planted = sr.planted_diploid(D)
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(reads, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, mask, D["R"], 32, D["overlap_min"], strands=3, reads_rc=Src)
    pile = Pileup(ctx, S, weight=D["weight"])
    pile.vote(rows, D["R"], Src)
    sites = pile.sites(*D["thresholds"])
    pile.close()
    return dict(D=D, reads=reads, hap_of=hap_of, mask=mask, S=S, Src=Src, rows=rows, sites=sites)


def records_of(out, off):
    return [[(int(x["site"]), int(x["allele"])) for x in out[int(off[k]):int(off[k + 1])]] for k in range(off.size - 1)]


def test_overlap_phase_is_alleles_then_phase(ctx, planted_world):
    """the records gathered on the device give what the records fetched to the host and handed to pba_alleles_phase give, and
    what phase_ref gives; one row per chunk gives the same"""
    w = planted_world
    D, S, Src, rows, sites = w["D"], w["S"], w["Src"], w["rows"], w["sites"]
    assert rows.size >= 5000 and sites.count_sel >= 1000
    out, off, _, ares = ctx.overlap_alleles(S, rows, D["R"], sites, reads_rc=Src)
    records = records_of(out, off)
    two = ctx.alleles_phase(sites, records, *pr.PARAMS)
    want = pr.phase_ref(sites.get(), records, *pr.PARAMS)
    same(two, *want)
    whole = ctx.overlap_phase(S, rows, D["R"], sites, *pr.PARAMS, reads_rc=Src)
    same(whole, *want)
    assert whole[3].tobytes() == ares.tobytes() and whole[2]["alleles_ms"] > 0 and whole[2]["phase_ms"] > 0
    assert want[2]["n_same"] > 1000 and want[2]["n_other"] > 1000 and want[2]["n_records"] == out.size
    some = slice(300, 420)                                       # one row per chunk: 120 rows of several targets
    part = ctx.overlap_phase(S, rows[some], D["R"], sites, *pr.PARAMS, reads_rc=Src, max_slots=1)
    same(part, *pr.phase_ref(sites.get(), records[some], *pr.PARAMS))
    again = ctx.overlap_phase(S, rows[some], D["R"], sites, *pr.PARAMS, reads_rc=Src)
    assert again[0].tobytes() == part[0].tobytes() and again[1].tobytes() == part[1].tobytes()
    hap = np.array(w["hap_of"])
    dec = whole[0]["label"] != 0
    right = (whole[0]["label"] > 0) == (hap[rows["target"]] == hap[rows["query"]])
    print("rows", rows.size, "decided", int(dec.sum()), "on hap_of's side", int((dec & right).sum()))
    assert int((dec & right).sum()) * 100 >= 95 * int(dec.sum())


def texts_of(S):
    return [S.get_text(k) for k in range(S.count)]


def test_correct_reads_phased_vs_cpu_composition(ctx, oracle, planted_world):
    """targets [72, 84): text, rows_out and the phase stats are what the CPU oracle's composition gives over the same rows"""
    w = planted_world
    D, S, Src, reads = w["D"], w["S"], w["Src"], w["reads"]
    lo, hi = 72, 84
    got, crows, pst, _ = ctx.correct_reads_phased(S, w["mask"], D["R"], D["thresholds"], *pr.PARAMS, overlap_min=D["overlap_min"],
                                                  weight=D["weight"], t_lo=lo, t_hi=hi, reads_rc=Src)
    tot = dict.fromkeys(COUNTS, 0)
    changed = 0
    for t in range(lo, hi):
        rows_t = w["rows"][w["rows"]["target"] == t]
        o = pr.correct_phased_ref(oracle, reads, t, list(rows_t), D["weight"], D["R"], D["thresholds"], pr.PARAMS)
        text = got.get_text(t - lo)
        assert text == o["text"], t
        assert (int(crows[t - lo]["target"]), int(crows[t - lo]["n_rows"]), int(crows[t - lo]["len_in"]), int(crows[t - lo]["len_out"])) == \
               (t, len(o["kept"]), len(reads[t]), len(text)), t
        changed += o["text"] != o["plain"]
        for k in COUNTS:
            tot[k] += o["stats"][k]
    assert {k: pst[k] for k in COUNTS} == tot and tot["n_other"] > 100 and changed >= 6
    assert ctx.last_correct_profile()["n_rows"] == int(crows["n_rows"].sum())


def test_correct_reads_phased_cuts_and_no_sites(ctx, planted_world):
    """the same answer however the range is cut; with min_depth above every depth no row is labelled and the result is
    pba_correct_reads' byte for byte; without keep_unphased an undecided row does not vote"""
    w = planted_world
    D, S, Src = w["D"], w["S"], w["Src"]
    kw = dict(overlap_min=D["overlap_min"], weight=D["weight"], reads_rc=Src)
    whole, wrows, wst, _ = ctx.correct_reads_phased(S, w["mask"], D["R"], D["thresholds"], *pr.PARAMS, **kw)
    want = texts_of(whole)
    full = ctx.overlap_phase(S, w["rows"], D["R"], w["sites"], *pr.PARAMS, reads_rc=Src)[2]
    assert {k: wst[k] for k in COUNTS} == {k: full[k] for k in COUNTS}
    assert int(wrows["n_rows"].sum()) == wst["n_same"] + wst["n_unphased"]
    for max_boxes in (1, 30000):
        part, prow, pst, _ = ctx.correct_reads_phased(S, w["mask"], D["R"], D["thresholds"], *pr.PARAMS, max_boxes=max_boxes, **kw)
        assert texts_of(part) == want and prow.tobytes() == wrows.tobytes()
        assert {k: pst[k] for k in COUNTS} == {k: wst[k] for k in COUNTS}
        chunks, boxes = 0, None                                  # the greedy take: a chunk holds one read at least
        for x in w["reads"]:
            if boxes is None or boxes + len(x) > max_boxes:
                chunks, boxes = chunks + 1, 0
            boxes += len(x)
        assert ctx.last_correct_profile()["n_chunks"] == chunks and chunks in (S.count, 11, 12)
    plain, prow, _ = ctx.correct_reads(S, w["mask"], D["R"], 32, D["overlap_min"], weight=D["weight"], reads_rc=Src)
    none, nrow, nst, _ = ctx.correct_reads_phased(S, w["mask"], D["R"], (60000, 1, 0), *pr.PARAMS, **kw)
    assert texts_of(none) == texts_of(plain) and nrow.tobytes() == prow.tobytes()
    assert (nst["n_sites"], nst["n_records"], nst["n_unphased"]) == (0, 0, int(prow["n_rows"].sum()))
    assert texts_of(plain) != want
    strict, srow, sst, _ = ctx.correct_reads_phased(S, w["mask"], D["R"], D["thresholds"], *pr.PARAMS, keep_unphased=False, **kw)
    assert int(srow["n_rows"].sum()) == sst["n_same"] == wst["n_same"] and wst["n_unphased"] > 0


# ----------------------------------------------------------------------------- refusals
def test_refusals(ctx, rule_world, planted_world):
    w, k = rule_world, planted_world
    sites, recs = w["sites"], w["recs"]
    good = w["rows"]["interleaved"]
    before = ctx.alleles_phase(sites, good, 2, 1, 1)
    sel0, sel2 = w["sel_of"][0], w["sel_of"][2]
    sup = next(x for x, s in enumerate(recs) if int(s["kind"]) == sr.SUP)
    a = int(recs[sel0[0]]["major"])
    for bad in ([[(recs.size, a)]],                              # beyond the count
                [[(sup, a)]],                                    # a SUP record
                [[(sel0[0], 5)]],                                # an allele beyond DEL
                [[(sel0[3], a), (sel0[2], a)]],                  # not ascending
                [[(sel0[3], a), (sel0[3], a)]],                  # not strictly
                [[(sel0[-1], a), (sel2[0], a)]]):                # two targets in one row
        assert status(lambda: ctx.alleles_phase(sites, bad, 2, 1, 1)) == -1
    for p in ((-1, 1, 1), (eng.PBA_PHASE_MAX_ITER + 1, 1, 1), (1, 0, 1), (1, 1, -1), (1, 1, 65536)):
        assert status(lambda: ctx.alleles_phase(sites, good, *p)) == -1
        assert status(lambda: ctx.overlap_phase(k["S"], k["rows"][:8], k["D"]["R"], k["sites"], *p, reads_rc=k["Src"])) == -1
        assert status(lambda: ctx.correct_reads_phased(k["S"], k["mask"], k["D"]["R"], k["D"]["thresholds"], *p, reads_rc=k["Src"])) == -1
    flat = np.array(good[0] + good[1], ALLELE_DTYPE)
    off = np.array([0, len(good[0]) + len(good[1]), len(good[0])], np.uint64)       # off decreases
    out = np.zeros(2, eng.PHASE_ROW_DTYPE)
    prm = eng._phase_params(1, 1, 1)
    assert ctx.lib.pba_alleles_phase(ctx.h, sites.h, eng._ptr(flat), eng._ptr(off), 2, eng._ptr(prm), eng._ptr(out), None, None) == -1
    assert ctx.lib.pba_alleles_phase(ctx.h, sites.h, eng._ptr(flat), eng._ptr(off), 2, None, eng._ptr(out), None, None) == -1
    assert eng._lib.load().pba_phase_rows_apply(None, None, 3, 1, None) == -1
    # rows: sites made from another set, rows outside the range of the sites, a row that is not a row, a missing reads_rc
    S, Src, rows, R = k["S"], k["Src"], k["rows"], k["D"]["R"]
    assert status(lambda: ctx.overlap_phase(S, rows[:50], R, sites, *pr.PARAMS, reads_rc=Src)) == -1
    sub = ctx.sites_create(S, np.zeros(0, SITE_DTYPE), 10, 20)
    assert status(lambda: ctx.overlap_phase(S, rows[:50], R, sub, *pr.PARAMS, reads_rc=Src)) == -1
    wrong = rows[:50].copy(); wrong["cost"][7] += 1
    assert status(lambda: ctx.overlap_phase(S, wrong, R, k["sites"], *pr.PARAMS, reads_rc=Src)) == -1
    minus = rows[rows["strand"] == -1][:5]
    assert status(lambda: ctx.overlap_phase(S, minus, R, k["sites"], *pr.PARAMS)) == -1
    for th in ((0, 1, 0), (1, 0, 0), (1, 1, 1001)):
        assert status(lambda: ctx.correct_reads_phased(S, k["mask"], R, th, *pr.PARAMS, reads_rc=Src)) == -1
    assert status(lambda: ctx.correct_reads_phased(S, k["mask"], R, k["D"]["thresholds"], *pr.PARAMS, weight=0, reads_rc=Src)) == -1
    # and all is as it was
    after = ctx.alleles_phase(sites, good, 2, 1, 1)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    assert ctx.overlap_phase(S, rows[:50], R, k["sites"], *pr.PARAMS, reads_rc=Src)[0].size == 50


# ----------------------------------------------------------------------------- streams and stale buffers
def one_pass(ctx, w, k):
    D = k["D"]
    a = ctx.alleles_phase(w["sites"], w["rows"]["fuzz"], 3, 1, 1)
    b = ctx.overlap_phase(k["S"], k["rows"][:400], D["R"], k["sites"], *pr.PARAMS, reads_rc=k["Src"], max_slots=64)
    c, crows, cst, _ = ctx.correct_reads_phased(k["S"], k["mask"], D["R"], D["thresholds"], *pr.PARAMS, overlap_min=D["overlap_min"],
                                                t_lo=20, t_hi=40, reads_rc=k["Src"], max_boxes=9000)
    return [a[0].tobytes(), a[1].tobytes(), b[0].tobytes(), b[1].tobytes(), b[3].tobytes(), crows.tobytes()] + texts_of(c) + \
           [{n: x[2][n] for n in COUNTS} for x in (a, b)] + [{n: cst[n] for n in COUNTS}]


def test_caller_stream_and_scribbled_buffers(ctx, rule_world, planted_world):
    """one pass of the three entry points on a caller-owned stream, one after every kept buffer was scribbled: the plain run's
    bytes"""
    import torch
    plain = one_pass(ctx, rule_world, planted_world)
    s = torch.cuda.Stream()
    try:
        ctx.set_stream(s.cuda_stream)
        with torch.cuda.stream(s):
            assert one_pass(ctx, rule_world, planted_world) == plain
    finally:
        ctx.set_stream(None)
    ctx.scribble(0xA5)
    assert one_pass(ctx, rule_world, planted_world) == plain


def test_bench_phase_tool():
    """tools/bench_phase.py on 600 reads x 3 kb: one JSON line with the phase call next to the allele walk, correct_reads_phased
    next to correct_reads, and the share of planted sites each leaves on the read's own haplotype"""
    p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "tools", "bench_phase.py"), "--reads", "600", "--len",
                        "3000", "--het", "500", "--reps", "2"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    print(lines[0])
    for k in ("alleles_ms", "phase_ms", "correct_ms", "correct_phased_ms"):
        assert 0 < out[k]["min"] <= out[k]["median"] <= out[k]["max"], k
    assert out["rows"] > 300 and out["sel_sites"] > 0 and out["rows_same"] > 0 and out["rows_other"] > 0
    assert 0 < out["own_allele_share"]["plain"] <= 1 and 0 < out["own_allele_share"]["phased"] <= 1
