"""The one-lane prefilters (prefilter.h) held to the reference row by row, through the entry points that call them, on the
inputs of prefilter_inputs.py: pairs whose first failing row is every row of 11 .. 64 a seeded pair can fail at, pairs that fail
in one stretch of equal thresholds only, pairs that ride the bound through row 64 and must be reported, the lengths around 32
and 64 on either side, and the thresholds of six R.  Every input's identity is proved from the oracle in the test that runs it.

  prefilter32_planes  k_locate<NB, false / true>: the failing row of every hit goes into the read's band cells, so n_cells tells
                      row f from row f + 1 (per read as well: one call per read); k_spaced_round: verdicts, as n_pairs and rows.
  prefilter32_fails   k_ovl_scan<false / true>: n_prefiltered and n_listed exactly, from an enumeration of every candidate.
  prefilter64         ovl_walk, the form the all-vs-all entry points take (every listed candidate has been through the scan's 32
                      rows, the walk runs rows 33 .. 64 on the first group of an item): rows and n_pairs.

                      test_walk_group_edges: the groups behind the first -- a run followed past its item's end, a run that
                      the next item must skip, a run that starts with the second group -- where nothing is prefiltered.

What this cannot show.  A candidate that passes rows 33 .. 64 falsely goes to the wavefront-wide aligner, which fails it at the
same row: no output row and no counter differs, so for prefilter64 only a false FAIL (a tightrope that goes unreported) and a
miscount are pinned.
Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import align_rings as ar
import map_ref
import prefilter_inputs as pi
from conftest import MASK_PAT
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL, PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP
from test_gpu_parity import prekeep  # noqa: F401  (the three ways the scan sizes the survivors' slices)

pytestmark = pytest.mark.gpu

LOC_COLS = ("nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs")
LOC_CASES = [(R, MASK_PAT) for R in pi.RS] + [(0.07, pi.ALT_PAT), (0.15, pi.ALT_PAT)]
_CACHE = {}


def concat(texts):
    return np.frombuffer(b"".join(texts), np.uint8), np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)


# ----------------------------------------------------------------------------- locate
def locate_expected(oracle, R, pat, NB):
    """the case, the proof of what it is, and the oracle's answer -- once per session"""
    key = ("loc", R, pat, NB)
    if key in _CACHE:
        return _CACHE[key]
    g, texts, meta = pi.locate_case(R, pat, NB)
    reach = pi.reachable(R, pat, True)
    seen, lanes, first, last, between = set(), set(), False, False, False
    for t, mt in zip(texts, meta):
        hits = pi.key_hits(g, t[:16], pat)
        if mt["kind"] == "filler":
            assert hits == []
            continue
        assert hits == [p for p, _, _ in mt["places"]]                         # its one probe hits where it was planted, only
        stopped = []                                                           # per hit: failed within the prefilter's rows?
        for h, (p, kind, f) in enumerate(mt["places"]):
            x = oracle.align(t, g[p:p + 2 * len(t) + 8], R)
            if kind in ("fail", "blip"):
                assert x["rc"] == -1 and x["fail_row"] == f and x["len_a"] == len(t), (mt, x)
                seen.add(f)
            elif kind == "dear":
                assert x["rc"] == -1 and x["fail_row"] > 64, (mt, x)
            else:
                assert x["rc"] > 0 and h == len(mt["places"]) - 1, (mt, x)          # reported, and the read's walk ends there
            stopped.append(x["rc"] == -1 and x["fail_row"] <= 32 and x["len_a"] >= 32)
            if stopped[-1]:
                lanes.add(h % 64)
        if len(stopped) >= 64:
            first, last = first or not stopped[0], last or not stopped[-1]
            between = between or any(a and not b and c for a, b, c in zip(stopped, stopped[1:], stopped[2:]))
    assert seen == set(reach)
    if reach:                                                                  # (R = 0.9: every hit survives)
        assert {0, 31, 32, 63} <= lanes and first and last and between
    assert sorted(len(mt["places"]) for mt in meta if mt["kind"] == "planted" and len(mt["places"]) > 1) in ([64, 65], [64, 65, 65, 130])
    reads, offs = concat(texts)
    garr = np.frombuffer(g, np.uint8)
    mask = eng.mask_from_pattern(pat)
    want, wst = oracle.locator(garr, mask, R, reads, offs, 1, pi.LOC_MIN_LEN, nthreads=8)
    assert wst["n_located"] == sum(mt["kind"] == "planted" and mt["places"][-1][1] in ("tight", "edge10") for mt in meta)
    _CACHE[key] = (g, texts, meta, mask, want, wst)
    return _CACHE[key]


@pytest.mark.parametrize("NB", [1, 2])
@pytest.mark.parametrize("R,pat", LOC_CASES)
def test_prefilter_rows_locate(ctx, oracle, R, pat, NB):
    """k_locate<NB, false>: rows and stats -- n_pairs and n_cells among them -- equal to the oracle's; nothing re-run."""
    g, texts, meta, mask, want, wst = locate_expected(oracle, R, pat, NB)
    T = ctx.seqs_from_list([g], strict_acgt=True)
    Rd = ctx.seqs_from_list(texts, strict_acgt=True)
    ix = ctx.index_build(T, 0, mask, PBA_INDEX_ALL)
    rows, st = ctx.locate(ix, T, 0, Rd, R, 1, pi.LOC_MIN_LEN, kernel=PBA_KERNEL_BITVEC)
    prof = ctx.last_profile()
    assert prof["nb_first"] == NB and prof["n_redo"] == 0
    for c in LOC_COLS:
        assert (rows[c] == want[c]).all(), c
    assert st == wst, (st, wst)
    if NB == 1:                                                              # read by read: a slip in one lane has no other read to cancel in
        six = map_ref.SetIndex(oracle, [g], mask)
        for t in texts:
            w = map_ref.walk_one(oracle, six, [g], t, mask, R, 1)
            _, s1 = ctx.locate(ix, T, 0, ctx.seqs_from_list([t], strict_acgt=True), R, 1, pi.LOC_MIN_LEN, kernel=PBA_KERNEL_BITVEC)
            assert (s1["n_cells"], s1["n_pairs"], s1["n_located"]) == (w["n_cells"], w["n_pairs"], w["found"]), (len(t), s1, w)


@pytest.mark.parametrize("NB", [1, 2])
@pytest.mark.parametrize("R", [0.15, 0.30])
def test_prefilter_rows_locate_set_form(ctx, oracle, R, NB):
    """k_locate<NB, true>, through the set index pba_map_reads uses: the same genome cut into six contigs inside its spacers."""
    g, texts, meta, mask, _, _ = locate_expected(oracle, R, MASK_PAT, NB)
    starts = sorted(p for mt in meta if mt["kind"] == "planted" for p, _, _ in mt["places"])
    cuts = [0] + [starts[len(starts) * k // 6] - 10 for k in range(1, 6)] + [len(g)]
    contigs = [g[a:b] for a, b in zip(cuts, cuts[1:])]
    want, wst, _ = map_ref.map_reads_ref(oracle, contigs, texts, mask, R, 1, pi.LOC_MIN_LEN, strands=1)
    assert wst[0]["n_pairs"] == sum(len(mt["places"]) for mt in meta if mt["kind"] == "planted")     # no place was cut
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(texts, strict_acgt=True)
    got, gst = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, R, 1, pi.LOC_MIN_LEN, kernel=PBA_KERNEL_BITVEC, strands=1)
    prof = ctx.last_profile()
    assert prof["nb_first"] == NB and prof["n_redo"] == 0
    for c in ("found", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs"):
        assert (got[c] == want[c]).all(), c
    for c in map_ref.STAT_KEYS:
        assert gst["strand"][0][c] == wst[0][c], (c, gst["strand"][0], wst[0])


@pytest.mark.parametrize("R", [0.15, 0.30])
def test_prefilter_applies_from_32_elements_on_either_side(ctx, oracle, R):
    """The genome side clipped to 31 .. 65 elements (contigs that end behind the hit; the read side of those lengths is part
    of every locate case): below 32 the pair reaches the full aligner and is counted once, with the cells of its row.  And the
    size guard of prefilter32_applies: with (maxn, maxm) = (60, 20) a read of 96 bases is the caller's to refuse."""
    contigs, texts, frows = pi.locate_b_edges(R)
    mask = eng.mask_from_pattern(MASK_PAT)
    for k, (c, t) in enumerate(zip(contigs, texts)):
        p = len(c) - pi.LOC_EDGE_MS[k]
        assert [pi.key_hits(x, t[:16], MASK_PAT) for x in contigs] == [[p] if j == k else [] for j in range(len(contigs))]
        x = oracle.align(t, c[p:], R)
        assert x["rc"] == -1 and x["fail_row"] == frows[k] and x["len_b"] == pi.LOC_EDGE_MS[k], x
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(texts, strict_acgt=True)
    reads, offs = concat(texts)
    want, wst, _ = map_ref.map_reads_ref(oracle, contigs, texts, mask, R, 1, pi.LOC_MIN_LEN, strands=1)
    got, gst = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, R, 1, pi.LOC_MIN_LEN, kernel=PBA_KERNEL_BITVEC, strands=1)
    assert (got["n_pairs"] == 1).all() and (got["n_pairs"] == want["n_pairs"]).all() and not got["found"].any()
    for c in map_ref.STAT_KEYS:
        assert gst["strand"][0][c] == wst[0][c], (c, gst["strand"][0], wst[0])
    for k, c in enumerate(contigs):                                           # ... and one contig at a time, against the oracle's locator
        rows, st = ctx.locate(ctx.index_build(T, k, mask, PBA_INDEX_ALL), T, k, Rd, R, 1, pi.LOC_MIN_LEN, kernel=PBA_KERNEL_BITVEC)
        wrows, wst1 = oracle.locator(np.frombuffer(c, np.uint8), mask, R, reads, offs, 1, pi.LOC_MIN_LEN)
        assert st == wst1 and (rows["n_pairs"] == wrows["n_pairs"]).all() and wst1["n_pairs"] == 1, (k, st, wst1)
    g, ltexts, meta, _, _, _ = locate_expected(oracle, R, MASK_PAT, 1)
    lreads, loffs = concat(ltexts)
    Tg = ctx.seqs_from_list([g], strict_acgt=True)
    rows, st = ctx.locate(ctx.index_build(Tg, 0, mask, PBA_INDEX_ALL), Tg, 0, ctx.seqs_from_list(ltexts, strict_acgt=True), R, 1,
                          pi.LOC_MIN_LEN, maxn=60, maxm=20, kernel=PBA_KERNEL_BITVEC)
    wrows, wst2 = oracle.locator(np.frombuffer(g, np.uint8), mask, R, lreads, loffs, 1, pi.LOC_MIN_LEN, maxn=60, maxm=20, nthreads=8)
    for c in LOC_COLS:
        assert (rows[c] == wrows[c]).all(), c
    assert st == wst2 and wst2["n_located"] == 0, (st, wst2)


# ----------------------------------------------------------------------------- all-vs-all: the scan and the walk
# (R, mask, ring of the walk's first launch: 1 from the reads themselves, 2 behind a filler; at R = 0.9 the walk's target alone asks for 3)
OVL_CASES = [(R, MASK_PAT, 1 if R < 0.5 else 3) for R in pi.RS] + [(0.30, MASK_PAT, 2), (0.15, pi.HEAVY_PAT, 1), (0.30, pi.HEAVY_PAT, 1)]


def overlap_expected(oracle, R, pat, NB):
    key = ("ovl", R, pat, NB)
    if key in _CACHE:
        return _CACHE[key]
    texts, designed, nq, wt = pi.overlap_case(R, pat)
    if NB == 2:                                                               # an unrelated read that sizes the plan
        texts = texts + [ar.pilot(ar.row_of(2, 2)[0], R, seed=3)[0]]
    md = 1 + int(max(len(t) for t in texts) * R)
    assert ar.nb1(md) == NB and max(len(t) for t in texts) < 20000
    cands, n_match = pi.overlap_candidates(texts, pat)
    kinds = {d[:4]: d[4:] for d in designed}
    assert set(kinds) <= {c[:4] for c in cands}
    if R < 0.5 and NB == 1:                                                   # the designed places and the four mirrors, nothing else
        assert len(cands) == n_match == len(designed) + 4
    pre, listed, tight = [], [], []
    for t, q, fwd, p, a, b in cands:
        x = oracle.align(a, b, R)
        kind, f = kinds.get((t, q, fwd, p), ("", 0))
        if kind in ("fail", "blip", "short"):
            assert x["rc"] == -1 and x["fail_row"] == f, (kind, f, x)
        if kind in ("tight", "edge10"):
            assert (x["rc"] > 0) == (kind == "tight") and (x["rc"] > 0 or x["fail_row"] > 64)
            tight += [(t, q)] if kind == "tight" else []
        stopped = x["rc"] == -1 and 11 <= x["fail_row"] <= 32 and x["len_a"] >= 32 and x["len_b"] >= 32
        (pre if stopped else listed).append(dict(t=t, q=q, fwd=fwd, p=p, kind=kind, x=x, idx=p if fwd else p - 16, tlen=len(texts[t])))
    # what the scan's edges need, present among the candidates
    for fwd in (True, False):
        assert {0, 1, 31} <= {c["idx"] % 32 for c in pre if c["fwd"] == fwd} or R >= 0.5
        assert {31, 32, 33, 63, 64, 65} <= {c["x"]["len_a"] for c in pre + listed if c["fwd"] == fwd}
    if 0.15 <= R < 0.5:                                                       # the indel pairs pass their 32 rows off the diagonal's own count
        for fwd in (True, False):
            ind = [c["x"] for c in listed if c["kind"] == "indel" and c["fwd"] == fwd]
            assert len(ind) >= 3 and all(x["rc"] > 0 or x["fail_row"] > 32 for x in ind)
    if R < 0.5:
        assert any(c["fwd"] and c["p"] == c["tlen"] - 32 for c in pre) and any(not c["fwd"] and c["idx"] == 0 for c in pre)
        assert {31, 32, 33, 63, 64, 65} <= {c["x"]["len_b"] for c in pre + listed}
        short = [c["x"] for c in listed if c["x"]["rc"] == -1 and c["x"]["fail_row"] <= 32]                  # below the edge: the aligner's
        assert {min(x["len_a"], x["len_b"]) for x in short} == {31} and {31} < {x["len_a"] for x in short} | {x["len_b"] for x in short}
    assert {len(texts[nq + t]) % 32 for t in range(8)} == {0, 1}
    # the walk's target: 64 listed candidates, a tightrope in the first and in the last slot of the sorted list
    w = sorted((c for c in listed if c["t"] == wt), key=lambda c: (c["q"], not c["fwd"], c["p"]))
    assert len(w) >= 64 and w[0]["kind"] == "tight" and w[0]["x"]["rc"] > 0 and sum(c["kind"] == "tight" and c["x"]["rc"] > 0 for c in w) == 2
    assert R >= 0.5 or (len(w) == 64 and w[-1]["kind"] == "tight")            # (R = 0.9: chance hits among the places, wherever they sort)
    if R < 0.5:
        for fwd in (True, False):
            big = {f for f in pi.reachable(R, pat, fwd) if f > 32}              # every row of 33 .. 64 in reach: 31 of them on this target
            assert len({c["x"]["fail_row"] for c in w if c["fwd"] == fwd and c["x"]["rc"] == -1} & big) == min(31, len(big))
            assert big <= {c["x"]["fail_row"] for c in listed if c["fwd"] == fwd and c["x"]["rc"] == -1}
    file = b"".join(eng.text2bin(t) for t in texts)
    rec_offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in texts[:-1]]).astype(np.uint64)
    mask = eng.mask_from_pattern(pat)
    want, pairs = [], 0
    for t in range(len(texts)):
        rows = oracle.spaced_round(texts[t], mask, R, file, rec_offs, 1, pi.OVL_MIN, buggy=False, nthreads=8)
        pairs += int(rows["n_pairs"].sum()) - int(rows["n_pairs"][t])
        want += [(t, q, int(rows["j"][q]), int(rows["dir"][q]), int(rows["ref_pos"][q]), int(rows["cost"][q]), int(rows["matlen_a"][q]),
                  int(rows["matlen_b"][q])) for q in range(len(texts)) if q != t and rows["found"][q]]
    assert set(tight) <= {(r[0], r[1]) for r in want} and len(tight) == 4 and {r[3] for r in want} == {1, -1}
    _CACHE[key] = dict(texts=texts, mask=mask, want=want, pairs=pairs, n_match=n_match, n_pre=len(pre), n_listed=len(listed), nq=nq, wt=wt,
                       file=file, rec_offs=rec_offs)
    return _CACHE[key]


@pytest.mark.parametrize("R,pat,NB", OVL_CASES)
def test_prefilter_rows_scan_and_walk(ctx, oracle, prekeep, R, pat, NB):
    """k_ovl_scan<false> (MASK_PAT) and <true> (HEAVY_PAT: the hashed table), then ovl_walk<NB> on what it listed: the overlaps
    are the oracle's composition, and of the candidates -- enumerated on the CPU, each judged by the oracle -- exactly those
    with both clipped lengths >= 32 and a first failing row in 11 .. 32 are counted as prefiltered, the rest listed."""
    E = overlap_expected(oracle, R, pat, NB)
    assert (bin(E["mask"]).count("1") > 26) == (pat == pi.HEAVY_PAT)
    S = ctx.seqs_from_list(E["texts"], strict_acgt=True)
    got, st = ctx.overlap_all(S, E["mask"], R, 1, pi.OVL_MIN, kernel=PBA_KERNEL_BITVEC)
    assert [tuple(int(v) for v in r) for r in got] == E["want"]
    assert st["n_pairs"] == E["pairs"] and st["n_candidates"] == E["n_match"]
    assert (st["n_prefiltered"], st["n_listed"]) == (E["n_pre"], E["n_listed"]), st
    assert st["wide_first"] == 0 and st["cap_overflow"] == (prekeep == "equal_room_overflows")


def straddle_expected(oracle, R, NB):
    """both views of the case, what each is, and the oracle's answer -- once per session"""
    key = ("straddle", R, NB)
    if key in _CACHE:
        return _CACHE[key]
    views, nq = pi.straddle_views(R, NB)
    out = {}
    for name, (texts, qtexts) in views.items():
        assert ar.nb1(1 + int(max(len(t) for t in texts) * R)) == NB and max(len(t) for t in texts) < 20000
        W = pi.walk_composition(oracle, texts, qtexts, R)
        assert pi.straddle_situations(W["slices"]) == {nq: "a", nq + 1: "b", nq + 2: "c"}
        want, pairs = pi.oracle_composition(oracle, texts, qtexts, R)
        assert (W["rows"], W["pairs"]) == (want, pairs) and len(want) >= 10
        out[name] = dict(texts=texts, want=want, pairs=pairs, n_match=W["n_match"], n_pre=W["n_pre"], n_listed=W["n_listed"])
    _CACHE[key] = out
    return out


@pytest.mark.parametrize("NB", [1, 2])
@pytest.mark.parametrize("R", [0.30, 0.15])
def test_walk_group_edges(ctx, oracle, R, NB):
    """ovl_walk<NB> behind an item's first group, through k_ovl_walk (pba_overlap_all) and k_ovl_walk_rc (the reverse-complement
    pass of pba_overlap_strands over the set with its queries flipped).  Three targets of 87 .. 93 listed candidates
    (prefilter_inputs.straddle_case; test_prefilter_inputs_cpu.py says what they are, and so does straddle_expected): a run
    that crosses slots 63 | 64, fails eight times behind the edge at rows 33 .. 64 -- the array's to find: nothing is prefiltered
    there -- and then succeeds; a run that succeeds at slot 63 and would again at slot 64, which its own item must not reach and
    the next one must skip; a run that starts at slot 64.  Rows equal to the oracle's composition, the counters to the
    enumeration's, and the row-sweep walk agrees."""
    E = straddle_expected(oracle, R, NB)
    mask = eng.mask_from_pattern(MASK_PAT)
    rows_of = lambda got: [tuple(int(r[c]) for c in ("target", "query", "dir", "ref_pos", "cost", "matlen_a", "matlen_b")) for r in got]
    for name, e in E.items():
        S = ctx.seqs_from_list(e["texts"], strict_acgt=True)
        for kernel in (PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP):
            if name == "forward":
                got, st = ctx.overlap_all(S, mask, R, 1, pi.OVL_MIN, kernel=kernel)
            else:
                got, sts = ctx.overlap_strands(S, mask, R, 1, pi.OVL_MIN, strands=2, kernel=kernel)
                st = sts[1]
                assert (got["strand"] == -1).all()
            print(name, kernel, {k: st[k] for k in ("n_candidates", "n_pairs", "n_overlaps", "n_listed", "n_prefiltered", "n_redo")})
            assert not got["j"].any() and rows_of(got) == e["want"], (name, kernel)
            assert st["n_pairs"] == e["pairs"] and st["n_overlaps"] == len(e["want"]), (name, kernel, st)
            if kernel == PBA_KERNEL_BITVEC:
                assert (st["n_candidates"], st["n_listed"], st["n_prefiltered"]) == (e["n_match"], e["n_listed"], e["n_pre"]), (name, st)


@pytest.mark.parametrize("R", [0.15, 0.30])
def test_prefilter_rows_spaced_round(ctx, oracle, R):
    """k_spaced_round: the same reads against three of the targets as locked references, both directions: rows and pair counts."""
    E = overlap_expected(oracle, R, MASK_PAT, 1)
    Rd = ctx.seqs_from_list(E["texts"], strict_acgt=True)
    pairs, found, dirs = 0, 0, set()
    for t in (E["nq"], E["nq"] + 3, E["wt"]):
        Rf = ctx.seqs_from_list([E["texts"][t]], strict_acgt=True)
        ix = ctx.index_build(Rf, 0, E["mask"], PBA_INDEX_HEAD_TAIL)
        rows = ctx.spaced_round(ix, Rf, 0, Rd, R, 1, pi.OVL_MIN, buggy_seed_at=False, kernel=PBA_KERNEL_BITVEC)
        want = oracle.spaced_round(E["texts"][t], E["mask"], R, E["file"], E["rec_offs"], 1, pi.OVL_MIN, buggy=False, nthreads=8)
        other = np.arange(len(E["texts"])) != t
        sel = other & (want["found"] == 1)
        pairs, found, dirs = pairs + int(want["n_pairs"][other].sum()), found + int(sel.sum()), dirs | set(int(d) for d in want["dir"][sel])
        for c in ("found", "j", "n_trials", "n_pairs"):
            assert (rows[c][other] == want[c][other]).all(), (t, c)
        for c in ("dir", "ref_pos", "cost", "matlen_a", "matlen_b"):
            assert (rows[c][sel] == want[c][sel]).all(), (t, c)
    assert pairs >= 70 and found >= 3 and dirs == {1, -1}
