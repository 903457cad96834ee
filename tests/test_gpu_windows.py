"""Per-window alignment counts from the device and rows trimmed where they break: the WindowSink of the traced bit-vector
pass (k_window_pairs) at the edges of its 64-op groups and of the window grid, the trim kernel (k_trim_rows) at the edges of
its 64-window steps, the row-level entry points chunked and capped, the refusals, all of it again over scribbled kept
buffers, and the planted 6 % input end to end -- every comparison exact, against tests/windows_ref.py applied to the CPU
oracle's own scripts and to the runs pba_align_batch_cigar gives for the same batch.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

import align_rings as ar
import cigar_ref as cr
import windows_ref as wr
from clip_ref import PLANTED, ROW_FIELDS
from conftest import MASK_PAT
from map_ref import many_contig_case, rc
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import ALN_COUNTS_DTYPE, PAIR_DTYPE, RESULT_DTYPE, STRAND_OVERLAP_DTYPE, TRIM_ROW_DTYPE, PbaError
from test_align_rings_cpu import EDGE_R, excursion_case, must_redo
from test_cigar_cpu import overlap_case
from test_gpu_align_rings import EDGE_ROWS, forced
from test_gpu_parity import check_result

pytestmark = pytest.mark.gpu
FLAGS = (0, cr.REVERSED, cr.B_IS_QUERY, cr.REVERSED | cr.B_IS_QUERY)
SENTINEL = -7
R = cr.PLANT_R


# ----------------------------------------------------------------------------- the sink
def place_at(B, rng, text, back, res, W):
    """text inside a sequence of its own with the accessor's origin at a position that is `res` modulo W; (seq, pos, len)"""
    org = len(text) - 1 if back and text else 0
    left = (res - org) % W + (W if W <= 64 else 0) * int(rng.randint(0, 2))
    s = B.add_seq(ar.rand_seq(rng, left) + text + ar.rand_seq(rng, int(rng.randint(0, 40))))
    return s, left + org, len(text)


def batch_of(cases, W, seed=1):
    """cases: [(tag, a elements, b elements, backward, residue of a's origin modulo W)]"""
    B, rng = ar.Batch(), np.random.RandomState(seed)
    for tag, a, b, back, res in cases:
        ta, tb = (a[::-1], b[::-1]) if back else (a, b)          # the texts as they lie in memory
        B.add_pair(place_at(B, rng, ta, back, res % W, W), B.place(rng, tb, back, 1), back, back, tag=tag)
    return B


def raw_windows(ctx, S, pairs, W, flags, slack=2, off=None, R=R):
    """pba_align_batch_windows over slots of the bound + slack, prefilled: (status, results, windows, offsets, nwin, counts)"""
    n = pairs.size
    if off is None:
        bounds = [wr.bound(int(p["a_pos"]), int(p["a_len"]), int(p["b_len"]), R, W, bool(int(p["flags"]) & 1)) + slack for p in pairs]
        off = np.concatenate([[0], np.cumsum(bounds)]).astype(np.uint64)
    out, nwin, counts = np.zeros(n, RESULT_DTYPE), np.full(n, SENTINEL, np.int32), np.zeros(n, ALN_COUNTS_DTYPE)
    win = np.zeros(int(off[-1]) + 1, ALN_COUNTS_DTYPE)
    for f in wr.CNT:
        win[f] = SENTINEL
    st = ctx.lib.pba_align_batch_windows(ctx.h, S.h, S.h, pairs.ctypes.data, n, R, 0, 0, W, flags, out.ctypes.data, win.ctypes.data,
                                         off.ctypes.data, nwin.ctypes.data, counts.ctypes.data)
    return st, out, win, off, nwin, counts


def check_sink(ctx, oracle, cases, W, flags=0, seed=1):
    """every pair's windows equal windows_ref of the oracle's script and of the device's own runs; nothing else is written"""
    B = batch_of(cases, W, seed)
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs, PAIR_DTYPE)
    st, out, win, off, nwin, counts = raw_windows(ctx, S, pairs, W, flags)
    assert st == 0, ctx.lib.pba_ctx_error(ctx.h).decode()
    _, runs, rcounts = ctx.align_batch_cigar(S, S, pairs, R, flags=flags)
    n_win_seen = []
    for q, x in enumerate(ar.expected(oracle, B, R)):
        tag = (B.meta[q]["tag"], W, flags)
        check_result(out[q], x, tag)
        o0, o1 = int(off[q]), int(off[q + 1])
        a, b = B.elems(q)
        back, a_pos = bool(B.pairs[q][6] & 1), B.pairs[q][1]
        if x["rc"] < 0:                                          # n_win = 0, the slot untouched, counts zero
            assert nwin[q] == 0 and all((win[f][o0:o1] == SENTINEL).all() for f in wr.CNT) and tuple(counts[q]) == (0, 0, 0, 0), tag
            continue
        want = wr.from_script(x["ops"], a, b, a_pos, back, W, flags)
        got = [tuple(int(v) for v in w) for w in win[o0:o0 + int(nwin[q])]]
        assert got == [wr.tup(w) for w in want], (tag, got, want)
        assert all((win[f][o0 + len(want):o1] == SENTINEL).all() for f in wr.CNT), tag
        assert wr.from_runs(runs[q], a_pos, back, W, flags) == want, tag
        assert tuple(int(v) for v in counts[q]) == wr.tup(wr.total(want)) == tuple(int(v) for v in rcounts[q]), tag
        wr.check_invariants(want, x, W, flags)
        n_win_seen.append(len(want))
    return n_win_seen


def planted():
    return [(tag, a, b) for tag, a, b, _ in cr.planted_pairs()]


def test_boundary_at_the_kth_op(ctx, oracle):
    """a window boundary as the k-th op from the goal, k at the edges of the 64-op groups: the op that consumes a-element
    len - k opens a window, in exact copies and with the planted edit beside it"""
    W = 50
    cases = []
    for k in cr.GROUP_EDGES:
        for tag, a, b in planted():
            if tag.endswith(f"@{k}") or tag in ("copy150", "copy400", f"ops{k}"):
                if len(a) >= k:
                    cases.append((f"{tag}/k{k}", a, b, False, -(len(a) - k + 1)))
    assert len(cases) >= 7 * 4
    seen = check_sink(ctx, oracle, cases, W)
    assert max(seen) >= 8 and min(seen) == 1
    check_sink(ctx, oracle, cases, W, cr.REVERSED | cr.B_IS_QUERY)


@pytest.mark.parametrize("W", (1, 7, 64, 10000))
def test_planted_pairs_on_every_grid(ctx, oracle, W):
    """all of cigar_ref's planted pairs -- copies over several groups (a 400-base copy at W = 7 closes ten windows in one group
    and put_run straddles them), the row-sweep corners, the borders (the leading INSERT of border:b-leads goes to window 0),
    the failures -- at grid residues 0, 1 and W - 1: W = 1, W larger than the pair (one window, or two at residue W - 1)"""
    for res in sorted({0, 1 % W, W - 1}):
        seen = check_sink(ctx, oracle, [(tag, a, b, False, res) for tag, a, b in planted()], W, seed=res + 1)
        assert len(seen) == 40
        if W == 10000:
            assert set(seen) == ({1} if res < W - 1 else {1, 2})
        if W == 1:
            assert max(seen) == 400
        if W == 7:
            assert max(seen) in (58, 59)


def test_insert_run_at_a_window_and_group_edge(ctx, oracle):
    """five bases b has and a lacks, met as ops 63 .. 67 from the goal (across the group edge), with the a-element before
    them the last of its window: the INSERTs belong to that window, the MATCH after them to the next"""
    rng = np.random.default_rng(77)
    W, cases = 40, []
    for n_after in (60, 62, 63, 64):
        x = cr._seq(rng, 200)
        p = len(x) - n_after - 1                                 # the a-element before the INSERT run
        for _ in range(200):                                     # a 5-mer the reference's tie-break leaves in one piece
            y = x[:p + 1] + cr._seq(rng, 5) + x[p + 1:]
            ops = np.asarray(oracle.align(x, y, R, want_ops=True)["ops"])
            at = len(ops) - np.flatnonzero(ops == 2)             # the INSERTs, counted from the goal
            if (ops != 1).sum() == 5 and at.tolist() == list(range(n_after + 5, n_after, -1)):
                break
        else:
            raise AssertionError(("no 5-mer stays in one piece", n_after))
        cases.append((f"ins5@{n_after}", x, y, False, -(p + 1)))
        cases.append((f"ins5@{n_after}/mid", x, y, False, 3))
    for fl in (0, cr.REVERSED):
        check_sink(ctx, oracle, cases, W, fl)


@pytest.mark.parametrize("flags", FLAGS)
def test_backward_and_longer_a(ctx, oracle, flags):
    """the flags batch of cigar_ref: forward and both-backward accessors, len_a > len_b, a few edits each, at two grids"""
    cases = []
    for k, (a, fa, b, fb) in enumerate(cr.flags_batch()):
        cases.append((f"flags{k}", a[::-1] if fa else a, b[::-1] if fb else b, fa, k * 5))
    assert any(c[3] for c in cases) and any(len(c[1]) > len(c[2]) for c in cases)
    for W in (7, 64):
        seen = check_sink(ctx, oracle, cases, W, flags)
        assert len(seen) == 12 and min(seen) >= 2 - (W == 64)


def test_500_pairs_in_one_launch(ctx, oracle):
    rng = np.random.RandomState(4242)
    cases = []
    for k in range(500):
        m = int(rng.randint(11, 260)) if k % 10 else int(rng.randint(1, 11))
        x = ar.rand_seq(rng, m)
        y = ar.mutate(rng, x, (0.0, 0.05, 0.12, 0.2)[k % 4], head=min(30, m // 2)) + ar.rand_seq(rng, int(rng.randint(0, 40)))
        a, b = (y, x) if k % 3 == 0 else (x, y)
        cases.append((f"p{k}", a, b, k % 4 == 1, int(rng.randint(0, 32))))
    seen = check_sink(ctx, oracle, cases, 32, cr.B_IS_QUERY)
    assert len(seen) >= 400 and max(seen) >= 8


def test_batch_refusals(ctx):
    cases = [(f"flags{k}", a[::-1] if fa else a, b[::-1] if fb else b, fa, k) for k, (a, fa, b, fb) in enumerate(cr.flags_batch())]
    B = batch_of(cases, 16)
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs, PAIR_DTYPE)
    st, _, _, off, _, _ = raw_windows(ctx, S, pairs, 16, 0, slack=0)
    assert st == 0
    short = off.copy()
    short[5:] -= 1                                               # pair 4 is one slot short of the bound
    assert raw_windows(ctx, S, pairs, 16, 0, off=short)[0] == -1
    assert raw_windows(ctx, S, pairs, 0, 0, off=off)[0] == -1     # W < 1
    assert raw_windows(ctx, S, pairs, 16, 4, off=off)[0] == -1    # an unknown flag
    N = ctx.seqs_from_list([s[:-1] + b"N" if len(s) > 3 else s for s in B.seqs])
    n = pairs.size
    out, nwin, counts = np.zeros(n, RESULT_DTYPE), np.zeros(n, np.int32), np.zeros(n, ALN_COUNTS_DTYPE)
    win = np.zeros(int(off[-1]) + 1, ALN_COUNTS_DTYPE)
    assert ctx.lib.pba_align_batch_windows(ctx.h, N.h, S.h, pairs.ctypes.data, n, R, 0, 0, 16, 0, out.ctypes.data, win.ctypes.data,
                                           off.ctypes.data, nwin.ctypes.data, counts.ctypes.data) == -6
    assert ctx.lib.pba_align_batch_windows(ctx.h, S.h, S.h, None, 0, R, 0, 0, 16, 0, None, None, None, None, None) == 0      # no pairs


# ----------------------------------------------------------------------------- every ring, and the re-run
RING_W = 37                                                      # does not divide 64: the window boundaries fall on varying lanes


def check_rings(ctx, oracle, B, R):
    """k_window_pairs over the batches test_gpu_cigar.py runs through k_cigar_pairs: every successful pair's windows equal
    windows_ref of the oracle's script under W = 37, origin-first with default names and goal-first with b as the query; the
    rest of every slot keeps its sentinel, a failing pair's whole slot does, counts is the windows' total.  The profile of
    each of the two calls."""
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs, PAIR_DTYPE)
    exp = ar.expected(oracle, B, R)                              # once, for both calls
    profs = []
    for flags in (0, cr.REVERSED | cr.B_IS_QUERY):
        st, out, win, off, nwin, counts = raw_windows(ctx, S, pairs, RING_W, flags, R=R)
        assert st == 0, ctx.lib.pba_ctx_error(ctx.h).decode()
        profs.append(ctx.last_profile())
        for q, x in enumerate(exp):
            tag = (B.meta[q]["tag"], flags)
            check_result(out[q], x, tag)
            o0, o1 = int(off[q]), int(off[q + 1])
            if x["rc"] < 0:
                assert nwin[q] == 0 and all((win[f][o0:o1] == SENTINEL).all() for f in wr.CNT) and tuple(counts[q]) == (0, 0, 0, 0), tag
                continue
            a, b = B.elems(q)
            want = wr.from_script(x["ops"], a, b, B.pairs[q][1], bool(B.pairs[q][6] & 1), RING_W, flags)
            assert int(nwin[q]) == len(want), (tag, int(nwin[q]), len(want))
            got = [tuple(int(v) for v in w) for w in win[o0:o0 + len(want)]]
            assert got == [wr.tup(w) for w in want], (tag, got, want)
            assert all((win[f][o0 + len(want):o1] == SENTINEL).all() for f in wr.CNT), tag
            assert tuple(int(v) for v in counts[q]) == wr.tup(wr.total(want)), tag
    return profs


@pytest.mark.parametrize("row", EDGE_ROWS)
def test_every_ring(ctx, oracle, row):
    """k_window_pairs<nb1> on the edge set built for that ring, behind its pilot"""
    for prof in check_rings(ctx, oracle, forced(row, ar.edge_pairs(row[0], EDGE_R)), EDGE_R):
        assert prof["nb_first"] == row[0]


def test_rerun_excursions(ctx, oracle):
    B, w, wl = excursion_case()
    need = len(must_redo(ar.expected(oracle, B, ar.EXC_R), B.meta, w, wl))
    for prof in check_rings(ctx, oracle, B, ar.EXC_R):
        assert prof["nb_first"] == 1 and prof["nb_redo"] == 2 and prof["n_redo"] >= need


@pytest.mark.parametrize("row", sorted(ar.WIDE))
def test_rerun_reference_band(ctx, oracle, row):
    B, R = ar.wide_pairs(row)
    for prof in check_rings(ctx, oracle, B.subset([0]), R):
        assert prof["nb_redo"] == row[1] and prof["n_redo"] == 1


# ----------------------------------------------------------------------------- the trim kernel
TW, TERR = 10, 0.25                                              # thr[10] = 2
G, BAD, EDGE, OVER = (9, 1, 0, 0), (7, 3, 0, 0), (8, 2, 0, 0), (7, 2, 0, 1)


def as_windows(tuples):
    out = np.zeros(len(tuples), ALN_COUNTS_DTYPE)
    for k, t in enumerate(tuples):
        out[k] = t
    return out


def check_trim(ctx, items, W, max_err, min_span):
    got = ctx.windows_trim([as_windows(it) for it in items], W, max_err, min_span)
    for q, it in enumerate(items):
        want = wr.trim([dict(zip(wr.CNT, t)) for t in it], W, max_err, min_span)
        assert {f: int(got[q][f]) for f in wr.SPAN_FIELDS} == want, (q, len(it), want)
    return got


def hand_items():
    items = []
    for n in (0, 1, 63, 64, 65, 128, 129, 200):
        items.append([G] * n)                                    # one run over all of it: up to four steps
        for bad_at in (0, 62, 63, 64, 65, n - 1):                # lane 0, lane 63, both sides of a step edge, the last window
            if 0 <= bad_at < n:
                it = [G] * n
                it[bad_at] = BAD
                items.append(it)
        if n >= 2:
            items.append([BAD] * n)                              # all windows bad
    items.append([BAD] + [G] * 198 + [BAD])                      # a run over three steps and a bit, closed at both ends
    items.append([G] * 70 + [BAD] + [G] * 70)                    # equal runs: the first wins
    items.append([G] * 60 + [BAD] + [G] * 70 + [BAD] + [G] * 65)  # a longer run after a shorter one, then a shorter again
    items.append([G] * 64 + [BAD] + [G] * 64)                    # equal runs that end and begin at step edges
    items.append([EDGE] * 5 + [OVER] + [EDGE] * 4)               # err == thr is good, thr + 1 is not
    items.append([(5, 0, 4, 0)] * 3)                             # na 9, thr 2, err 4: bad
    items.append([(0, 0, 0, 3), G, G])                           # a window without an a-element: thr[0] = 0 < 3
    return items


def test_trim_kernel_edges(ctx):
    items = hand_items()
    got = check_trim(ctx, items, TW, TERR, 0)
    assert {int(s) for s in got["state"]} == {wr.DROPPED, wr.WHOLE, wr.CUT} and int(got["n_runs"].max()) == 3
    for min_span in (700, 701):                                  # [G] * 70 + ...: 700 a-elements met, missed by one
        s = check_trim(ctx, [[G] * 70 + [BAD] + [G] * 70], TW, TERR, min_span)[0]
        assert int(s["state"]) == (wr.CUT if min_span == 700 else wr.DROPPED) and int(s["n_runs"]) == 2
    s = check_trim(ctx, [[(0, 0, 4, 0)] * 3 + [(0, 0, 0, 3)] + [G]], TW, 1.0, 0)[0]   # the winner (12 a-elements) has no b-element
    assert int(s["state"]) == wr.DROPPED
    assert len(ctx.windows_trim([], TW, TERR, 0)) == 0
    for W, e, m in ((0, 0.25, 0), (10, -0.1, 0), (10, 1.5, 0), (10, float("nan"), 0), (10, 0.25, -1)):
        with pytest.raises(PbaError) as ex:
            ctx.windows_trim([as_windows([G])], W, e, m)
        assert ex.value.status == -1
    with pytest.raises(PbaError):
        ctx.windows_trim([as_windows([(9, 1, 1, 0)])], 10, 0.25, 0)              # a window of 11 a-elements on a grid of 10


def test_trim_kernel_fuzz(ctx):
    """20 000 items of 0 .. 200 windows, good with probability 0.5 .. 0.97, ragged a-element counts"""
    rng = np.random.default_rng(515)
    items = []
    for k in range(20000):
        n = int(rng.integers(0, 201)) if k % 8 == 0 else int(rng.integers(0, 24))
        na = rng.integers(1, TW + 1, n)
        err = np.where(rng.random(n) < rng.uniform(0.5, 0.97), 0, 1) * rng.integers(1, 6, n) + (rng.random(n) < 0.3)
        err = np.minimum(err, na)
        x = rng.integers(0, err + 1)
        items.append([(int(na[i] - err[i]), int(x[i]), int(err[i] - x[i]), int(rng.integers(0, 3))) for i in range(n)])
    got = check_trim(ctx, items, TW, TERR, 12)
    assert {int(s) for s in got["state"]} == {wr.DROPPED, wr.WHOLE, wr.CUT} and int(got["n_runs"].max()) >= 5


# ----------------------------------------------------------------------------- rows
@pytest.fixture(scope="module")
def overlaps(ctx, oracle):
    """the engine's own rows of a small mixed-strand set, and the reference's windows of every row from the oracle's script"""
    texts = overlap_case()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, eng.mask_from_pattern(MASK_PAT), 0.30, 32, 64, strands=3, reads_rc=Src)
    assert {(int(r["strand"]), int(r["dir"])) for r in rows} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}
    return dict(texts=texts, S=S, Src=Src, rows=rows)


def want_row_windows(oracle, o, W, default_names=False):
    return [wr.row_windows(oracle, r, o["texts"], 0.30, W, wr.overlap_row_flags(r) & ~(cr.B_IS_QUERY if default_names else 0))[0]
            for r in o["rows"]]


def check_overlap_windows(ctx, oracle, o, W=32):
    want = want_row_windows(oracle, o, W)
    woff, wtotal, wdense = cr.layout(want)
    bounds = []
    for r in o["rows"]:
        p = eng.overlap_row_pair(r, len(o["texts"][int(r["target"])]), len(o["texts"][int(r["query"])]))
        bounds.append(wr.bound(int(p["a_pos"]), int(p["a_len"]), int(p["b_len"]), 0.30, W, int(r["dir"]) == -1))
    for ms in (0, sum(bounds) // 3, 1):                          # the default, three chunks or more, one row per chunk
        wins, counts, off, res, total = ctx.overlap_windows(o["S"], o["rows"], 0.30, W, reads_rc=o["Src"], max_slots=ms)
        assert off.tolist() == woff and total == wtotal, ms
        for k, r in enumerate(o["rows"]):
            assert [tuple(int(v) for v in w) for w in wins[k]] == [wr.tup(w) for w in want[k]], (k, ms)
            assert tuple(int(v) for v in counts[k]) == wr.tup(wr.total(want[k])), k
            assert (res[k]["cost"], res[k]["matlen_a"], res[k]["matlen_b"]) == (r["cost"], r["matlen_a"], r["matlen_b"])
            assert len(want[k]) <= bounds[k]
    cap = woff[len(woff) // 2] + 1                               # below the total: whole rows only, offsets and total complete
    wins, _, off, _, total = ctx.overlap_windows(o["S"], o["rows"], 0.30, W, reads_rc=o["Src"], cap=cap)
    assert off.tolist() == woff and total == wtotal
    kept = [k for k in range(len(want)) if woff[k + 1] <= cap]
    assert 0 < len(kept) < len(want) and all(wins[k] is None for k in range(len(kept), len(want)))
    assert all([tuple(int(v) for v in w) for w in wins[k]] == [wr.tup(w) for w in want[k]] for k in kept)
    return want


def check_overlap_trim(ctx, oracle, o, W, max_err, min_span):
    want = [wr.row_trim(r, len(o["texts"][int(r["query"])]), wins, W, max_err, min_span)
            for r, wins in zip(o["rows"], want_row_windows(oracle, o, W, default_names=True))]
    for ms in (0, 1):
        got, st = ctx.overlap_trim(o["S"], o["rows"], 0.30, W, max_err, min_span, reads_rc=o["Src"], max_slots=ms)
        for k in range(len(want)):
            assert {f: int(got[k][f]) for f in wr.ROW_FIELDS} == want[k], (k, ms, W)
        n_state = [sum(t["state"] == s for t in want) for s in (wr.DROPPED, wr.WHOLE, wr.CUT)]
        assert [st["n_dropped"], st["n_whole"], st["n_cut"]] == n_state and st["n_rows"] == len(want)
        assert st["n_windows"] == sum(t["n_win"] for t in want) and st["n_chunks"] == (1 if ms == 0 else len(want))
    assert eng.trim_rows_apply(o["rows"], got).tolist() == wr.apply_trims(o["rows"], want).tolist()
    return want


def test_overlap_rows_windows(ctx, oracle, overlaps):
    want = check_overlap_windows(ctx, oracle, overlaps)
    assert max(len(w) for w in want) >= 20
    # the target's forward order on the target's own grid: the rows of one target agree on where a window lies
    for k, r in enumerate(overlaps["rows"]):
        first = (int(r["t_beg"]) // 32 + 1) * 32 - int(r["t_beg"])              # target bases of the first window
        assert wr.consumed_a(want[k][0], cr.B_IS_QUERY) == min(first, int(r["matlen_a"])), k


def test_overlap_rows_trim(ctx, oracle, overlaps):
    seen = set()
    for W, max_err, min_span in ((100, 0.25, 64), (32, 0.15, 64), (32, 0.15, 300), (64, 0.0, 0), (1000, 1.0, 0)):
        want = check_overlap_trim(ctx, oracle, overlaps, W, max_err, min_span)
        seen |= {(t["state"], int(r["dir"]), int(r["strand"])) for t, r in zip(want, overlaps["rows"])}
    assert {s for s, _, _ in seen} == {wr.DROPPED, wr.WHOLE, wr.CUT}
    assert {(d, s) for st, d, s in seen if st == wr.CUT} == {(1, 1), (1, -1), (-1, 1), (-1, -1)}


def test_rows_refusals(ctx, overlaps):
    o = overlaps
    for W, e, m in ((0, 0.25, 0), (10, -0.5, 0), (10, 1.01, 0), (10, 0.25, -1)):
        with pytest.raises(PbaError) as ex:
            ctx.overlap_trim(o["S"], o["rows"], 0.30, W, e, m, reads_rc=o["Src"])
        assert ex.value.status == -1
    with pytest.raises(PbaError) as ex:
        ctx.overlap_windows(o["S"], o["rows"], 0.30, 0, reads_rc=o["Src"])
    assert ex.value.status == -1
    bad = o["rows"].copy()
    bad["matlen_b"][1] -= 1                                      # not a row of these sets: the re-run disagrees
    for call in (lambda: ctx.overlap_windows(o["S"], bad, 0.30, 32, reads_rc=o["Src"]),
                 lambda: ctx.overlap_trim(o["S"], bad, 0.30, 32, reads_rc=o["Src"]),
                 lambda: ctx.overlap_windows(o["S"], o["rows"], 0.30, 32),                   # a strand -1 row without reads_rc
                 lambda: ctx.overlap_trim(o["S"], o["rows"], 0.30, 32)):
        with pytest.raises(PbaError) as ex:
            call()
        assert ex.value.status == -1
    bad = o["rows"].copy()
    bad["target"][0] = len(o["texts"])
    with pytest.raises(PbaError):
        ctx.overlap_trim(o["S"], bad, 0.30, 32, reads_rc=o["Src"])
    none = np.zeros(0, STRAND_OVERLAP_DTYPE)                     # zero rows are legal
    wins, _, off, _, total = ctx.overlap_windows(o["S"], none, 0.30, 32, reads_rc=o["Src"])
    assert wins == [] and off.tolist() == [0] and total == 0
    got, st = ctx.overlap_trim(o["S"], none, 0.30, 32, reads_rc=o["Src"])
    assert len(got) == 0 and st["n_rows"] == 0 and TRIM_ROW_DTYPE.itemsize == 44


MAP_R = 0.30


def test_mapped_rows_windows(ctx, oracle):
    """a small mapped set: the grid lies on the read (rc(read) for strand -1), windows origin-first, default names"""
    contigs, reads, _ = many_contig_case(961, n_reads=40)
    mask = eng.mask_from_pattern(MASK_PAT)
    T, Rd = ctx.seqs_from_list(contigs, strict_acgt=True), ctx.seqs_from_list(reads, strict_acgt=True)
    Rc = ctx.seqs_revcomp(Rd)
    rows, _ = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, MAP_R, 50, 500, strands=3, reads_rc=Rc)
    want = []
    for r in rows:
        if not r["found"]:
            want.append([])
            continue
        _, ap, al, _, bp, bl, _ = cr.map_row_aln_pair(r, len(contigs[int(r["contig"])]), len(reads[int(r["read"])]), MAP_R)
        text = reads[int(r["read"])] if r["strand"] == 1 else rc(reads[int(r["read"])])
        a, b = text[ap:ap + al], contigs[int(r["contig"])][bp:bp + bl]
        x = oracle.align(a, b, MAP_R, want_ops=True)
        assert (x["rc"] >= 0, x["cost"], x["matlen_a"], x["matlen_b"]) == (True, r["cost"], r["matlen_a"], r["matlen_b"])
        want.append(wr.from_script(x["ops"], a, b, ap, False, 64, 0))
    assert sum(1 for r in rows if r["found"]) >= 10 and {int(s) for s in rows["strand"]} >= {1, -1}
    woff, wtotal, _ = cr.layout(want)
    for ms in (0, 1):
        wins, counts, off, res, total = ctx.map_windows(T, Rd, rows, MAP_R, 64, reads_rc=Rc, max_slots=ms)
        assert off.tolist() == woff and total == wtotal
        for k in range(len(rows)):
            assert [tuple(int(v) for v in w) for w in wins[k]] == [wr.tup(w) for w in want[k]], k
            assert tuple(int(v) for v in counts[k]) == wr.tup(wr.total(want[k])), k
    with pytest.raises(PbaError) as ex:
        ctx.map_windows(T, Rd, rows, MAP_R, 0, reads_rc=Rc)
    assert ex.value.status == -1


@pytest.mark.parametrize("byte", (0x00, 0xFF, 0x5A))
def test_over_scribbled_kept_buffers(ctx, oracle, overlaps, byte):
    """the new entry points keep no buffer of their own between calls; what they share -- the traced pass's scratch, the
    work-queue counters -- is scribbled after a larger call of the same entry points, and every answer holds"""
    ctx.trim()
    rng = np.random.RandomState(9)
    big = [(f"decoy{k}", x, x, False, 0) for k, x in enumerate(ar.rand_seq(rng, 3000) for _ in range(64))]
    B = batch_of(big, 100)
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    assert raw_windows(ctx, S, np.array(B.pairs, PAIR_DTYPE), 100, 0)[0] == 0
    assert ctx.kept_bytes()["scratch"] > 0
    ctx.scribble(byte)
    before = ctx.kept_bytes()
    check_sink(ctx, oracle, [(tag, a, b, False, 3) for tag, a, b in planted()], 7)
    check_overlap_windows(ctx, oracle, overlaps)
    ctx.scribble(byte)
    check_overlap_trim(ctx, oracle, overlaps, 32, 0.15, 64)
    check_trim(ctx, hand_items(), TW, TERR, 0)
    assert ctx.kept_bytes()["scratch"] == before["scratch"]       # the cases ran inside the scribbled scratch
    ctx.trim()


# ----------------------------------------------------------------------------- end to end
def test_end_to_end_planted(ctx, oracle):
    """The planted 6 % input of tests/test_windows_cpu.py::test_planted_six_percent through Context.clip_reads and
    Context.clip_reads_trimmed.  Conditions (windows_ref.planted_conditions): under plain clip at least 6 of the 11 chimeras
    stay WHOLE (observed: 10); under the trimmed rows none is WHOLE, at most 2 keep both J - margin and J + margin (observed:
    0), and at least as many clean reads stay whole as under plain clip, minus 4 (observed difference: 0).  Every 40th row's
    trim record is also held to the reference over the oracle's script; everything else is printed."""
    P, T = PLANTED, wr.TRIM
    texts, chim = wr.planted_reads_6()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    mask = eng.mask_from_pattern(MASK_PAT)
    _, plain, rows0, _ = ctx.clip_reads(S, mask, P["R"], margin=P["margin"], min_cov=P["min_cov"], targets_per_call=50)
    clipped, table, rows, stats, trims, tstats = ctx.clip_reads_trimmed(S, mask, P["R"], T["W"], T["max_err"], T["min_span"],
                                                                        margin=P["margin"], min_cov=P["min_cov"], targets_per_call=50)
    assert np.array_equal(rows, rows0) and len(trims) == len(rows) and clipped.count == len(texts)
    print(len(rows), "rows;", tstats, stats)
    for k in range(0, len(rows), 40):
        wins, _ = wr.row_windows(oracle, rows[k], texts, P["R"], T["W"], cr.REVERSED if int(rows[k]["dir"]) == -1 else 0)
        want = wr.row_trim(rows[k], len(texts[int(rows[k]["query"])]), wins, T["W"], T["max_err"], T["min_span"])
        assert {f: int(trims[k][f]) for f in wr.ROW_FIELDS} == want, k
    as_table = lambda t: [tuple(int(r[f]) for f in ROW_FIELDS) for r in t]
    wr.planted_conditions(as_table(plain), as_table(table), chim, P["margin"])
    assert tstats["n_cut"] + tstats["n_whole"] + tstats["n_dropped"] == len(rows) and tstats["n_cut"] >= 1
