"""The reference-shaped row sweep (align_rowsweep.h) and the text entry points at the edges of the sweep's own geometry,
against the oracle -- exact: results, whole edit scripts, every cell of the DP matrix.  tests/rowsweep_inputs.py builds the
inputs, tests/test_rowsweep_inputs_cpu.py proves from the oracle alone that each is what it is named for.
Needs a real MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

import align_rings as ar
import rowsweep_inputs as ri
from pacbioassembly_amd.engine import PAIR_DTYPE, PBA_KERNEL_AUTO, PBA_KERNEL_ROWSWEEP, RESULT_DTYPE
from test_gpu_parity import check_result

pytestmark = pytest.mark.gpu

FORMS = ["acgt", "acgt_rowsweep", "bytes"]


@pytest.fixture(params=FORMS)
def form(request, monkeypatch):
    """The three ways a text pair is answered: ACGT through the bit-vector array (the m <= 10 corner inside it is the row
    sweep), ACGT through the row sweep (PBA_TEXT_ROWSWEEP=1), bytes outside ACGT (the row sweep, the only form they have)."""
    if request.param == "acgt_rowsweep":
        monkeypatch.setenv("PBA_TEXT_ROWSWEEP", "1")
    return request.param


def in_form(c, form):
    return c.translated() if form == "bytes" else c


def check_swept(got, exp, tag):
    """check_result, and the cell at the end of the diagonal as the row sweep reports it (also for a rejected pair)"""
    check_result(got, exp, tag)
    if min(exp["len_a"], exp["len_b"]) >= 1:
        assert int(got["diag_cost"]) == (-1 if exp["diag"] is None else exp["diag"]), (tag, int(got["diag_cost"]), exp["diag"])


# ----------------------------------------------------------------------------- packed batch
@pytest.mark.parametrize("R", [ri.R_EDGE, ri.R_EQ])
def test_packed_batch_rowsweep(ctx, oracle, R):
    """Every pair of one R in one align_batch and one align_batch_trace under PBA_KERNEL_ROWSWEEP: k_align_pairs<0>, then
    k_align_pairs_trace + k_trace_walk with one block per pair and the parent areas rounded to 16."""
    cs = [c for c in ri.all_cases() if c.R == R]
    assert len(cs) >= 20
    B = ri.batch_of(cs)
    exp = ri.expected(oracle, cs)
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs, PAIR_DTYPE)
    out = ctx.align_batch(S, S, pairs, R, kernel=PBA_KERNEL_ROWSWEEP)
    assert ctx.last_profile()["nb_first"] == 0
    for c, got, x in zip(cs, out, exp):
        check_swept(got, x, c.tag)
    out, ops = ctx.align_batch_trace(S, S, pairs, R, kernel=PBA_KERNEL_ROWSWEEP)
    assert ctx.last_profile()["nb_first"] == 0
    for c, got, o, x in zip(cs, out, ops, exp):
        check_swept(got, x, c.tag)
        assert o.tolist() == x["ops"].tolist(), c.tag


# ----------------------------------------------------------------------------- text entry points
@pytest.mark.parametrize("cls", ri.classes())
def test_text_entry_points(ctx, oracle, form, cls):
    """pba_align_text and pba_align_text_trace, one pair per call, forward and backward accessors as the case drew them."""
    cs = ri.of_class(cls)
    for c, x in zip(cs, ri.expected(oracle, cs)):
        t = in_form(c, form)
        got = ctx.align_text(t.mem_a(), t.mem_b(), t.R, not t.fa, not t.fb)
        got2, ops = ctx.align_text_trace(t.mem_a(), t.mem_b(), t.R, not t.fa, not t.fb)
        if form == "acgt":
            check_result(got, x, (c.tag, form))
            check_result(got2, x, (c.tag, form))
        else:
            check_swept(got, x, (c.tag, form))
            check_swept(got2, x, (c.tag, form))
        assert ops.tolist() == x["ops"].tolist(), (c.tag, form)


# ----------------------------------------------------------------------------- the DP matrix
SEAM_COLS = (0, 1, 62, 63, 64, 65, 126, 127, 128, 129)


def oracle_cells(oracle, x, rows, cols):
    """(cost, parent) arrays [len(rows), len(cols)] of the cells (i, c) as the most recent oracle.align left them: 0xFFFF / 0
    where it wrote none.  Row 0 is init_cell's for every j <= max_dst (seq_aligner.h:144-149), also past a len_b below max_dst,
    where oracle.cell answers for no cell."""
    md = x["max_dst"]
    cost = np.full((len(rows), len(cols)), 0xFFFF, np.uint16)
    par = np.zeros((len(rows), len(cols)), np.uint8)
    f, al, cv, pv = oracle.lib.orc_aligner_cell, oracle._aligner, C.c_int(), C.c_int()
    for a, i in enumerate(rows):
        for b, c in enumerate(cols):
            j = i + c - md
            if f(al, i, j, C.byref(cv), C.byref(pv)) == 0:
                cost[a, b], par[a, b] = cv.value, pv.value
            elif i == 0 and 0 <= j <= md:
                cost[a, b], par[a, b] = j, 2 if j else 0
    return cost, par


@pytest.mark.parametrize("cls", ri.classes())
def test_text_matrix(ctx, oracle, cls):
    """pba_align_text_matrix on the ACGT and the translated form: every cell (cost and parent) of the pairs with len_a <= 110;
    of the larger ones rows 0 .. 12, max_dst - 1 .. max_dst + 1 (where c_lo leaves 0), the last three rows swept and the one
    behind them, and in every row the columns either side of each 64-cell group seam and of the band's two edges.  Cells
    the oracle did not write hold 0xFFFF / 0.  A wrong parent order at a seam (MATCH before INSERT before DELETE, strict) or a
    wrong `left` in lane 0 shows here and nowhere else unless the path happens to cross it."""
    n_full = n_cells = 0
    cs = ri.of_class(cls)
    for c, x in zip(cs, ri.expected(oracle, cs)):
        oracle.align(c.a, c.b, c.R)                     # (the matrix read below is that of the most recent align)
        la, md = x["len_a"], x["max_dst"]
        W = 2 * md + 1
        swept = x["fail_row"] or la
        if la <= 110:
            rows, cols = list(range(la + 1)), list(range(W))
            n_full += 1
        else:
            rows = sorted({i for i in list(range(13)) + [md - 1, md, md + 1, swept - 2, swept - 1, swept, swept + 1] if 0 <= i <= la})
            cols = sorted({k for k in SEAM_COLS + (W - 2, W - 1) if k < W})
        want = [oracle_cells(oracle, x, rows, list(range(W)))]
        if la > 110:
            want.append(oracle_cells(oracle, x, list(range(la + 1)), cols))
        for form in ("acgt", "bytes"):
            t = in_form(c, form)
            got, cost, par, rows_swept = ctx.align_text_matrix(t.mem_a(), t.mem_b(), t.R, not t.fa, not t.fb)
            check_swept(got, x, (c.tag, form))
            assert rows_swept == swept and cost.shape == (la + 1, W) == par.shape, (c.tag, form, rows_swept, swept)
            views = [(cost[rows, :], par[rows, :])] + ([(cost[:, cols], par[:, cols])] if la > 110 else [])
            for (wc, wp), (gc, gp) in zip(want, views):
                bad = np.argwhere((wc != gc) | (wp != gp))
                assert bad.size == 0, (c.tag, form, "first differing (row index, column index) of the checked block", bad[0].tolist(),
                                       rows if gc.shape[0] == len(rows) else "all rows", cols if gc.shape[1] == len(cols) else "all columns")
                n_cells += wc.size
    assert n_cells > 0 and (n_full > 0 or cls.startswith("group:W1"))      # (m >= 207 there: no pair of those classes is read in full)


# ----------------------------------------------------------------------------- ops_cap
def raw_text_trace(ctx, t, cap, room):
    """pba_align_text_trace through the raw ABI with ops_cap = cap and a buffer of `room` bytes pre-filled with 0xEE"""
    a, b = t.mem_a(), t.mem_b()
    abuf, bbuf = np.frombuffer(a + b"\0", np.uint8), np.frombuffer(b + b"\0", np.uint8)
    pa = abuf.ctypes.data + (len(a) - 1 if t.fa and a else 0)
    pb = bbuf.ctypes.data + (len(b) - 1 if t.fb and b else 0)
    out = np.zeros(1, RESULT_DTYPE)
    ops = np.full(room, 0xEE, np.uint8)
    ne = C.c_int32(-7)
    ctx.check(ctx.lib.pba_align_text_trace(ctx.h, C.c_void_p(pa), int(not t.fa), len(a), C.c_void_p(pb), int(not t.fb), len(b), t.R, 0, 0,
                                           C.c_void_p(out.ctypes.data), C.c_void_p(ops.ctypes.data), cap, C.byref(ne)), "align_text_trace")
    return out[0], ops, ne.value


def cap_cases(oracle):
    """three accepted pairs with a script of some length: one inside the m <= 10 corner, one of the group set whose goal is off
    the diagonal's end, the (63, 64) tie with its 64 inserted bases"""
    cs = ri.all_cases()
    exp = ri.expected(oracle, cs)
    pick = [next(c for c, x in zip(cs, exp) if c.cls == "small" and x["rc"] >= 0 and 8 <= min(x["len_a"], x["len_b"]) <= 10
                 and len(set(x["ops"].tolist())) >= 2),
            next(c for c, x in zip(cs, exp) if c.cls == "group:W129" and x["rc"] >= 0 and x["matlen_b"] > x["len_a"]),
            next(c for c in cs if c.tag == "tie_row:63,64:tail40")]
    return pick, ri.expected(oracle, pick)


def test_ops_cap_prefix(ctx, oracle, form):
    """include/pba.h: *nedit is the full length whatever ops_cap is, ops receives the first min(nedit, ops_cap) ops in edits[]
    order, and nothing behind them is written -- in every form (the row sweep's walk meets the ops goal-first)."""
    pick, exp = cap_cases(oracle)
    for c, x in zip(pick, exp):
        want = x["ops"]
        n = int(want.size)
        assert n == x["nedit"] >= 9 and want[:n - 1].tolist() != want[1:].tolist(), c.tag      # the first n - 1 ops are not the last n - 1
        t = in_form(c, form)
        for cap in (0, 1, n - 1, n, n + 1):
            got, ops, ne = raw_text_trace(ctx, t, cap, n + 8)
            check_result(got, x, (c.tag, form, cap))
            k = min(n, cap)
            assert ne == n, (c.tag, form, cap, ne)
            assert ops[:k].tolist() == want[:k].tolist(), (c.tag, form, cap)
            assert (ops[k:] == 0xEE).all(), (c.tag, form, cap)


# ----------------------------------------------------------------------------- above the bit-vector limit
def test_auto_above_bitvec_limit(ctx, oracle):
    """PBA_KERNEL_AUTO with a pair whose band (max_dst 10 795) is the first the bit-vector array does not take: the batch goes
    to trace_rowsweep by its band width.  The pilot fails in its first rows; only its parent area is large (under 1 GB)."""
    R = ri.R_EDGE
    grp = [c for c in ri.all_cases() if c.cls.startswith("group")]
    cs = grp[::len(grp) // 16][:16]
    assert len(cs) == 16 and len({c.cls for c in cs}) == 6
    pil = ar.pilot(10795, R)
    assert not ar.bitvec_supports(10795) and ar.bitvec_supports(10794)
    assert (len(pil[0]) + 1) * (2 * 10795 + 1) < 1 << 30
    B = ri.batch_of(cs).with_pilot(pil)
    px = oracle.align(pil[0], pil[1], R, want_ops=True)
    assert px["max_dst"] == 10795 and px["rc"] == -1 and 11 <= px["fail_row"] <= 32
    exp = [px] + ri.expected(oracle, cs)
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    pairs = np.array(B.pairs, PAIR_DTYPE)
    out = ctx.align_batch(S, S, pairs, R, kernel=PBA_KERNEL_AUTO)
    assert ctx.last_profile()["nb_first"] == 0
    for q, (got, x) in enumerate(zip(out, exp)):
        check_result(got, x, B.meta[q]["tag"])
    out, ops = ctx.align_batch_trace(S, S, pairs, R, kernel=PBA_KERNEL_AUTO)
    assert ctx.last_profile()["nb_first"] == 0
    for q, (got, o, x) in enumerate(zip(out, ops, exp)):
        check_result(got, x, B.meta[q]["tag"])
        assert o.tolist() == x["ops"].tolist(), B.meta[q]["tag"]
