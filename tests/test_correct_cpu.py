"""Read correction, the part that needs no GPU: pba_overlap_row_pair (host arithmetic of libpba.so) turns an overlap row
into the pair of accessors a locked spaced_seed round aligned to find it.  Checked against the CPU oracle: aligning exactly
those accessors gives the row's cost and match lengths back."""
import collections
import ctypes as C

import numpy as np

from conftest import MASK_PAT
from correct_helpers import intervals, mixed_reads, oracle_rows, pair_texts
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PAIR_DTYPE, STRAND_OVERLAP_DTYPE, PbaError

import pytest


def test_row_pair_realigns_to_the_row(lib, oracle):
    """60 reads of 1.5-2.5 kb, 15 % error, 12x, about half of them reverse-complemented: for every row the oracle finds on
    either strand, the pair reproduces cost / matlen_a / matlen_b, and the row's forward-strand intervals are the ones the
    pair's accessors and the match lengths span."""
    texts, _, flip = mixed_reads(301, 302, 60, 2500, 10000, rl_min=1500)
    assert 15 <= int(flip.sum()) <= 45
    mask = eng.mask_from_pattern(MASK_PAT)
    rows = oracle_rows(oracle, texts, mask)
    combos = collections.Counter((int(r["strand"]), int(r["dir"])) for r in rows)
    assert len(rows) >= 100, len(rows)
    for s in (1, -1):
        for d in (1, -1):
            assert combos[(s, d)] >= 5, combos
    for r in rows:
        tl, ql = len(texts[int(r["target"])]), len(texts[int(r["query"])])
        pr = eng.overlap_row_pair(r, tl, ql)
        assert int(pr["a_seq"]) == int(r["target"]) and int(pr["b_seq"]) == int(r["query"])
        fwd = int(r["dir"]) == 1
        assert int(pr["flags"]) == (0 if fwd else 3)
        a, b, f = pair_texts(pr, texts, int(r["strand"]))
        assert f == fwd and len(a) == int(pr["a_len"]) and len(b) == int(pr["b_len"])
        res = oracle.align(a, b, 0.30, a_fwd=fwd, b_fwd=fwd)
        assert res["rc"] >= 0, (r, res)
        assert (res["cost"], res["matlen_a"], res["matlen_b"]) == (int(r["cost"]), int(r["matlen_a"]), int(r["matlen_b"])), (r, res)
        # the intervals the accessors and match lengths span, on the text that was walked ...
        ap, bp, ma, mb = int(pr["a_pos"]), int(pr["b_pos"]), int(r["matlen_a"]), int(r["matlen_b"])
        t_iv = (ap, ap + ma) if fwd else (ap - ma + 1, ap + 1)
        b_iv = (bp, bp + mb) if fwd else (bp - mb + 1, bp + 1)
        # ... the query's mapped back to its forward strand for a strand -1 row
        q_iv = b_iv if int(r["strand"]) > 0 else (ql - b_iv[1], ql - b_iv[0])
        assert (int(r["t_beg"]), int(r["t_end"])) == t_iv and (int(r["q_beg"]), int(r["q_end"])) == q_iv, r
        assert (int(r["t_beg"]), int(r["t_end"]), int(r["q_beg"]), int(r["q_end"])) == intervals(r, ql)
        assert 0 <= t_iv[0] < t_iv[1] <= tl and 0 <= q_iv[0] < q_iv[1] <= ql


def row(**kw):
    r = np.zeros(1, STRAND_OVERLAP_DTYPE)[0]
    r["strand"], r["dir"] = 1, 1
    for k, v in kw.items():
        r[k] = v
    return r


def test_row_pair_argument_checks(lib):
    ok = eng.overlap_row_pair(row(target=3, query=5, j=10, ref_pos=100), 1000, 500)
    assert tuple(int(ok[k]) for k in PAIR_DTYPE.names) == (3, 100, 900, 5, 10, 490, 0)
    bw = eng.overlap_row_pair(row(target=3, query=5, j=10, ref_pos=100, dir=-1, strand=-1), 1000, 500)
    assert tuple(int(bw[k]) for k in PAIR_DTYPE.names) == (3, 115, 116, 5, 489, 490, 3)
    # the last legal positions
    eng.overlap_row_pair(row(j=499, ref_pos=999), 1000, 500)
    eng.overlap_row_pair(row(j=499, ref_pos=984, dir=-1), 1000, 500)

    def status(r, tl=1000, ql=500):
        with pytest.raises(PbaError) as e:
            eng.overlap_row_pair(r, tl, ql)
        return e.value.status

    assert status(row(j=0, ref_pos=1000)) == -1                   # forward accessor starts past the target
    assert status(row(j=0, ref_pos=985, dir=-1)) == -1            # backward accessor starts at ref_pos + 15 >= len
    assert status(row(j=500, ref_pos=0)) == -1                    # nothing left of the query
    assert status(row(j=0, ref_pos=0), tl=0) == -1
    assert status(row(j=-1, ref_pos=0)) == -1 and status(row(j=0, ref_pos=-1)) == -1
    assert status(row(j=0, ref_pos=0, dir=0)) == -1 and status(row(j=0, ref_pos=0, strand=0)) == -1
    assert status(row(j=0, ref_pos=0, target=-1)) == -1 and status(row(j=0, ref_pos=0, query=-1)) == -1
    r = np.zeros(1, STRAND_OVERLAP_DTYPE)
    r[0] = row(j=0, ref_pos=0)
    out = np.zeros(1, PAIR_DTYPE)
    assert lib.pba_overlap_row_pair(None, 10, 10, C.c_void_p(out.ctypes.data)) == -1
    assert lib.pba_overlap_row_pair(C.c_void_p(r.ctypes.data), 10, 10, None) == -1
    assert lib.pba_overlap_row_pair(C.c_void_p(r.ctypes.data), 10, 10, C.c_void_p(out.ctypes.data)) == 0
