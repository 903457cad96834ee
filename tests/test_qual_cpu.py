"""The evidence rule without a GPU: pba_qual_phred (host arithmetic of include/pba.h) against tests/qual_ref.py on the rule's
own edges, and qual_ref's evidence / summary / low_spans / fastq_image -- the expectation tests/test_gpu_qual.py holds the
device to -- on hand-built cases whose answers are written out here.  All comparisons are exact."""
import numpy as np
import pytest

import qual_ref as qr
from pacbioassembly_amd import engine as eng

WORKED = [((1, 1), 4), ((20, 20), 13), ((15, 20), 5), ((8, 8), 10), ((7, 7), 9), ((65535, 65535), 48)]


def test_worked_values(lib):
    for (a, n), want in WORKED:
        assert qr.phred(a, n) == want and lib.pba_qual_phred(a, n, 60) == want and eng.qual_phred(a, n) == want, (a, n)
    assert qr.phred(9, 5) == qr.phred(5, 5) and lib.pba_qual_phred(9, 5, 60) == lib.pba_qual_phred(5, 5, 60)
    assert qr.S[10] == 10000 and (0 + 1) * qr.S[10] == (8 + 2) * 1000          # phred(8, 8) sits on an equality
    assert [qr.S[q] for q in (0, 9, 10, 59, 60)] == [1000, 7943, 10000, 794300000, 1000000000]
    assert qr.D == tuple(int(np.floor(1000 * 10 ** (r / 10) + 1e-9)) for r in range(10))


def test_every_threshold_and_its_neighbours(lib):
    """For each q in 0..60: the first N that reaches it (with 0, 1, 3 and 20 dissenting observations), one below, one above."""
    for q in range(61):
        for against in (0, 1, 3, 20):
            n0 = qr.threshold_n(q, against)
            assert qr.phred(n0 - against, n0) >= q
            if n0 > against:
                assert qr.phred(n0 - 1 - against, n0 - 1) < q, (q, against)
            for n in (n0 - 1, n0, n0 + 1):
                if n >= against:
                    assert lib.pba_qual_phred(n - against, n, 60) == qr.phred(n - against, n), (q, against, n)


@pytest.mark.parametrize("qmax", [0, 1, 10, 60])
def test_grid_at_every_cap(lib, qmax):
    agree, n = qr.phred_grid()
    want = qr.phred_array(agree, n, qmax)
    got = np.array([lib.pba_qual_phred(int(a), int(x), qmax) for a, x in zip(agree, n)])
    assert (got == want).all(), np.flatnonzero(got != want)[:8]
    assert want.max() <= qmax
    for a, x in list(zip(agree, n))[:40]:                                        # the array form and the integer form agree
        assert qr.phred(int(a), int(x), qmax) == int(qr.phred_array([a], [x], qmax)[0])


def test_limits(lib):
    big = 2 ** 31 + 65534
    assert (big + 2) * 1000 < 2 ** 63 and (big + 1) * qr.S[60] < 2 ** 63          # the products stay below 2^63
    for a in (0, 1, 65535, 2 ** 31, 2 ** 32 - 1):
        assert lib.pba_qual_phred(a, big, 60) == qr.phred(a, big)
    assert lib.pba_qual_phred(65535, big, 60) == 0 and lib.pba_qual_phred(2 ** 32 - 1, big, 60) == 60
    for a, n in ((9, 5), (65535, 1), (2 ** 32 - 1, 0)):                            # agree > N: nothing stands against
        assert lib.pba_qual_phred(a, n, 60) == qr.phred(a, n) == qr.phred(n, n)
    for qmax in (-1, 61):
        assert lib.pba_qual_phred(20, 20, qmax) == -1 and qr.phred(20, 20, qmax) == -1 and eng.qual_phred(20, 20, qmax) == -1
    assert lib.pba_qual_phred(20, 20, 0) == 0 and lib.pba_qual_phred(20, 20, 10) == 10 and lib.pba_qual_phred(20, 20, 60) == 13


def box(sel=(0, 0, 0, 0), sup=(0, 0, 0, 0), tot=1):
    return list(sel), list(sup), tot


def run_evidence(boxes, weight, qmax=60):
    sel, sup, tot = (np.array([b[k] for b in boxes]) for k in range(3))
    return qr.evidence(sel.astype(np.uint16), sup.astype(np.uint16), tot.astype(np.int32), weight, qmax)


@pytest.mark.parametrize("weight", [1, 3, 65535])
def test_evidence_on_hand_built_boxes(weight):
    w = weight
    hi3, hi4 = min(w + 3, 65535), min(w + 4, 65535)          # (a counter holds weight + votes <= 65 535)
    boxes = [
        box(sel=(w, 0, 0, 0), tot=1),                        # 0: fresh, nobody voted: V only
        box(sel=(hi3, 0, 1, 0), tot=5),                      # 1: V only, 4 rows, one against
        box(sel=(0, 2, 0, 0), tot=4),                        # 2: a tie 2 * max == tot: neither (weight 1 stands for the lost own vote)
        box(sel=(0, 1, 0, 0), sup=(0, 0, 0, 3), tot=4),      # 3: S only
        box(sel=(0, 0, hi4, 0), sup=(5, 0, 0, 0), tot=5),    # 4: both, the selection's first; sup counter above tot - 1
        box(sel=(1, 1, 1, 1), sup=(1, 1, 0, 0), tot=5),      # 5: neither
        box(sel=(0, 0, 0, 2), sup=(0, 2, 0, 0), tot=3),      # 6: both at 2 of 3
    ]
    ev = run_evidence(boxes, weight)
    assert ev["text"] == b"AATGATC"
    assert ev["src"].tolist() == [0, 1, 3 | qr.SUP, 4, 4 | qr.SUP, 6, 6 | qr.SUP]
    assert ev["agree"].tolist() == [w, hi3, 3, hi4, 5, 2, 2]
    assert ev["depth"].tolist() == [0, 4, 3, 4, 4, 2, 2]
    n = [w, 4 + w, 3 + w, 4 + w, 4 + w, 2 + w, 2 + w]
    assert ev["qv"].tolist() == [qr.phred(a, x) for a, x in zip(ev["agree"].tolist(), n)]
    if weight == 1:
        # by hand: 1/3 -> 4; 2/7 -> S <= 3500: 5; 2/6 -> S <= 3000: 4; 1/7 -> S <= 7000: 8 (twice); 2/5 -> S <= 2500: 3 (twice)
        assert ev["qv"].tolist() == [4, 5, 4, 8, 8, 3, 3]
    if weight == 65535:
        assert ev["qv"][0] == 48 and ev["qv"][2] == qr.phred(3, 65538) == 0
    assert run_evidence(boxes, weight, 5)["qv"].tolist() == [min(5, q) for q in ev["qv"].tolist()]
    assert run_evidence(boxes, weight, 0)["qv"].tolist() == [0] * 7
    deep = run_evidence([box(sel=(65535, 0, 0, 0), tot=70000)], weight)          # depth saturates, agree does not pass u16
    assert deep["depth"].tolist() == [65535] and deep["agree"].tolist() == [65535] and len(deep["text"]) == 1 - (2 * 65535 <= 70000)
    empty = qr.evidence(np.zeros((0, 4), np.uint16), np.zeros((0, 4), np.uint16), np.zeros(0, np.int32), weight)
    assert empty["text"] == b"" and all(len(empty[k]) == 0 for k in ("qv", "depth", "agree", "src"))


def test_low_spans_and_summary_by_hand():
    #          seq 0 (6 bases)        seq 1 (empty)  seq 2 (4 bases)      seq 3 (3 bases)
    lengths = [6, 0, 4, 3]
    qv = [5, 20, 3, 4, 20, 2] + [1, 1, 30, 9] + [30, 30, 30]
    depth = [0, 7, 7, 9, 0, 1] + [2, 2, 2, 2] + [0, 0, 0]
    src = [0, 1, 2, 2 | qr.SUP, 3, 5] + [0, 1, 2, 3] + [0, qr.SUP, 1]
    sp = qr.low_spans(lengths, qv, 10, 1)
    # the run through seq 0's last base and seq 2's first bases are two spans: a run never crosses into the next sequence
    assert sp.tolist() == [(0, 0, 1, 5), (0, 2, 4, 3), (0, 5, 6, 2), (2, 0, 2, 1), (2, 3, 4, 9)]
    assert qr.low_spans(lengths, qv, 10, 2).tolist() == [(0, 2, 4, 3), (2, 0, 2, 1)]
    assert qr.low_spans(lengths, qv, 10, 3).tolist() == [] and qr.low_spans(lengths, qv, 0, 1).tolist() == []
    assert qr.low_spans(lengths, qv, 94, 1).tolist() == [(0, 0, 6, 2), (2, 0, 4, 1), (3, 0, 3, 30)]
    rows = qr.summary(lengths, qv, depth, src, 10)
    assert rows["seq"].tolist() == [0, 1, 2, 3] and rows["len"].tolist() == lengths
    assert rows["n_sel"].tolist() == [5, 0, 4, 2] and rows["n_sup"].tolist() == [1, 0, 0, 1]
    assert rows["n_unvoted"].tolist() == [2, 0, 0, 3] and rows["n_below"].tolist() == [4, 0, 3, 0]
    assert rows["n_low_runs"].tolist() == [3, 0, 2, 0] and rows["min_qv"].tolist() == [2, -1, 1, 30]
    assert rows["max_depth"].tolist() == [9, 0, 2, 0] and rows["sum_qv"].tolist() == [54, 0, 41, 90]
    assert rows["sum_depth"].tolist() == [24, 0, 8, 0] and not rows["pad"].any()
    assert qr.ROW_DTYPE == eng.QUAL_ROW_DTYPE and qr.SPAN_DTYPE == eng.QUAL_SPAN_DTYPE


def test_fastq_image_by_hand():
    texts = [b"ACGT", b"", b"TT"]
    quals = [[0, 1, 60, 93], [], [9, 10]]
    assert qr.fastq_image(texts, quals) == b"@0\nACGT\n+\n!\"]~\n@1\n\n+\n\n@2\nTT\n+\n*+\n"
    assert qr.fastq_image(texts[1:], quals[1:], first_id=1) == b"@1\n\n+\n\n@2\nTT\n+\n*+\n"
    assert qr.fastq_image(texts, quals, names=["r one", b"e", 7]) == b"@r one\nACGT\n+\n!\"]~\n@e\n\n+\n\n@7\nTT\n+\n*+\n"
    assert eng.fastx_sniff(qr.fastq_image(texts, quals)) == eng.PBA_FX_FASTQ
