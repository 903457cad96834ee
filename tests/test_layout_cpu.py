"""tests/layout_ref.py -- the layout semantics of DESIGN §5.6 in plain Python, the expectation pba_layout_* is held to on the
device (tests/test_gpu_layout.py) -- pinned without a GPU: on cases computed by hand, on a synthetic tiling whose answer is
known from the read starts, and on rows composed from the CPU oracle the way the engine's overlapper composes them."""
import numpy as np
import pytest

from conftest import MASK_PAT
from layout_ref import CONTAINED, HAND_CASES, PLACED, combine, hand_texts, layout_ref, make_rows, rc, tiling
from pacbioassembly_amd import engine as eng


@pytest.mark.parametrize("case", HAND_CASES, ids=[c["name"] for c in HAND_CASES])
def test_reference_on_hand_cases(lib, case):
    """The four dovetail orientations, a reversed middle read, containment and refused containment, dropped dovetails, the
    container's row, the tie-breaks, a best edge that is not mutual, the hang threshold, min_reads, rings of five and two:
    expected tables, contigs and counters are written out in HAND_CASES with their arithmetic."""
    texts = hand_texts(case)
    got = layout_ref(case["lens"], make_rows(case["rows"]), case["hang"], case["min_reads"], texts)
    assert got["table"] == case["table"]
    assert got["contigs"] == case["contigs"]
    assert got["stats"] == case["stats"]
    # the texts follow from the table: every placed read supplies [skip, skip + adv) of its walked text at `offset`
    for (head, n_reads, length), text in zip(got["contigs"], got["texts"]):
        assert len(text) == length
    for r, state, contig, rank, orient, offset, skip, adv, container in got["table"]:
        if state == PLACED:
            x = rc(texts[r]) if orient else texts[r]
            assert got["texts"][contig][offset:offset + adv] == x[skip:skip + adv]


def test_reference_hand_texts_spelled_out(lib):
    """two of the hand cases down to the bases"""
    by_name = {c["name"]: c for c in HAND_CASES}
    c = by_name["three_reads_middle_reversed"]
    t = hand_texts(c)
    got = layout_ref(c["lens"], make_rows(c["rows"]), c["hang"], c["min_reads"], t)
    assert got["texts"] == [t[0] + rc(t[1])[60:] + t[2][50:]]
    c = by_name["ring_of_five"]
    t = hand_texts(c)
    got = layout_ref(c["lens"], make_rows(c["rows"]), c["hang"], c["min_reads"], t)
    assert got["texts"] == [t[0] + t[2][60:] + t[3][60:] + t[1][60:] + t[4][60:]]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_reference_on_a_synthetic_tiling(lib, seed):
    """Error-free reads of 1 300 bases starting every 150-400 bases of a 9 000-base genome, random strands, shuffled ids;
    exact cost-0 rows from the known starts in both views.  One contig: the covered span, forward when the traversal starts
    at the leftmost read (whatever that read's strand: it is then walked in the orientation that undoes it) and
    reverse-complemented when it starts at the rightmost."""
    rng = np.random.default_rng(seed)
    steps = []
    while sum(steps) + 1300 + 400 <= 9000:
        steps.append(int(rng.integers(150, 401)))
    n = len(steps) + 1
    til = tiling(rng, [1300] * n, steps, min_ov=64)
    genome, starts, flips = til[0], til[1], til[2]
    texts, rows, ids = combine(rng, [til])
    new = ids[0]
    got = layout_ref([len(x) for x in texts], rows, 64, 2, texts)
    assert len(got["contigs"]) == 1 and got["stats"]["n_placed"] == n and got["stats"]["n_cycles"] == 0
    head, n_reads, length = got["contigs"][0]
    assert n_reads == n and length == len(genome) == starts[-1] + 1300
    assert head == min(int(new[0]), int(new[-1]))
    from_left = head == int(new[0])
    assert got["texts"][0] == (genome if from_left else rc(genome))
    orient = got["table"][head][4]
    assert orient == (int(flips[0]) if from_left else 1 - int(flips[-1]))        # the head read's strand decides how it is walked
    ranks = [got["table"][int(k)][3] for k in new]
    assert ranks == (list(range(n)) if from_left else list(range(n - 1, -1, -1)))
    assert got["stats"]["n_internal"] == 0 and got["stats"]["n_contain"] == 0 and got["stats"]["n_mated_ends"] == 2 * (n - 1)


def oracle_rows(oracle, texts, mask, R=0.30, max_trial=32, overlap_min=64):
    """pba_overlap_strands rows composed from the CPU oracle: every read as the locked reference of a spaced_seed round over
    the file of the reads (strand +1) and of their reverse complements (strand -1), sorted by (target, query), +1 first;
    intervals as include/pba.h gives them."""
    n = len(texts)
    files = []
    for tx in (texts, [rc(x) for x in texts]):
        offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in tx[:-1]]).astype(np.uint64)
        files.append((b"".join(eng.text2bin(t) for t in tx), offs))
    out = []
    for t in range(n):
        per = [oracle.spaced_round(texts[t], mask, R, f, o, max_trial, overlap_min, buggy=False, nthreads=8) for f, o in files]
        for q in range(n):
            for strand, rows in ((1, per[0]), (-1, per[1])):
                if q == t or not rows["found"][q]:
                    continue
                j, d, pos, ma, mb = (int(rows[k][q]) for k in ("j", "dir", "ref_pos", "matlen_a", "matlen_b"))
                slen = len(texts[q])
                tb, te = (pos, pos + ma) if d == 1 else (pos + 16 - ma, pos + 16)
                qb, qe = (j, j + mb) if d == 1 else (slen - j - mb, slen - j)
                if strand == -1:
                    qb, qe = slen - qe, slen - qb
                out.append((t, q, strand, int(rows["cost"][q]), tb, te, qb, qe))
    return make_rows(out)


def test_reference_on_oracle_rows(lib, oracle):
    """The inputs of tests/test_gpu_layout.py::test_engine_rows (seeds 71 / 72 / 73), with the rows composed from the CPU
    oracle: no row is internal, every contig is a substring of the genome or of its reverse complement, and some contig
    holds at least 3 reads -- so that test's conditions are met by the reference alone, before any device is involved."""
    g = eng.synth_genome(71, 9000)
    reads, offs, _ = eng.synth_reads(72, g, 64, 1300, 0.0, 0.0, 0.0)
    texts = [reads[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(64)]
    flip = np.random.default_rng(73).permutation(64) < 32
    texts = [rc(x) if f else x for x, f in zip(texts, flip)]
    rows = oracle_rows(oracle, texts, eng.mask_from_pattern(MASK_PAT))
    got = layout_ref([1300] * 64, rows, 64, 2, texts)
    print("contig sizes (reads, bases):", [(c[1], c[2]) for c in got["contigs"]], got["stats"])
    assert len(rows) > 100 and got["stats"]["n_internal"] == 0
    genome = g.tobytes()
    assert got["texts"] and all(t in genome or t in rc(genome) for t in got["texts"])
    assert max(c[1] for c in got["contigs"]) >= 3
    assert all(s in (PLACED, CONTAINED, 0) for _, s, *_ in got["table"])
