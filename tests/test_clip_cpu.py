"""tests/clip_ref.py -- the clip rule of DESIGN §5.8 in plain Python, the expectation pba_clip_* is held to on the device
(tests/test_gpu_clip.py) -- pinned without a GPU: on cases computed by hand, and on a read set with planted chimeras and
junk tails whose rows come from the CPU oracle the way the engine's overlapper composes them.  The structural conditions
the GPU end-to-end test relies on are proven here, for the same input, before any device is involved."""
import pytest

from clip_ref import (CUT, DROPPED, HAND_CASES, PLANTED, PLANTED_CHIMERAS_SPANNED_MAX, WHOLE, clip_ref, entries, hand_texts, make_rows,
                      n_chunks, planted_reads, planted_report, runs_of)
from conftest import MASK_PAT
from correct_helpers import oracle_rows
from pacbioassembly_amd import engine as eng


@pytest.mark.parametrize("case", HAND_CASES, ids=[c["name"] for c in HAND_CASES])
def test_reference_on_hand_cases(lib, case):
    """Expected tables and counters are written out in HAND_CASES with their arithmetic."""
    texts = hand_texts(case)
    got = clip_ref(case["lens"], make_rows(case["rows"]), case["margin"], case["min_cov"], case["min_len"], case["flags"], texts)
    assert got["table"] == case["table"]
    assert got["stats"] == case["stats"]
    assert [len(t) for t in got["texts"]] == [row[3] - row[2] for row in got["table"]]
    st = got["stats"]
    assert st["n_whole"] + st["n_cut"] + st["n_dropped"] == len(case["lens"])


def test_reference_pieces_by_hand(lib):
    assert runs_of([0, 2, 2, 1, 3, 0, 2], 2) == [(1, 3), (4, 5), (6, 7)] and runs_of([], 1) == [] and runs_of([1, 1], 1) == [(0, 2)]
    assert [entries(L) for L in (0, 2, 3, 4, 6, 7)] == [4, 4, 4, 8, 8, 8]
    lens = [3, 3, 10, 3]                                      # entries 4, 4, 12, 4
    assert [n_chunks(lens, b) for b in (1, 4, 8, 12, 16, 19, 20, 24)] == [4, 4, 3, 3, 2, 2, 2, 1]
    # coverage spelled out: one interval [2, 9) at margin 2 covers [4, 7)
    got = clip_ref([10, 10], make_rows([(0, 1, 1, 0, 2, 9, 0, 7)]), 2, 1, 0, 1)
    assert got["cov"][0] == [0, 0, 0, 0, 1, 1, 1, 0, 0, 0] and got["table"][0] == (0, CUT, 2, 9, 1, 1, 1, 3)
    assert got["table"][1] == (1, DROPPED, 0, 0, 0, 0, 0, 0)


def test_reference_on_planted_reads(lib, oracle):
    """The planted input of tests/test_gpu_clip.py::test_end_to_end_planted with the rows from the CPU oracle.  Conditions:
    no planted chimera stays WHOLE; at most PLANTED_CHIMERAS_SPANNED_MAX of them keep both J - margin and J + margin.
    What happens to clean reads is printed, never asserted: the overlapper's recall on 1.5 kb reads at 15 % error is low."""
    P = PLANTED
    texts, chim, junk = planted_reads()
    assert len(texts) == P["n"] and len(chim) >= 10 and len(junk) >= 10
    rows = oracle_rows(oracle, texts, eng.mask_from_pattern(MASK_PAT), P["R"], nthreads=16)
    got = clip_ref([len(t) for t in texts], rows, P["margin"], P["min_cov"])
    rep = planted_report(got["table"], chim, junk, P["margin"])
    print(len(rows), "rows;", rep, got["stats"])
    for i, J in sorted(chim.items()):
        print("chimera", i, "junction", J, "of", len(texts[i]), "->", got["table"][i])
    for i, (lo, hi) in sorted(junk.items()):
        print("junk", i, (lo, hi), "of", len(texts[i]), "->", got["table"][i])
    assert rep["chimeras_whole"] == 0
    assert rep["chimeras_spanned"] <= PLANTED_CHIMERAS_SPANNED_MAX
    assert all(t[1] in (DROPPED, WHOLE, CUT) for t in got["table"])
