"""Clipping reads to their overlap-supported span on the device (pba_clip_*): the per-read table, the counters,
the coverage of single reads and the clipped set must be IDENTICAL to tests/clip_ref.py, the rule restated sequentially
(tests/test_clip_cpu.py pins that reference by hand and proves the planted input's conditions).  Needs a real MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

from clip_ref import (ACGT, COUNTERS, CUT, DROPPED, HAND_CASES, KEEP_UNSEEN, PLANTED, PLANTED_CHIMERAS_SPANNED_MAX, QUERIES, ROW_FIELDS,
                      STEP, TARGETS, WHOLE, clip_ref, entries, hand_texts, make_rows, n_chunks, planted_reads, planted_report)
from conftest import MASK_PAT
from correct_helpers import oracle_rows
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PbaError

pytestmark = pytest.mark.gpu


def exported(ctx, S):
    """The packed arena of a set (pba_seqs_export) and its offsets, on the host (tests/test_gpu_layout.py: exported)."""
    import torch
    buf = torch.zeros(max(S.packed_bytes, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs = S.export(buf.data_ptr(), buf.numel())
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:S.packed_bytes].tobytes(), offs.tolist()


def same_set(ctx, got, want, texts):
    assert got.count == want.count and got.max_len == want.max_len
    assert got.lengths().tolist() == want.lengths().tolist() == [len(t) for t in texts]
    for i in range(0, want.count, max(1, want.count // 64)):
        assert got.get_text(i) == texts[i], i
    assert exported(ctx, got) == exported(ctx, want)          # byte for byte, pad bits and layout included


def clip(ctx, S, rows, margin, min_cov, min_len=0, flags=TARGETS | QUERIES, max_bases=0):
    return ctx.clip(S, rows, margin, min_cov, min_len, flags & 3, bool(flags & KEEP_UNSEEN), max_bases)


def check_against_ref(ctx, texts, rows, margin, min_cov, min_len=0, flags=TARGETS | QUERIES, max_bases=0, S=None, want=None, cov_of=(),
                      apply=True):
    """Clip on the device == the reference: table, counters, coverage of the reads in cov_of, the clipped set (byte for byte).
    Returns (reference result, device table, device stats)."""
    lens = [len(x) for x in texts]
    want = want if want is not None else clip_ref(lens, rows, margin, min_cov, min_len, flags, texts)
    S = S if S is not None else ctx.seqs_from_list(texts, strict_acgt=True)
    cl = clip(ctx, S, rows, margin, min_cov, min_len, flags, max_bases)
    table = cl.rows()
    assert [tuple(int(r[f]) for f in ROW_FIELDS) for r in table] == want["table"]
    st = cl.stats
    assert {k: int(st[k]) for k in COUNTERS} == want["stats"]
    for x in cov_of:
        assert ctx.clip_coverage(S, rows, x, margin, flags & 3).tolist() == want["cov"][x], x
    if apply:
        same_set(ctx, cl.apply(S), ctx.seqs_from_list(want["texts"]), want["texts"])
        assert cl.stats["gather_ms"] > 0 or not want["stats"]["n_bases_out"]
    cl.close()
    return want, table, st


@pytest.mark.parametrize("case", HAND_CASES, ids=[c["name"] for c in HAND_CASES])
def test_hand_rows(ctx, case):
    """Rows written by hand (tests/clip_ref.py: HAND_CASES, with the arithmetic next to each): cov == c and c - 1, margin 0
    with the -1 on entry L, intervals of 2m and 2m + 1 bases, kept length == min_len and min_len - 1, KEEP_UNSEEN on and off
    for an unseen read shorter than min_len, the three role masks, a strand -1 row used as given, two equal runs."""
    want, _, _ = check_against_ref(ctx, hand_texts(case), make_rows(case["rows"]), case["margin"], case["min_cov"], case["min_len"],
                                   case["flags"], cov_of=range(len(case["lens"])))
    assert want["table"] == case["table"] and want["stats"] == case["stats"]


S_ = STEP
EDGE_LENS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, S_ - 1, S_, S_ + 1, 2 * S_ - 1, 2 * S_, 2 * S_ + 1, 70001]


def edge_rows():
    """Target intervals on the reads of EDGE_LENS (read k has length EDGE_LENS[k]); at margin 0 and min_cov 1 every interval
    is a run unless two touch.  The query of every row is another read whose interval is not counted (TARGETS only)."""
    iv = {k: [(0, EDGE_LENS[k])] for k in (1, 2, 3, 4, 6, 7, 9, 10)}          # the whole read: position 0 and position L - 1
    iv[5] = [(1, 4)]                                                        # L = 5: neither end
    iv[8] = [(0, 64), (64, 65)]                                             # L = 65: two intervals that touch are ONE run
    iv[11] = [(0, 1), (256, 257)]                                           # L = 257: the first and the last position alone
    iv[12] = [(8 * k + 4, 8 * k + 8) for k in range(127)]                   # L = STEP - 1: a run from lane edge to lane edge, every second lane
    iv[13] = [(8 * k + 1, 8 * k + 6) for k in range(127)] + [(S_ - 5, S_)]  # L = STEP: runs inside lanes and across one lane edge; the last ends the read at the step edge
    iv[14] = [(0, 10), (S_ - 24, S_ + 1)]                                   # L = STEP + 1: across the step edge to L - 1
    iv[15] = [(256 * w - 5, 256 * w) if w & 1 else (256 * w, 256 * w + 5) for w in range(1, 8)]   # ends / starts at every wavefront edge (w = 4: starts at the step edge)
    iv[16] = [(S_ - 7, S_), (S_ + 3, S_ + 10)]                              # two runs of 7 in different steps: the smaller start wins; one ends at the step edge
    iv[17] = [(10, 20), (S_ + 500, S_ + 600), (2 * S_, 2 * S_ + 1)]         # a longer run after a shorter one wins; the last step holds one position
    iv[18] = [(0, 50), (S_ - 10, 2 * S_ + 10),                              # touches 0; spans three steps (steps 3 and 4 hold nothing)
              (5 * S_ + 100, 5 * S_ + 200), (10 * S_, 10 * S_ + 1), (20 * S_ - 1, 20 * S_),   # one position at a step's start, one at a step's end
              (30 * S_, 31 * S_), (69000, 70001)]                           # exactly one whole step; touches L - 1
    out = []
    for k, ivs in sorted(iv.items()):
        q = 17 if k == 18 else 18
        out += [(k, q, 1 if (k + b) & 1 else -1, 0, b, e, 0, 1) for b, e in ivs]
    return out


def test_sweep_edges(ctx):
    """Runs at every lane, wavefront and step edge of k_clip_sweep, in reads of 0 .. 70 001 bases (the long one is swept by
    its one workgroup in 69 steps)."""
    rng = np.random.default_rng(401)
    texts = [rng.choice(ACGT, n).tobytes() for n in EDGE_LENS]
    tup = edge_rows()
    rows = make_rows([tup[int(k)] for k in rng.permutation(len(tup))])
    want, _, _ = check_against_ref(ctx, texts, rows, 0, 1, 0, TARGETS, cov_of=(5, 8, 13, 15, 18))
    T = want["table"]
    assert T[0] == (0, DROPPED, 0, 0, 0, 0, 0, 0)
    assert all(T[k][1:4] == (WHOLE, 0, EDGE_LENS[k]) for k in (1, 2, 3, 4, 6, 7, 8, 9, 10)) and T[8][4:6] == (2, 1)
    assert T[5][1:4] == (CUT, 1, 4) and T[11][1:4] == (CUT, 0, 1) and T[11][5] == 2
    assert T[12][1:4] == (CUT, 4, 8) and T[12][5] == 127 and T[12][7] == 4 * 127
    assert T[13][1:4] == (CUT, 1, 6) and T[13][5] == 128
    assert T[14][1:4] == (CUT, S_ - 24, S_ + 1) and T[15][1:4] == (CUT, 251, 256) and T[15][5] == 7
    assert T[16][1:4] == (CUT, S_ - 7, S_) and T[17][1:4] == (CUT, S_ + 500, S_ + 600)
    assert T[18][1:4] == (CUT, S_ - 10, 2 * S_ + 10) and T[18][5] == 7
    # the same intervals under a margin and at a threshold of 2 (every row twice: cov == c; with one of them once: c - 1)
    check_against_ref(ctx, texts, rows, 2, 1, 3, TARGETS, cov_of=(12, 18))
    lone = rows["target"] == 5                                # read 5's only interval stays at cov 1 = c - 1
    want2, _, _ = check_against_ref(ctx, texts, np.concatenate([rows, rows[~lone]]), 0, 2, 0, TARGETS, cov_of=(5, 18))
    assert want2["table"][5] == (5, DROPPED, 0, 0, 1, 0, 1, 0)
    assert [t[:4] + t[5:6] + t[7:] for t in want2["table"] if t[0] != 5] == [t[:4] + t[5:6] + t[7:] for t in T if t[0] != 5]


def test_margin_and_threshold_edges(ctx):
    """What HAND_CASES leaves: the kept interval reaching 0 and L exactly, and every margin / threshold around one pile.
    (max(s - m, 0) and min(e + m, L) can never bind with valid rows: a run starts at some b + m and ends at some e - m, so
    s - m = b >= 0 and e + m <= L; the kernel keeps the clamp for the reason the rule states it.)"""
    lens = [100, 100, 40]
    texts = [np.random.default_rng(402).choice(ACGT, n).tobytes() for n in lens]
    tup = [(0, 1, 1, 0, 0, 100, 0, 100), (0, 1, -1, 0, 0, 100, 0, 100), (1, 0, 1, 0, 5, 97, 0, 92), (0, 1, 1, 0, 30, 70, 10, 50)]
    rows = make_rows(tup)
    for margin in (0, 1, 19, 20, 21, 49, 50, 51):
        for min_cov in (1, 2, 3, 4, 5, 6):
            for flags in (TARGETS | QUERIES, TARGETS | QUERIES | KEEP_UNSEEN):
                want, _, _ = check_against_ref(ctx, texts, rows, margin, min_cov, 30, flags, cov_of=(0,), apply=margin in (0, 20))
    want, _, _ = check_against_ref(ctx, texts, rows, 10, 2, 0, TARGETS)
    assert want["table"][0][:4] == (0, WHOLE, 0, 100) and want["table"][1][1] == DROPPED      # kept reaches 0 and L exactly
    want, _, _ = check_against_ref(ctx, texts, rows, 10, 1, 0, TARGETS)
    assert want["table"][1][:4] == (1, CUT, 5, 97)


def test_many_identical_intervals_on_one_read(ctx):
    """5 000 rows with the same intervals: 10 000 atomic adds on the same two entries of each read."""
    texts = [np.random.default_rng(403).choice(ACGT, n).tobytes() for n in (300, 50)]
    rows = make_rows([(0, 1, 1, 0, 20, 280, 0, 50)] * 5000)
    want, _, _ = check_against_ref(ctx, texts, rows, 5, 5000, cov_of=(0, 1))
    assert want["table"] == [(0, CUT, 20, 280, 5000, 1, 5000, 250), (1, WHOLE, 0, 50, 5000, 1, 5000, 40)]
    want, _, _ = check_against_ref(ctx, texts, rows, 5, 5001)
    assert want["stats"]["n_dropped"] == 2 and want["table"][0][6] == 5000


@pytest.fixture(scope="module")
def fuzz():
    """About 300 reads of 0 .. 2 600 bases (some longer than a step, two empty) and 20 000 random valid rows: nothing to do
    with real overlaps.  The references for the three role masks are computed once."""
    rng = np.random.default_rng(404)
    lens = [int(x) for x in rng.integers(40, 400, 300)]
    for k in (7, 90, 201):
        lens[k] = int(rng.integers(STEP + 1, 2600))
    lens[33] = lens[150] = 0
    lens[299] = 2 * STEP
    texts = [rng.choice(ACGT, n).tobytes() for n in lens]
    live = [k for k, n in enumerate(lens) if n > 0]
    tup = []
    while len(tup) < 20000:
        t, q = (live[int(x)] for x in rng.integers(0, len(live), 2))
        if t == q:
            continue
        tb, te = sorted(rng.choice(lens[t] + 1, 2, replace=False))
        qb, qe = sorted(rng.choice(lens[q] + 1, 2, replace=False))
        tup.append((t, q, int(rng.choice((1, -1))), 0, int(tb), int(te), int(qb), int(qe)))
    rows = make_rows(tup)
    want = {f: clip_ref(lens, rows, 12, 12, 25, f, texts) for f in (TARGETS, QUERIES, TARGETS | QUERIES)}
    return texts, rows, want


@pytest.mark.parametrize("flags", [TARGETS, QUERIES, TARGETS | QUERIES])
def test_fuzz_roles(ctx, fuzz, flags):
    """The same rows with roles 1, 2 and 3: table, counters, the clipped set, the coverage of sampled reads."""
    texts, rows, want = fuzz
    w, _, _ = check_against_ref(ctx, texts, rows, 12, 12, 25, flags, want=want[flags], cov_of=(0, 7, 33, 201, 299))
    st = w["stats"]
    assert st["n_iv"] == (2 if flags == 3 else 1) * 20000 and st["n_iv_short"] > 500
    assert st["n_cut"] > 100 and st["n_multi_run"] > 10 and st["n_dropped"] >= 2


def test_chunks(ctx, fuzz):
    """The fuzz under max_bases = 0 (one chunk), = the entries of an empty read (one read per chunk), = the longest read's
    entries, = a third of all entries: the same table and counters, n_chunks as predicted from the lengths."""
    texts, rows, want = fuzz
    lens = [len(t) for t in texts]
    total = sum(entries(n) for n in lens)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    for max_bases, chunks in ((0, 1), (entries(0), len(lens)), (entries(max(lens)), None), (total // 3, None), (total, 1), (total - 1, 2)):
        _, _, st = check_against_ref(ctx, texts, rows, 12, 12, 25, 3, max_bases=max_bases, S=S, want=want[3], apply=False)
        assert st["n_chunks"] == (chunks if chunks is not None else n_chunks(lens, max_bases)), max_bases
    assert n_chunks(lens, entries(max(lens))) > 20 and n_chunks(lens, total // 3) in (3, 4)


def test_gather_packing_edges(ctx):
    """Kept intervals of 0 .. 33 bases beginning at every residue mod 16, longer ones at every residue, the 70 001-base read
    cut at both ends, dropped reads between kept ones: byte for byte what seqs_from_list makes of the sliced texts."""
    rng = np.random.default_rng(405)
    lens, tup = [], []
    for k in range(34):                                       # kept length k (0: no row, the read is dropped)
        lens.append(120)
        if k:
            b = (5 * k) % 16 + 16 * (k % 3)
            tup.append((k, 0, 1, 0, b, b + k, 0, 1))
    for r in range(16):                                       # longer than a group, from every residue
        lens.append(200)
        tup.append((34 + r, 0, -1, 0, r, r + 40 + 3 * r, 0, 1))
    lens += [70001, 30, 64]                                   # reads 50, 51 (no row: dropped between two kept ones), 52
    tup += [(50, 0, 1, 0, 7, 69990, 0, 1), (52, 0, 1, 0, 0, 64, 0, 1)]
    texts = [rng.choice(ACGT, n).tobytes() for n in lens]
    want, table, _ = check_against_ref(ctx, texts, make_rows(tup), 0, 1, 0, TARGETS)
    assert sorted({int(r["beg"]) % 16 for r in table if r["state"] != DROPPED}) == list(range(16))
    assert [len(t) for t in want["texts"][:34]] == list(range(34)) and len(want["texts"][50]) == 69983
    assert want["table"][51][1] == DROPPED and want["table"][52][1] == WHOLE and want["stats"]["n_dropped"] == 2


def test_empty_set_and_empty_rows(ctx):
    none = make_rows([])
    want, table, st = check_against_ref(ctx, [], none, 10, 2)
    assert table.size == 0 and st["n_chunks"] == 0
    texts = [b"ACGTACGTAC", b"", b"TTG"]
    want, _, _ = check_against_ref(ctx, texts, none, 10, 2)
    assert want["stats"]["n_dropped"] == 3 and want["texts"] == [b"", b"", b""]
    want, _, _ = check_against_ref(ctx, texts, none, 10, 2, 5, TARGETS | KEEP_UNSEEN)
    assert want["stats"]["n_whole"] == want["stats"]["n_unseen"] == 3 and want["texts"] == texts


def test_refusals(ctx):
    """Every refusal gives its status, and a valid call on the same ctx succeeds afterwards."""
    case = HAND_CASES[0]
    texts = hand_texts(case)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    good = case["rows"][0]

    def status(rows, margin=10, min_cov=2, min_len=0, roles=3):
        with pytest.raises(PbaError) as e:
            ctx.clip(S, make_rows(rows), margin, min_cov, min_len, roles)
        return e.value.status

    bad_rows = {
        "target == query": (0, 0, 1, 0, 40, 100, 0, 60), "target outside": (2, 1, 1, 0, 40, 100, 0, 60),
        "query negative": (0, -1, 1, 0, 40, 100, 0, 60), "t interval beyond its read": (0, 1, 1, 0, 40, 101, 0, 60),
        "q interval negative": (0, 1, 1, 0, 40, 100, -1, 60), "t interval empty": (0, 1, 1, 0, 40, 40, 0, 60),
        "q interval reversed": (0, 1, 1, 0, 40, 100, 60, 0), "strand 0": (0, 1, 0, 0, 40, 100, 0, 60), "strand 2": (0, 1, 2, 0, 40, 100, 0, 60),
    }
    for what, row in bad_rows.items():
        assert status([good, row]) == -1, what
        with pytest.raises(PbaError) as e:
            ctx.clip_coverage(S, make_rows([good, row]), 0)
        assert e.value.status == -1, what
    assert status([good], margin=-1) == -1 and status([good], min_cov=0) == -1 and status([good], min_len=-1) == -1
    assert status([good], roles=0) == -1 and status([good], roles=8) == -1 and status([good], roles=16 | 1) == -1
    for kw in (dict(margin=-1), dict(roles=0), dict(roles=8 | 1), dict(read=2)):
        with pytest.raises(PbaError) as e:
            ctx.clip_coverage(S, make_rows([good]), **{"read": 0, **kw})
        assert e.value.status == -1, kw
    check_against_ref(ctx, texts, make_rows(case["rows"]), case["margin"], case["min_cov"], S=S, flags=case["flags"])
    cl = ctx.clip(S, make_rows(case["rows"]), case["margin"], case["min_cov"], roles=case["flags"])
    for other in ([texts[0]], [texts[0], texts[1][:-1]], texts + [b"ACGT"]):             # another count, other lengths
        with pytest.raises(PbaError) as e:
            cl.apply(ctx.seqs_from_list(other, strict_acgt=True))
        assert e.value.status == -1
    out = np.zeros(2, eng.CLIP_ROW_DTYPE)
    assert ctx.lib.pba_clip_rows(ctx.h, cl.h, C.c_void_p(out.ctypes.data), 1) == -1          # room for one row of two
    cov, n = np.full(8, -7, np.int32), C.c_uint32()
    rows = make_rows(case["rows"])
    assert ctx.lib.pba_clip_coverage(ctx.h, S.h, C.c_void_p(rows.ctypes.data), rows.size, 10, 1, 0, C.c_void_p(cov.ctypes.data), 7, C.byref(n)) == 0
    assert n.value == 100 and cov[:7].tolist() == [0] * 7 and cov[7] == -7                   # cap below L: L reported, cap written
    # bytes outside ACGT: create reads only the lengths; apply would give code 3 back as T
    with_n = ctx.seqs_from_list([texts[0], texts[1][:50] + b"N" + texts[1][51:]])
    cl_n = ctx.clip(with_n, rows, case["margin"], case["min_cov"], roles=case["flags"])
    assert [tuple(int(r[f]) for f in ROW_FIELDS) for r in cl_n.rows()] == case["table"]
    with pytest.raises(PbaError) as e:
        cl_n.apply(with_n)
    assert e.value.status == -6                                                              # PBA_E_ALPHABET
    cl_n.close()
    same_set(ctx, cl.apply(S), ctx.seqs_from_list([texts[0][20:60], b""]), [texts[0][20:60], b""])
    cl.close()


def test_end_to_end_planted(ctx, oracle):
    """The planted input of tests/test_clip_cpu.py::test_reference_on_planted_reads through Context.clip_reads: the rows are
    the oracle's, the table is the reference's, the clipped set is the sliced texts -- so the structural conditions proven
    there on the CPU hold here by equality (and are asserted again)."""
    P = PLANTED
    texts, chim, junk = planted_reads()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    mask = eng.mask_from_pattern(MASK_PAT)
    clipped, table, rows, stats = ctx.clip_reads(S, mask, P["R"], margin=P["margin"], min_cov=P["min_cov"], targets_per_call=50)
    want_rows = oracle_rows(oracle, texts, mask, P["R"], nthreads=16)
    assert np.array_equal(rows, want_rows)
    want = clip_ref([len(t) for t in texts], rows, P["margin"], P["min_cov"], texts=texts)
    assert [tuple(int(r[f]) for f in ROW_FIELDS) for r in table] == want["table"]
    assert {k: int(stats[k]) for k in COUNTERS} == want["stats"]
    same_set(ctx, clipped, ctx.seqs_from_list(want["texts"]), want["texts"])
    rep = planted_report(want["table"], chim, junk, P["margin"])
    print(len(rows), "rows;", rep, stats)
    assert rep["chimeras_whole"] == 0 and rep["chimeras_spanned"] <= PLANTED_CHIMERAS_SPANNED_MAX
