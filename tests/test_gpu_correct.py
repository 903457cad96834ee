"""Read correction from overlap pile-ups on the device (pba_pileup_*, pba_correct_reads): every read takes the reference
role, its overlap rows vote on it, evolve gives the corrected read.  Held to the CPU oracle composed the same way
(tests/correct_helpers.py: ref_seq ctor, align with traceback, elect, evolve), box for box and byte for byte.  Needs a real
MI355X (-m gpu)."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import MASK_PAT, ROOT
from correct_helpers import check_dump_cap, mixed_reads, oracle_correct, rc
from pacbioassembly_amd import Pileup
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PAIR_DTYPE, PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP, PbaError

pytestmark = pytest.mark.gpu
KERNELS = [PBA_KERNEL_ROWSWEEP, PBA_KERNEL_BITVEC]
R = 0.30


def rows_by_target(rows, n):
    out = [[] for _ in range(n)]
    for r in rows:
        out[int(r["target"])].append(r)
    return out


def exported(S):
    import torch
    buf = torch.zeros(max(S.packed_bytes, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                  # the fill runs on torch's stream, the export on the engine's
    offs = S.export(buf.data_ptr(), buf.numel())
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:S.packed_bytes].tobytes(), offs.tolist()


def same_bytes(got, want):
    """Two exported sets are byte for byte the same (reports where they part, not two megabyte strings)."""
    assert got[1] == want[1] and len(got[0]) == len(want[0])
    if got[0] != want[0]:
        a, b = np.frombuffer(got[0], np.uint8), np.frombuffer(want[0], np.uint8)
        at = np.flatnonzero(a != b)
        seq = int(np.searchsorted(np.array(got[1]), at[0], side="right")) - 1
        raise AssertionError(f"{at.size} packed bytes differ, the first at {int(at[0])} (sequence {seq}, byte {int(at[0]) - got[1][seq]}): "
                             f"{a[at[0]]:#x} != {b[at[0]]:#x}")


def texts_of(S):
    return [S.get_text(i) for i in range(S.count)]


@pytest.fixture(scope="module")
def small_set():
    texts, _, flip = mixed_reads(401, 402, 250, 3000, 31000, rl_min=2000, extra=2)      # 250 reads of 2-3 kb at 20x, 2 unrelated
    return texts, flip


@pytest.mark.parametrize("weight", [1, 3])
@pytest.mark.parametrize("kernel", KERNELS)
def test_boxes_and_text_vs_oracle_every_target(ctx, oracle, small_set, kernel, weight):
    texts, flip = small_set
    n = len(texts)
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, mask, R, 32, 64, strands=3, kernel=kernel, reads_rc=Src)
    combos = collections.Counter((int(r["strand"]), int(r["dir"])) for r in rows)
    assert all(combos[(s, d)] > 0 for s in (1, -1) for d in (1, -1)), combos
    per = rows_by_target(rows, n)
    pile = Pileup(ctx, S, weight=weight)
    res = pile.vote(rows, R, reads_rc=Src)
    for c in ("cost", "matlen_a", "matlen_b"):
        assert (res[c] == rows[c]).all(), c
    want = [oracle_correct(oracle, texts, t, per[t], weight, R) for t in range(n)]
    for t in range(n):
        got = pile.dump(t)
        for x, y, name in zip(got, want[t][:3], ("sel", "sup", "tot")):
            assert x.shape == y.shape and (x == y).all(), (t, name)
    corrected, crows = pile.evolve()
    assert corrected.count == n and len(crows) == n
    changed = zero_rows = 0
    for t in range(n):
        got = corrected.get_text(t)
        assert got == want[t][3], t
        assert (int(crows[t]["target"]), int(crows[t]["n_rows"]), int(crows[t]["len_in"]), int(crows[t]["len_out"])) == \
               (t, len(per[t]), len(texts[t]), len(got)), t
        changed += got != texts[t]
        if not per[t]:
            zero_rows += 1
            assert got == texts[t], t                               # no votes: the read comes back as it went in
    assert changed * 2 >= n, (changed, n)
    assert zero_rows >= 1 and not per[n - 1] and not per[n - 2]     # the two unrelated reads at least
    for call in (lambda: pile.dump(0), lambda: pile.evolve(), lambda: pile.vote(rows[:1], R, reads_rc=Src)):   # spent
        with pytest.raises(PbaError) as e:
            call()
        assert e.value.status == -1


def test_15kb_reads(ctx, oracle):
    """400 reads x 15 kb at 20x (the band widths the headline kernels are instantiated for): every target corrected on the
    GPU, 8 of them compared with the oracle.  Some pairs must go to the second, reference-band pass of the voting kernel,
    and at least one of the 8 compared targets must own such a row: asserted from the profile of each vote batch."""
    texts, _, flip = mixed_reads(411, 412, 400, 15000, 300000)
    n = len(texts)
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, mask, R, 32, 64, strands=3, reads_rc=Src)
    per = rows_by_target(rows, n)
    pile = Pileup(ctx, S)
    voted = [t for t in range(n) if per[t]]
    assert len(voted) * 10 >= n * 9

    def vote(part):
        """One batch (rows of one strand): returns how many of its pairs the narrow pass could not certify and the
        reference-band launch re-ran (pba_profile.n_redo of the batch)."""
        if len(part) == 0:
            return 0
        pile.vote(part, R, reads_rc=Src)
        prof = ctx.last_profile()
        assert prof["n_first"] == len(part) and prof["nb_first"] > 0
        return int(prof["n_redo"])

    # 24 candidate targets are voted on their own, strand by strand, so that the targets owning re-run rows are known
    cands = [int(t) for t in np.random.default_rng(413).choice(voted, 24, replace=False)]
    redo_of = {}
    for t in cands:
        mine = np.array(per[t], rows.dtype)
        redo_of[t] = vote(mine[mine["strand"] == 1]) + vote(mine[mine["strand"] == -1])
    rest = rows[~np.isin(rows["target"], cands)]
    n_redo = sum(redo_of.values()) + vote(rest[rest["strand"] == 1]) + vote(rest[rest["strand"] == -1])
    print("pairs re-run at the reference band:", n_redo, "of", len(rows), "; per candidate target:", redo_of)
    assert n_redo > 0                                                   # the re-run path was really taken
    with_redo = [t for t in cands if redo_of[t] > 0]
    assert with_redo                                                    # ... and by rows of targets the oracle is asked about
    sample = (with_redo[:4] + [t for t in cands if redo_of[t] == 0] + with_redo[4:])[:8]
    assert len(sample) == 8 and any(redo_of[t] > 0 for t in sample)
    dumps = {t: pile.dump(t) for t in sample}
    corrected, crows = pile.evolve()
    assert [int(x) for x in crows["n_rows"]] == [len(p) for p in per]
    assert [int(x) for x in crows["len_in"]] == [len(x) for x in texts]
    assert corrected.lengths().tolist() == [int(x) for x in crows["len_out"]]
    for t in sample:
        sel, sup, tot, want = oracle_correct(oracle, texts, t, per[t], 1, R)
        for x, y, name in zip(dumps[t], (sel, sup, tot), ("sel", "sup", "tot")):
            assert (x == y).all(), (t, name)
        assert corrected.get_text(t) == want, t
    # the one-call form gives the same set
    again, crows2, st = ctx.correct_reads(S, mask, R, 32, 64, reads_rc=Src)
    assert (crows2 == crows).all()
    same_bytes(exported(again), exported(corrected))
    assert st[0]["n_overlaps"] + st[1]["n_overlaps"] == len(rows)


def test_same_answer_however_it_is_cut(ctx, small_set):
    texts, _ = small_set
    n = len(texts)
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    whole, wrows, wst = ctx.correct_reads(S, mask, R, 32, 64)            # reads_rc built inside
    want = texts_of(whole)
    assert whole.count == n and sum(t != x for t, x in zip(want, texts)) * 2 >= n
    # three unequal ranges
    got, grow = [], []
    for a, b in ((0, 7), (7, 8), (8, n)):
        part, prow, _ = ctx.correct_reads(S, mask, R, 32, 64, t_lo=a, t_hi=b, reads_rc=Src)
        assert part.count == b - a
        got += texts_of(part)
        grow.append(prow)
    assert got == want and (np.concatenate(grow) == wrows).all()
    # the pile-up driven by hand, rows shuffled and voted in two calls
    rows, _ = ctx.overlap_strands(S, mask, R, 32, 64, strands=3, reads_rc=Src)
    assert wst[0]["n_overlaps"] + wst[1]["n_overlaps"] == len(rows)
    sh = rows[np.random.default_rng(7).permutation(len(rows))]
    pile = Pileup(ctx, S)
    pile.vote(sh[:len(sh) // 3], R, reads_rc=Src)
    pile.vote(sh[len(sh) // 3:], R, reads_rc=Src)
    hand, hrow = pile.evolve()
    assert texts_of(hand) == want and (hrow == wrows).all()
    # the corrected set is byte for byte what seqs_from_list makes of its texts
    same_bytes(exported(whole), exported(ctx.seqs_from_list(want, strict_acgt=True)))
    same_bytes(exported(hand), exported(whole))
    # one strand only: other rows, and the rows it reports are that strand's
    plus, prow, pst = ctx.correct_reads(S, mask, R, 32, 64, strands=1)
    assert int(prow["n_rows"].sum()) == int((rows["strand"] == 1).sum()) == pst[0]["n_overlaps"] and pst[1]["n_overlaps"] == 0
    # the existing single-reference path on 10 targets: pba_cons_create + pba_cons_vote_pairs + pba_cons_evolve
    per = rows_by_target(rows, n)
    picks = [t for t in np.random.default_rng(8).permutation(n) if len(per[t]) >= 3][:10]
    assert len(picks) == 10
    for t in picks:
        c = eng.Consensus(ctx, texts[t], 1, max_len=len(texts[t]) + 64)
        for strand, B in ((1, S), (-1, Src)):
            pr = [eng.overlap_row_pair(r, len(texts[t]), len(texts[int(r["query"])])) for r in per[t] if int(r["strand"]) == strand]
            if pr:
                c.vote_pairs(S, int(t), B, np.array(pr, PAIR_DTYPE), R, 64)
        assert c.evolve() == want[t], t


def test_correct_reads_in_internal_chunks(ctx, small_set):
    """pba_correct_reads_budget with a ceiling on the boxes of a chunk: the range goes through in several chunks inside one
    call (texts stitched on the device, stats summed, rows_out per chunk) and gives what the one-chunk call gives; a ceiling
    below one read still takes a read per chunk; an empty range gives an empty set."""
    texts, _ = small_set
    n = len(texts)
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    whole, wrows, wst = ctx.correct_reads(S, mask, R, 32, 64, reads_rc=Src)
    assert ctx.last_correct_profile()["n_chunks"] == 1
    total = sum(len(x) for x in texts)
    for max_boxes, lo, hi in ((total // 5, 0, n), (1, 3, 40), (7000, 11, n)):
        part, prow, pst = ctx.correct_reads(S, mask, R, 32, 64, t_lo=lo, t_hi=hi, reads_rc=Src, max_boxes=max_boxes)
        prof = ctx.last_correct_profile()
        # the chunks the budget implies: consecutive reads while their bases fit, at least one read each
        want_chunks, boxes = 0, None
        for t in range(lo, hi):
            if boxes is None or boxes + len(texts[t]) > max_boxes:
                want_chunks, boxes = want_chunks + 1, 0
            boxes += len(texts[t])
        assert prof["n_chunks"] == want_chunks and want_chunks >= 5, (prof, want_chunks)
        assert prof["n_bases_in"] == sum(len(x) for x in texts[lo:hi]) and prof["n_rows"] == int(wrows["n_rows"][lo:hi].sum())
        assert part.count == hi - lo and (prow == wrows[lo:hi]).all()
        assert texts_of(part) == [whole.get_text(t) for t in range(lo, hi)]
        assert prof["n_bases_out"] == int(prow["len_out"].sum())
        same_bytes(exported(part), exported(ctx.seqs_from_list(texts_of(part), strict_acgt=True)))
        if (lo, hi) == (0, n):
            for k in (0, 1):
                for f in ("n_candidates", "n_pairs", "n_overlaps", "n_listed", "n_probe_entries"):
                    assert pst[k][f] == wst[k][f], (k, f)
    empty, erow, _ = ctx.correct_reads(S, mask, R, 32, 64, t_lo=9, t_hi=9, reads_rc=Src)
    assert empty.count == 0 and len(erow) == 0 and ctx.last_correct_profile()["n_chunks"] == 0


def test_refusals(ctx, small_set):
    texts, _ = small_set
    texts = texts[:60] + texts[-1:]
    n = len(texts)
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    rows, _ = ctx.overlap_strands(S, mask, R, 32, 64, strands=3, reads_rc=Src)
    inside = rows[(rows["target"] >= 10) & (rows["target"] < 30)]
    minus = inside[inside["strand"] == -1]
    assert len(inside) > 20 and len(minus) > 0 and (rows["target"] >= 30).any()
    pile = Pileup(ctx, S, 10, 30)
    pile.vote(inside[:5], R, reads_rc=Src)
    before = [pile.dump(t) for t in range(10, 30)]

    def unchanged():
        for t, b in zip(range(10, 30), before):
            assert all((x == y).all() for x, y in zip(pile.dump(t), b)), t

    def status(call):
        with pytest.raises(PbaError) as e:
            call()
        return e.value.status

    outside = np.concatenate([inside[5:8], rows[rows["target"] >= 30][:1]])
    assert status(lambda: pile.vote(outside, R, reads_rc=Src)) == -1              # a target outside [10, 30)
    unchanged()
    assert status(lambda: pile.vote(np.concatenate([inside[5:8], minus[:1]]), R)) == -1    # strand -1 without reads_rc
    unchanged()
    bad = inside[5:8].copy()
    bad["ref_pos"][1] = len(texts[int(bad["target"][1])])                      # accessor outside its read
    assert status(lambda: pile.vote(bad, R, reads_rc=Src)) == -1
    unchanged()
    N = ctx.seqs_from_list([x[:-1] + b"N" for x in texts])
    assert status(lambda: pile.vote(inside[5:8], R, reads_rc=N)) == -6             # a non-ACGT set
    unchanged()
    assert status(lambda: Pileup(ctx, N)) == -6
    assert status(lambda: ctx.correct_reads(N, mask, R)) == -6
    assert status(lambda: ctx.correct_reads(S, mask, R, reads_rc=N)) == -6
    assert status(lambda: Pileup(ctx, S, weight=0)) == -1 and status(lambda: Pileup(ctx, S, weight=0x10000)) == -1
    assert status(lambda: ctx.correct_reads(S, mask, R, weight=0)) == -1
    assert status(lambda: Pileup(ctx, S, 5, n + 1)) == -1
    assert status(lambda: pile.dump(30)) == -1 and status(lambda: pile.dump(9)) == -1
    # a dump into fewer slots than the target has boxes: 40 boxes, room for 7
    S40 = ctx.seqs_from_list([b"ACGTTGCAAC" * 4], strict_acgt=True)
    p40 = Pileup(ctx, S40, weight=3)
    check_dump_cap(lambda *a: ctx.lib.pba_pileup_dump(ctx.h, p40.h, 0, *a), p40.dump(0))
    other = ctx.seqs_from_list(texts[:-1], strict_acgt=True)                     # not the set of this pile-up
    pile_o = Pileup(ctx, other, 10, 30)
    assert status(lambda: pile_o.vote(inside[5:8], R, reads_rc=Src)) == -1
    # the pile-up still works after the refusals
    pile.vote(inside[5:], R, reads_rc=Src)
    fresh = Pileup(ctx, S, 10, 30)
    fresh.vote(inside, R, reads_rc=Src)
    assert texts_of(pile.evolve()[0]) == texts_of(fresh.evolve()[0])
    # a tampered cost: found when the row is re-run, i.e. after the batch has voted -- INVALID, and the pile-up is spent
    tam = inside[:4].copy()
    tam["cost"][2] += 1
    p2 = Pileup(ctx, S, 10, 30)
    with pytest.raises(PbaError) as e:
        p2.vote(tam, R, reads_rc=Src)
    assert e.value.status == -1 and "re-runs" in str(e.value)
    assert status(lambda: p2.dump(10)) == -1 and status(lambda: p2.evolve()) == -1


def test_bench_correct_tool():
    """tools/bench_correct.py on 2 000 reads x 3 kb: one JSON line with the stage times and rates, and correction brings the
    sampled reads closer to the genome they were drawn from (a property of the reference's vote at 20x, confirmed with the
    CPU oracle alone on this seed: see the numbers in DESIGN.md)."""
    p = subprocess.run(["timeout", "-k", "10", "540", sys.executable, os.path.join(ROOT, "tools", "bench_correct.py"), "--reads", "2000",
                        "--read-len", "3000", "--reps", "2"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    print(lines[0])
    for k in ("overlap_ms", "vote_ms", "evolve_ms"):
        assert out[k]["min"] > 0 and out[k]["min"] <= out[k]["median"] <= out[k]["max"], k
    assert out["rows_voted"] > 2000 and out["rows_voted_per_s"] > 0 and out["bases_corrected_per_s"] > 0
    assert out["bases_in"] == 2000 * 3000
    ts = out["truth_sample"]
    assert ts["targets"] == 200
    assert ts["mean_distance_after"] < ts["mean_distance_before"], ts
