"""pba_index_build_set and pba_map_reads: the seed index over every sequence of a set, and the locate against many contigs
on both strands of the reads.  The expected answer is never the engine's: the numpy index of tests/index_ref.py, the C
oracle's locator (one contig), and the plain restatement of tests/map_ref.py (many contigs; pinned to the oracle in
tests/test_map_ref_cpu.py).  Needs a real MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLD, MASK_PAT
from index_ref import np_index, runs
from map_ref import MANY_LENS, intervals, many_contig_case, map_reads_ref, merge_strands, rand_text, rc, repeat_case
from pacbioassembly_amd import _lib
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import MAP_ROW_DTYPE, PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP, PbaError

pytestmark = pytest.mark.gpu
KERNELS = [PBA_KERNEL_ROWSWEEP, PBA_KERNEL_BITVEC]
R = 0.30
SEED_MASKS = [l.strip() for l in open(f"{GOLD}/seeds.txt") if l.strip()]
ROW_COLS = ("read", "nseq", "found", "strand", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs",
            "r_beg", "r_end", "c_beg", "c_end")
STAT_COLS = ("n_pairs", "n_located", "n_probe_hits", "n_cells")


def same_rows(got, want, cols=ROW_COLS):
    for c in cols:
        bad = np.flatnonzero(got[c] != want[c])
        assert bad.size == 0, (c, bad[:8].tolist(), got[bad[:4]], want[bad[:4]])


def same_stats(got, want):
    for k in range(2):
        for c in STAT_COLS:
            assert got["strand"][k][c] == want[k][c], (k, c, got["strand"][k], want[k])


def raw_map_reads(ctx, ix, T, Rd, R, trials, min_len, kernel, strands, reads_rc=None):
    """The ctypes call itself: (status, rows, PbaMapStats)."""
    rows = np.zeros(max(Rd.count, 1), MAP_ROW_DTYPE)
    st = _lib.PbaMapStats()
    rc_h = reads_rc.h if reads_rc is not None else None
    status = ctx.lib.pba_map_reads(ctx.h, ix.h, T.h, Rd.h, rc_h, R, trials, min_len, 0, 0, kernel, strands,
                                   C.c_void_p(rows.ctypes.data), C.byref(st))
    return status, rows[:Rd.count], st


# ----------------------------------------------------------------------------- 1. the set index
@pytest.mark.parametrize("pat", [SEED_MASKS[0], SEED_MASKS[3], SEED_MASKS[7]])
def test_set_index(ctx, pat):
    """Contigs of 0, 7, 16, 17, 4 097 and 30 000 bases: dump and find give the per-contig reference lists shifted by cum[c],
    merged by key with contig order inside a key."""
    mask = eng.mask_from_pattern(pat)
    lens = [0, 7, 16, 17, 4097, 30000]
    rng = np.random.default_rng(900)
    contigs = [rand_text(rng, n) for n in lens]
    cum = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ents = []
    for c, t in enumerate(contigs):
        k, p, _ = np_index(t, mask, "all")
        ents.append((k.astype(np.uint64) << np.uint64(32)) | (p.astype(np.int64) + cum[c]).astype(np.uint64))
    e = np.sort(np.concatenate(ents))              # global positions ascend with (contig, pos): one sort is the merge
    wkeys, wpos = (e >> np.uint64(32)).astype(np.uint32), (e & np.uint64(0xFFFFFFFF)).astype(np.int32)
    assert wkeys.size > 30000 and (wpos >= cum[5]).any() and (wpos < cum[2]).any()
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    ix = ctx.index_build_set(T, mask)
    assert ix.seqs == len(lens) and ix.visited == int(cum[-1]) and ix.entries == wkeys.size
    keys, pos = ix.dump()
    assert (keys == wkeys).all() and (pos == wpos).all()
    dk, cnt = runs(wkeys)
    cands = (np.arange(1, 4096, dtype=np.uint64) * np.uint64(2654435761)).astype(np.uint32) & np.uint32(mask)
    absent = int(cands[(cands != 0) & ~np.isin(cands, dk)][0])
    q = np.concatenate([dk, np.array([0, absent], np.uint32)])
    off, hp = ix.find(q)
    assert (np.diff(off.astype(np.int64)) == np.concatenate([cnt, [0, 0]])).all() and (hp == wpos).all()
    one = ctx.index_build(T, 5, mask)
    assert one.seqs == 1


# ----------------------------------------------------------------------------- 2. one contig: the new path is the old one
def test_one_contig_equals_locate(ctx):
    mask = eng.mask_from_pattern(MASK_PAT)
    g = eng.synth_genome(911, 40000)
    text, offs, _ = eng.synth_reads(912, g, 300, 2000, 0.04, 0.04, 0.04)
    rng = np.random.default_rng(913)
    reads = [text[int(offs[i]):int(offs[i + 1])].tobytes()[:int(rng.integers(600, 2001))] for i in range(300)]
    T = ctx.seqs_from_text(g, np.array([0, g.size], np.uint64), strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    want, wst = ctx.locate(ctx.index_build(T, 0, mask), T, 0, Rd, R, 50, 500)
    ix = ctx.index_build_set(T, mask)
    assert ix.seqs == 1
    got, gst = ctx.map_reads(ix, T, Rd, R, 50, 500, strands=1)
    assert want["found"].sum() > 200
    for c in want.dtype.names:
        assert (got[c] == want[c]).all(), c
    assert (got["contig"] == np.where(want["found"] == 1, 0, -1)).all() and (got["strand"] == want["found"]).all()
    assert gst["strand"][0] == wst and gst["n_second_walk"] == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_contig_both_strands(ctx, oracle, kernel):
    """Half the reads reverse-complemented: the rows are Oracle.locator's on the reads and on their reverse complements,
    merged -- the + row if found, else the - row, n_pairs summed."""
    mask = eng.mask_from_pattern(MASK_PAT)
    g = eng.synth_genome(921, 40000)
    text, offs, _ = eng.synth_reads(922, g, 200, 1500, 0.04, 0.04, 0.04)
    rng = np.random.default_rng(923)
    reads = [text[int(offs[i]):int(offs[i + 1])].tobytes()[:int(rng.integers(450, 1501))] for i in range(200)]
    reads = [rc(x) if f else x for x, f in zip(reads, rng.integers(0, 2, 200))]
    plus, pst = oracle.locator(g, mask, R, *eng.concat(reads), 50, 500, nthreads=8)
    minus, _ = oracle.locator(g, mask, R, *eng.concat([rc(x) for x in reads]), 50, 500, nthreads=8)
    want = merge_strands(plus, minus, [len(x) for x in reads])
    assert (want["strand"] == 1).sum() > 50 and (want["strand"] == -1).sum() > 50 and (want["nseq"] < 0).any()
    T = ctx.seqs_from_text(g, np.array([0, g.size], np.uint64), strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    got, gst = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, R, 50, 500, kernel=kernel, strands=3)
    same_rows(got, want)
    assert gst["strand"][0] == pst
    walked = (plus["found"] == 0) & (plus["nseq"] >= 0)
    assert gst["n_second_walk"] == walked.sum() and gst["strand"][1]["n_pairs"] == minus["n_pairs"][walked].sum()
    assert gst["strand"][1]["n_located"] == minus["found"][walked].sum()


# ----------------------------------------------------------------------------- 3. many contigs, both strands
@pytest.fixture(scope="module")
def many(oracle):
    contigs, reads, flipped = many_contig_case(801)
    mask = eng.mask_from_pattern(MASK_PAT)
    rows, stats, walks = map_reads_ref(oracle, contigs, reads, mask, R, 50, 500, strands=3)
    return contigs, reads, mask, rows, stats


def test_many_contig_case_holds_what_it_is_for(many):
    """From the restatement alone: a found read on every non-degenerate contig, both strands, failures that cost pairs, a
    row at position 0, an alignment that reaches a contig's last base, a read remainder longer than the contig's."""
    contigs, reads, _, rows, _ = many
    f = rows[rows["found"] == 1]
    assert len(contigs) == 8 and len(reads) == 400
    assert sorted(set(f["contig"].tolist())) == [c for c, n in enumerate(MANY_LENS) if n >= 600]
    assert (f["strand"] == 1).sum() > 100 and (f["strand"] == -1).sum() > 100
    assert ((rows["found"] == 0) & (rows["n_pairs"] > 0)).sum() >= 10
    assert ((rows["found"] == 0) & (rows["nseq"] >= 0)).sum() >= 20 and (rows["nseq"] < 0).sum() == 10
    assert (f["pos"] == 0).any()
    assert any(int(r["c_end"]) == len(contigs[int(r["contig"])]) for r in f)
    assert any(len(reads[int(r["read"])]) - int(r["j"]) > len(contigs[int(r["contig"])]) - int(r["pos"]) for r in f)


@pytest.fixture(scope="module")
def many_on_device(ctx, many):
    contigs, reads, mask, _, _ = many
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    return T, Rd, ctx.index_build_set(T, mask)


@pytest.mark.parametrize("kernel", KERNELS)
def test_many_contigs_both_strands(ctx, many, many_on_device, kernel):
    _, _, _, want, wst = many
    T, Rd, ix = many_on_device
    status, got, st = raw_map_reads(ctx, ix, T, Rd, R, 50, 500, kernel, 3)
    assert status == 0, ctx.lib.pba_ctx_error(ctx.h)
    same_rows(got, want)
    for k in range(2):
        for c in STAT_COLS + ("n_reads_kept",):
            assert getattr(st.strand[k], c) == wst[k][c], (k, c)
    assert st.n_second_walk == wst[1]["n_reads_kept"]


# ----------------------------------------------------------------------------- 4. hit groups across contigs
@pytest.mark.parametrize("kernel", KERNELS)
def test_hit_groups_across_contigs(ctx, oracle, kernel):
    """A 300-base segment planted 100 times over 5 contigs: a probe inside it has 100 hits, two groups of the kernel's walk,
    spanning contigs.  n_pairs is where a wrong count of the failed hits of a group shows."""
    contigs, reads, _ = repeat_case(811)
    mask = eng.mask_from_pattern(MASK_PAT)
    want, wst, walks = map_reads_ref(oracle, contigs, reads, mask, R, 50, 500, strands=1)
    w = [x[1] for x in walks]
    assert len(reads) == 50 and want["found"].sum() >= 45
    assert any(x["found"] and x["rank"] >= 64 for x in w)
    assert any(x["found"] and x["contig"] != x["first_contig"] for x in w)
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    got, gst = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, R, 50, 500, kernel=kernel, strands=1)
    same_rows(got, want)
    same_stats(gst, wst)


# ----------------------------------------------------------------------------- 5. the reference-band re-run
def test_reference_band_rerun(ctx, oracle):
    """16 reads of 15 kb on two 30 kb contigs, of each contig four at 15 % error and four at 21 %: some reads go to the second,
    reference-band launch, and the rows are Oracle.locator's per contig, merged (a read is found on one contig only).
    Which reads must go there is known from the oracle alone: at 15 kb the first launch holds two blocks per lane, its window
    is as wide as that ring lets it be, (2 * 2016 + 64 - 4) * 2 / 3 = 2 728 columns (bv_pass1_w), and a goal above the window
    cannot be certified inside it.  A success at 15 % costs ~2 150, inside the window; one at 21 % costs ~2 900 and must be
    re-run.  A read without a single pair has nothing to re-run.
    n_pairs: the kernel tries j first, then contig, so a found read leaves out the other contig's hits behind its j --
    between its own contig's count and the sum."""
    mask = eng.mask_from_pattern(MASK_PAT)
    g = eng.synth_genome(931, 60000)
    contigs = [g[:30000].tobytes(), g[30000:].tobytes()]
    reads = []
    for c in range(2):
        for first, p in ((0, 0.05), (4, 0.07)):
            text, offs, _ = eng.synth_reads(932 + c, g[30000 * c:30000 * (c + 1)], 8, 15000, p, p, p)
            reads += [text[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(first, first + 4)]
    rtext, roffs = eng.concat(reads)
    per = [oracle.locator(np.frombuffer(t, np.uint8), mask, R, rtext, roffs, 50, 500, nthreads=8)[0] for t in contigs]
    assert ((per[0]["found"] + per[1]["found"]) <= 1).all() and per[0]["found"].sum() >= 3 and per[1]["found"].sum() >= 3
    window = (2 * 2016 + 64 - 4) * 2 // 3
    cost = np.maximum(per[0]["cost"], per[1]["cost"])                   # (-1 where not found)
    must_redo = int((cost > window).sum())
    can_redo = int(((per[0]["n_pairs"] + per[1]["n_pairs"]) > 0).sum())
    assert must_redo >= 3 and ((cost > 0) & (cost <= window)).sum() >= 3 and can_redo < 16
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    got, _ = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, R, 50, 500, strands=1)
    prof = ctx.last_profile()
    print("reads re-run at the reference band:", prof["n_redo"], "of", prof["n_first"], "; the oracle's costs say at least",
          must_redo, "and at most", can_redo)
    assert prof["n_first"] == 16 and prof["nb_first"] == 2 and prof["nb_redo"] > 2
    assert prof["n_redo"] > 0 and must_redo <= prof["n_redo"] <= can_redo
    for r in range(16):
        c = 0 if per[0][r]["found"] else (1 if per[1][r]["found"] else -1)
        assert int(got[r]["contig"]) == c and int(got[r]["strand"]) == (1 if c >= 0 else 0)
        for k in ("found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b"):
            assert int(got[r][k]) == int(per[max(c, 0)][r][k]), (r, k)
        both = int(per[0][r]["n_pairs"]) + int(per[1][r]["n_pairs"])
        assert (int(per[c][r]["n_pairs"]) if c >= 0 else both) <= int(got[r]["n_pairs"]) <= both, r


# ----------------------------------------------------------------------------- 6. strands, reads_rc, refusals
def test_strands_and_reads_rc(ctx, many, many_on_device):
    contigs, reads, mask, want, _ = many
    T, Rd, ix = many_on_device
    Rc = ctx.seqs_revcomp(Rd)
    lens = np.array([len(x) for x in reads])
    # strands = 2 is strands = 1 on the reverse complements, intervals flipped
    minus, mst = ctx.map_reads(ix, T, Rd, R, 50, 500, strands=2, reads_rc=Rc)
    plus_of_rc, pst = ctx.map_reads(ix, T, Rc, R, 50, 500, strands=1)
    for c in ("read", "nseq", "found", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "diag_cost", "n_pairs",
              "c_beg", "c_end"):
        assert (minus[c] == plus_of_rc[c]).all(), c
    assert (minus["strand"] == -plus_of_rc["strand"]).all() and (minus["found"] == 1).sum() > 100
    f = minus["found"] == 1
    assert (minus["r_beg"][f] == lens[f] - plus_of_rc["r_end"][f]).all() and (minus["r_end"][f] == lens[f] - plus_of_rc["r_beg"][f]).all()
    assert mst["strand"][1] == pst["strand"][0] and mst["strand"][0]["n_pairs"] == 0 and mst["n_second_walk"] == 0
    # strands = 3: reads_rc given or built inside
    a, ast = ctx.map_reads(ix, T, Rd, R, 50, 500, strands=3, reads_rc=Rc)
    b, bst = ctx.map_reads(ix, T, Rd, R, 50, 500, strands=3)
    assert (a == b).all() and ast == bst
    same_rows(a, want)
    # refusals
    def status_of(call):
        with pytest.raises(PbaError) as e:
            call()
        return e.value.status
    other_lens = ctx.seqs_from_list([x[:-1] for x in reads], strict_acgt=True)
    assert status_of(lambda: ctx.map_reads(ix, T, Rd, R, 50, 500, strands=3, reads_rc=other_lens)) == _lib.PBA_E_INVALID
    fewer = ctx.seqs_from_list(reads[:-1], strict_acgt=True)
    assert status_of(lambda: ctx.map_reads(ix, T, Rd, R, 50, 500, strands=3, reads_rc=fewer)) == _lib.PBA_E_INVALID
    T2 = ctx.seqs_from_list(contigs[:-1], strict_acgt=True)
    assert status_of(lambda: ctx.map_reads(ctx.index_build_set(T2, mask), T, Rd, R, 50, 500)) == _lib.PBA_E_INVALID
    T4 = ctx.seqs_from_list([contigs[0] + contigs[2], b"", b""] + contigs[3:], strict_acgt=True)   # same count and total, other lengths
    assert status_of(lambda: ctx.map_reads(ctx.index_build_set(T4, mask), T, Rd, R, 50, 500)) == _lib.PBA_E_INVALID
    assert status_of(lambda: ctx.map_reads(ctx.index_build(T, 0, mask), T, Rd, R, 50, 500)) == _lib.PBA_E_INVALID
    for bad in (0, 4):
        assert status_of(lambda: ctx.map_reads(ix, T, Rd, R, 50, 500, strands=bad)) == _lib.PBA_E_INVALID
    # bytes outside ACGT: legal for the index, refused by the locate
    Tn = ctx.seqs_from_list([contigs[0][:500] + b"N" + contigs[0][501:2000], contigs[2]], strict_acgt=False)
    ixn = ctx.index_build_set(Tn, mask)
    assert Tn.non_acgt and ixn.seqs == 2 and ixn.visited == 5000
    assert status_of(lambda: ctx.map_reads(ixn, Tn, Rd, R, 50, 500)) == _lib.PBA_E_ALPHABET
    Rn = ctx.seqs_from_list([reads[0][:100] + b"n" + reads[0][101:]], strict_acgt=False)
    assert status_of(lambda: ctx.map_reads(ix, T, Rn, R, 50, 500)) == _lib.PBA_E_ALPHABET
    # an empty read set
    empty = ctx.seqs_from_list([], strict_acgt=True)
    status, rows, st = raw_map_reads(ctx, ix, T, empty, R, 50, 500, 0, 3)
    assert status == 0 and len(rows) == 0 and st.n_second_walk == 0 and st.strand[0].n_pairs == 0


def test_total_length_limit(ctx):
    """0x7FFFFFF0 bases in all are refused, from the lengths on the host, before anything is allocated for the index.  The set
    is 512 views of one 1 MiB packed buffer (pba_seqs_from_device_packed: offsets may repeat), so nothing of that size is
    packed or uploaded; the set's own bit planes are what it costs."""
    import torch
    n, per = 512, 4 * (1 << 20)
    assert n * per == 1 << 31
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lens = np.full(n, per, np.uint32)
    lens[-1] = per - 16                                                   # total 0x7FFFFFF0: at the limit
    S = ctx.seqs_from_device_packed(buf.data_ptr(), buf.numel(), np.zeros(n, np.uint64), lens)
    with pytest.raises(PbaError) as e:
        ctx.index_build_set(S, 0xFFFFFFFF)
    assert e.value.status == _lib.PBA_E_TOOLONG
    S.close()


# ----------------------------------------------------------------------------- 7. the Python surface
def test_python_surface(ctx, many, many_on_device):
    T, Rd, ix = many_on_device
    status, raw, st = raw_map_reads(ctx, ix, T, Rd, R, 50, 500, 0, 3)
    assert status == 0
    rows, stats = ctx.map_reads(ix, T, Rd, R, 50, 500)
    assert rows.dtype == MAP_ROW_DTYPE and (rows == raw).all()
    assert stats["n_second_walk"] == st.n_second_walk
    for k in range(2):
        assert stats["strand"][k] == {n: getattr(st.strand[k], n) for n, _ in _lib.PbaLocStats._fields_}
    for r in rows[rows["found"] == 1][:50]:
        assert (int(r["r_beg"]), int(r["r_end"]), int(r["c_beg"]), int(r["c_end"])) == \
            intervals(int(r["strand"]), 1, int(r["j"]), int(r["pos"]), int(r["matlen_a"]), int(r["matlen_b"]), int(Rd.lengths()[int(r["read"])]))
