"""The seed-key census on the device (pba_census_*, pba_overlap_strands_masked): every counter, total, histogram
slot, cutoff, per-read profile, masked probe entry and overlap row must be IDENTICAL to tests/census_ref.py, the rule restated
in plain numpy (tests/test_census_cpu.py pins that reference by hand and proves the planted set's conditions).  Needs a real
MI355X (-m gpu)."""
import functools

import numpy as np
import pytest

import census_ref as cr
import overlap_ref as orf
from pacbioassembly_amd import _lib
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP, PbaError

pytestmark = pytest.mark.gpu
U32_MAX = cr.U32_MAX
ROW9 = ("target", "query", "strand", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b")


@functools.lru_cache(maxsize=None)
def ref_census(shape, mask_name, mode):
    return cr.census(cr.edge_texts(shape), cr.MASKS[mask_name], mode)


@functools.lru_cache(maxsize=None)
def edge_set(ctx, shape):
    return ctx.seqs_from_list(cr.edge_texts(shape))


def refused(status, fn, *a, **kw):
    with pytest.raises(PbaError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value


def check_census(cen, want, mask, seed=3):
    """the whole table: every key the reference holds, 1 000 keys it does not, the totals, n_distinct and max_count"""
    st = cen.stats
    print({k: st[k] for k in ("n_seqs", "bits", "n_visited", "n_counted", "n_zero_keys")})
    assert (st["n_seqs"], st["bits"]) == (want["n_seqs"], cr.bits_of(mask))
    assert (st["n_visited"], st["n_counted"], st["n_zero_keys"]) == (want["n_visited"], want["n_counted"], want["n_zero_keys"])
    keys = np.array(sorted(want["count"]), np.uint32)
    assert cen.lookup(keys).tolist() == [want["count"][int(k)] for k in keys]
    rng = np.random.default_rng(seed)
    absent = np.array([k for k in (rng.integers(0, 1 << 32, 1400, dtype=np.uint64) & np.uint64(mask)).tolist() if k not in want["count"]][:998]
                      + [0, ~mask & 0xFFFFFFFF], np.uint32)
    assert absent.size >= 2 and not cen.lookup(absent).any()
    if keys.size:                                             # keys are masked inside: bits outside the mask do not matter
        assert cen.lookup(keys[:64] | np.uint32(~mask & 0xFFFFFFFF)).tolist() == [want["count"][int(k)] for k in keys[:64]]
    _, nd, mx = cen.histogram(2)
    assert (nd, mx) == (len(want["count"]), max(want["count"].values(), default=0))


@pytest.mark.parametrize("mode", ("head_tail", "all"))
@pytest.mark.parametrize("mask_name", sorted(cr.MASKS))
@pytest.mark.parametrize("shape", cr.SHAPES)
def test_census_edges(ctx, shape, mask_name, mode):
    """23 lengths on the chunk, wavefront, tile and head / tail / middle edges, five contents, masks of 2, 4, 24 and 26 bits"""
    mask = cr.MASKS[mask_name]
    cen = ctx.census(edge_set(ctx, shape), mask, mode)
    check_census(cen, ref_census(shape, mask_name, mode), mask)
    cen.close()


RULE_EDGES = (16, 17, 33, 20016, 20017, 40016, 40017, 40100)      # no position; one; the head alone up to its last length; the first
                                                                  # tail position; head and tail whole; the first lengths with a gap


def test_census_and_index_visit_the_same_positions_at_the_rule_edges(ctx):
    """The two device consumers of the visiting rule (csrc/index_plan.h) held to each other through the library, one random
    sequence per edge length of the rule: the head_tail census of a sequence alone has visited what the head_tail index of that
    sequence reports, has counted the index's entries, and holds for a key of the index the length of the run find returns."""
    import index_ref as ir
    mask = cr.MASKS["w12"]
    rng = np.random.default_rng(20016)
    texts = [cr.ACGT[rng.integers(0, 4, n)].tobytes() for n in RULE_EDGES]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    for i, (n, text) in enumerate(zip(RULE_EDGES, texts)):
        ref_keys, _, _ = ir.np_index(text, mask, "head_tail")
        n_visited = ir.visit_order(n, "head_tail")[0].size
        assert ref_keys.size == n_visited and (n_visited > 0) == (n > 16), n      # no zero key in this text: counted == visited is no accident
        cen = ctx.census(S, mask, "head_tail", i, i + 1)
        ix = ctx.index_build(S, i, mask, eng.PBA_INDEX_HEAD_TAIL)
        visited = ix.visited if ix.visited < 1 << 31 else 0                       # (below 16 bases the index reports a negative count as it is)
        st = cen.stats
        print(n, {k: st[k] for k in ("n_visited", "n_counted", "n_zero_keys")}, ix.visited, ix.entries)
        assert st["n_visited"] == visited == n_visited, n
        assert st["n_counted"] == ix.entries == ref_keys.size, n
        keys, _ = ix.dump()
        if keys.size:
            sel = rng.choice(keys, 64)
            off, _ = ix.find(sel)
            runs = np.diff(off.astype(np.int64))
            assert runs.min() >= 1 and cen.lookup(sel).tolist() == runs.tolist(), n
        ix.close()
        cen.close()


def test_add_ranges_and_sets(ctx):
    """create(0, k) + add(k, n) is create(0, n); two different sets added are the sum of their censuses"""
    S, mask = edge_set(ctx, "random"), cr.MASKS["w12"]
    n = S.count
    for mode in ("head_tail", "all"):
        want = ref_census("random", "w12", mode)
        for k in (0, 1, 15, n):
            cen = ctx.census(S, mask, mode, 0, k).add(S, k, n)
            check_census(cen, want, mask)
            cen.close()
        cen = ctx.census(S, mask, mode, 14, 15).add(S, 0, 14).add(S, 15, n).add(S, 3, 3)
        check_census(cen, want, mask)
        cen.add(edge_set(ctx, "period7"))
        check_census(cen, cr.merged(want, ref_census("period7", "w12", mode)), mask)
        cen.close()


def test_contention(ctx):
    """300 reads of 1 000 T: one key, every add to one counter"""
    texts = [b"T" * 1000] * 300
    S = ctx.seqs_from_list(texts)
    for name in ("w1", "w12"):
        mask = cr.MASKS[name]
        for mode, visited in (("head_tail", 300 * 984), ("all", 300 * 1000)):
            cen = ctx.census(S, mask, mode)
            assert cen.lookup([mask]).tolist() == [visited] and cen.stats["n_counted"] == visited and cen.stats["n_zero_keys"] == 0
            assert cen.histogram(4)[1:] == (1, visited)
            cen.close()


def test_records_layout(ctx):
    """a binary read file's records are byte-aligned behind 4-byte headers: the same census as the text-built set"""
    texts = [t for t in cr.edge_texts("random") if 0 < len(t) < 20000] + cr.edge_texts("period2")[-3:]      # (a record file holds no empty read)
    S = ctx.seqs_from_records(b"".join(eng.text2bin(t) for t in texts), 0, 1 << 30)
    assert S.count == len(texts)
    for mode in ("head_tail", "all"):
        cen = ctx.census(S, cr.MASKS["w12"], mode)
        check_census(cen, cr.census(texts, cr.MASKS["w12"], mode), cr.MASKS["w12"])
        cen.close()


@pytest.mark.parametrize("shape, mask_name", [("random", "w12"), ("random", "w2"), ("period7", "w13"), ("all_t", "w1"), ("all_a", "w12")])
def test_histogram_and_cutoff(ctx, shape, mask_name):
    mask = cr.MASKS[mask_name]
    for mode in ("head_tail", "all"):
        want = ref_census(shape, mask_name, mode)
        cen = ctx.census(edge_set(ctx, shape), mask, mode)
        for cap in (2, 3, 17, 65536):
            hist, nd, mx = cen.histogram(cap)
            w, wnd, wmx = cr.histogram(want, mask, cap)
            assert (nd, mx) == (wnd, wmx) and hist.tolist() == w.tolist(), (mode, cap)
            assert int(hist[0]) == (1 << cr.bits_of(mask)) - nd and int(hist.sum()) == 1 << cr.bits_of(mask)
        for frac in (0, 0.001, 0.05, 1):
            for cap, floor in ((65536, 1), (17, 1), (65536, 5)):
                w = cr.cutoff(cr.histogram(want, mask, cap)[0], frac, floor)
                if w is None:
                    refused(_lib.PBA_E_TOOLONG, cen.cutoff, frac, floor, cap)
                else:
                    assert cen.cutoff(frac, floor, cap) == w, (mode, frac, cap, floor)
        cen.close()


def test_read_repeats(ctx):
    """on the planted set, and on the edge set with a census of ANOTHER set, at max_occ 0, the cutoff and UINT32_MAX"""
    texts, _ = cr.planted_reads()
    mask = cr.MASKS["w12"]
    S = ctx.seqs_from_list(texts)
    cen, want = ctx.census(S, mask), cr.census(texts, mask, "head_tail")
    cut = cen.cutoff(0.01, cap=200)
    assert cut == cr.PLANTED["max_occ"]
    for mo in (0, cut, 20, U32_MAX):
        over, vis = cen.read_repeats(S, mo)
        w_over, w_vis = cr.read_repeats(want, texts, mask, "head_tail", mo)
        assert over.tolist() == w_over.tolist() and vis.tolist() == w_vis.tolist(), mo
    assert cen.read_repeats(S, cut)[0].max() > 50 and not cen.read_repeats(S, U32_MAX)[0].any()
    cen.close()
    for mode, shape in (("head_tail", "period7"), ("all", "random"), ("all", "all_a"), ("head_tail", "all_t")):
        other = cr.edge_texts(shape)
        base = ref_census("random", "w2", mode)
        cen = ctx.census(edge_set(ctx, "random"), cr.MASKS["w2"], mode)
        for mo in (0, sorted(base["count"].values())[len(base["count"]) // 2], U32_MAX):
            over, vis = cen.read_repeats(edge_set(ctx, shape), mo)
            w_over, w_vis = cr.read_repeats(base, other, cr.MASKS["w2"], mode, mo)
            assert over.tolist() == w_over.tolist() and vis.tolist() == w_vis.tolist(), (mode, shape, mo)
        cen.close()


def test_mask_probes(ctx):
    """in place on the entry buffer of pba_overlap_probes, all-ones padding in it beforehand: the entries left, sorted, are the
    reference's, n_masked is exact, a second call masks nothing, another mask is refused"""
    import torch
    texts, _ = cr.planted_reads()
    P, mask = cr.PLANTED, cr.MASKS["w12"]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    cen, want = ctx.census(S, mask), cr.census(texts, mask, "head_tail")
    n, t2, GUARD = len(texts), 2 * P["max_trial"], 64
    for lo, hi in ((0, n), (7, 19), (5, 5)):
        for mo in (P["max_occ"], 0, U32_MAX):
            entries = orf.probe_entries(texts, mask, P["max_trial"], lo, hi)
            w_left, w_masked = cr.masked_entries(entries, want, mo)
            buf = torch.full(((hi - lo) * t2 + GUARD,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()                   # the fill runs on torch's stream, the emit on the engine's
            cnt = ctx.overlap_probes(S, lo, hi, mask, P["max_trial"], buf.data_ptr(), (hi - lo) * t2)
            assert cnt == entries.size
            # the whole buffer, padding behind the entries included, as an all-gathered one would be handed over
            assert cen.mask_probes(buf.data_ptr(), buf.numel(), mo) == w_masked
            host = buf.cpu().numpy().view(np.uint64)
            left = np.sort(host[host != cr.ALL_ONES])
            assert left.tolist() == w_left.tolist() and (host[cnt:] == cr.ALL_ONES).all(), (lo, hi, mo)
            assert cen.mask_probes(buf.data_ptr(), buf.numel(), mo) == 0                      # idempotent
            assert (buf.cpu().numpy().view(np.uint64) == host).all()
            if mo == P["max_occ"] and hi - lo == n:
                assert 0 < w_masked < entries.size
    refused(_lib.PBA_E_INVALID, cen.mask_probes, buf.data_ptr(), buf.numel(), 3, cr.MASKS["w13"])
    cen.close()


@functools.lru_cache(maxsize=None)
def planted_want(oracle, max_occ, t_lo=0, t_hi=None):
    texts, _ = cr.planted_reads()
    P, mask = cr.PLANTED, cr.MASKS["w12"]
    cen = cr.census(texts, mask, "head_tail")
    cache = planted_want.cache_of_verdicts
    return {s: cr.masked_composition(oracle, texts, q, P["R"], mask, P["max_trial"], P["overlap_min"], cen, max_occ, cache, t_lo, t_hi)
            for s, q in ((1, None), (-1, tuple(orf.comp(t) for t in texts)))}


planted_want.cache_of_verdicts = {}


def check_masked(got, sts, n_masked, want, strands=3):
    rows = sorted([(r[0], r[1], s) + tuple(r[2:]) for s in (1, -1) if strands & (1 if s > 0 else 2) for r in want[s]["rows"]],
                  key=lambda r: (r[0], r[1], -r[2]))
    assert [tuple(int(r[c]) for c in ROW9) for r in got] == rows
    for k, s in enumerate((1, -1)):
        if not strands & (1 << k):
            continue
        st, w = sts[k], want[s]
        print(s, {f: st[f] for f in ("n_probe_entries", "n_candidates", "n_pairs", "n_overlaps")}, n_masked[k])
        assert (st["n_probe_entries"], st["n_candidates"], st["n_pairs"], st["n_overlaps"]) == (w["n_probe_entries"], w["n_match"], w["pairs"], len(w["rows"]))
        assert n_masked[k] == w["n_masked"]


@pytest.mark.parametrize("kernel", (PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP))
def test_overlap_strands_masked(ctx, oracle, kernel):
    texts, _ = cr.planted_reads()
    P, mask = cr.PLANTED, cr.MASKS["w12"]
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    Src = ctx.seqs_revcomp(S)
    cen = ctx.census(S, mask)
    call = lambda mo, **kw: ctx.overlap_strands_masked(S, mask, P["R"], cen, mo, P["max_trial"], P["overlap_min"], kernel=kernel, **kw)
    want = planted_want(oracle, P["max_occ"])
    assert want[1]["n_masked"] > 0 and want[-1]["n_masked"] > 0 and len(want[1]["rows"]) >= 20
    got, sts, nm = call(P["max_occ"])
    check_masked(got, sts, nm, want)
    got2, sts2, nm2 = call(P["max_occ"], reads_rc=Src)                        # reads_rc given: the same
    assert got2.tobytes() == got.tobytes() and nm2 == nm
    for strands in (1, 2):
        g, s, m = call(P["max_occ"], strands=strands)
        check_masked(g, s, m, want, strands)
    g, s, m = call(P["max_occ"], t_lo=9, t_hi=23)                               # a target range: the tables are the whole set's
    check_masked(g, s, m, planted_want(oracle, P["max_occ"], 9, 23))
    # no cutoff: pba_overlap_strands row for row, every column
    plain, pst = ctx.overlap_strands(S, mask, P["R"], P["max_trial"], P["overlap_min"], kernel=kernel)
    g, s, m = call(U32_MAX)
    assert g.tobytes() == plain.tobytes() and len(g) > len(got) and m == [0, 0]
    for k in range(2):
        assert all(s[k][f] == pst[k][f] for f in ("n_probe_entries", "n_candidates", "n_pairs", "n_overlaps", "n_listed", "n_prefiltered"))
    check_masked(g, s, m, planted_want(oracle, U32_MAX))
    # cutoff 0: every probe whose key any read's index visits is out; what is left (tests/test_census_cpu.py says which) matches nothing
    g, s, m = call(0)
    check_masked(g, s, m, planted_want(oracle, 0))
    assert len(g) == 0 and all(s[k]["n_candidates"] == 0 and s[k]["n_pairs"] == 0 for k in range(2))
    Src.close()
    cen.close()


def test_refusals(ctx):
    S = edge_set(ctx, "random")
    refused(_lib.PBA_E_TOOLONG, ctx.census, S, cr.MASK_27_BITS)
    refused(_lib.PBA_E_TOOLONG, ctx.census, S, 0xFFFFFFFF, "all")
    refused(_lib.PBA_E_INVALID, ctx.census, S, 0)
    refused(_lib.PBA_E_INVALID, ctx.census, S, cr.MASKS["w12"], 2)
    refused(_lib.PBA_E_INVALID, ctx.census, S, cr.MASKS["w12"], -1)
    refused(_lib.PBA_E_INVALID, ctx.census, S, cr.MASKS["w12"], "all", 3, 2)
    refused(_lib.PBA_E_INVALID, ctx.census, S, cr.MASKS["w12"], "all", 0, S.count + 1)
    cen = ctx.census(S, cr.MASKS["w12"], "all", 0, 2)
    refused(_lib.PBA_E_INVALID, cen.add, S, 5, 4)
    refused(_lib.PBA_E_INVALID, cen.add, S, 0, S.count + 1)
    refused(_lib.PBA_E_INVALID, cen.histogram, 1)
    refused(_lib.PBA_E_INVALID, cen.histogram, 0)
    over = np.zeros(S.count, np.uint32)
    st = ctx.lib.pba_census_read_repeats(ctx.h, cen.h, S.h, 1, over.ctypes.data, over.ctypes.data, S.count - 1)
    assert st == _lib.PBA_E_INVALID                                                           # room too small
    check_census(cen, cr.census(cr.edge_texts("random")[:2], cr.MASKS["w12"], "all"), cr.MASKS["w12"])   # a refused call changed nothing
    texts, _ = cr.planted_reads()
    P = cr.PLANTED
    R = ctx.seqs_from_list(texts, strict_acgt=True)
    ok = ctx.census(R, cr.MASKS["w12"])
    for bad in (ctx.census(R, cr.MASKS["w12"], "all"), ctx.census(R, cr.MASKS["w13"])):      # an ALL-mode census; a census of another mask
        refused(_lib.PBA_E_INVALID, ctx.overlap_strands_masked, R, cr.MASKS["w12"], P["R"], bad, 3, P["max_trial"], P["overlap_min"])
        bad.close()
    refused(_lib.PBA_E_INVALID, ctx.overlap_strands_masked, R, cr.MASKS["w12"], P["R"], ok, 3, P["max_trial"], P["overlap_min"], strands=0)
    refused(_lib.PBA_E_INVALID, ctx.overlap_strands_masked, R, cr.MASKS["w12"], P["R"], ok, 3, P["max_trial"], P["overlap_min"], t_lo=5, t_hi=4)
    refused(_lib.PBA_E_INVALID, ctx.overlap_strands_masked, R, cr.MASKS["w12"], P["R"], ok, 3, 64, P["overlap_min"])
    refused(_lib.PBA_E_INVALID, ctx.overlap_strands_masked, R, cr.MASKS["w12"], P["R"], None, 3, P["max_trial"], P["overlap_min"])
    refused(_lib.PBA_E_ALPHABET, ctx.overlap_strands_masked, ctx.seqs_from_list([b"ACGTN" * 40] * 2), cr.MASKS["w12"], P["R"], ok, 3)
    ok.close()
    cen.close()


def test_repeated_calls_allocate_nothing_and_stale_buffers_do_not_matter(ctx):
    """add / lookup / histogram / read_repeats / mask_probes a second time: no kept buffer grew; and with every kept buffer
    scribbled over in between, the answers are the same"""
    import torch
    texts, _ = cr.planted_reads()
    mask, P = cr.MASKS["w12"], cr.PLANTED
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    keys = np.array(sorted(cr.census(texts, mask, "head_tail")["count"]), np.uint32)
    buf = torch.full((len(texts) * 2 * P["max_trial"],), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def once():
        cen = ctx.census(S, mask, "head_tail", 0, 10).add(S, 10, len(texts))
        ctx.overlap_probes(S, 0, len(texts), mask, P["max_trial"], buf.data_ptr(), buf.numel())
        out = (cen.stats["n_counted"], cen.lookup(keys).tolist(), cen.histogram(300)[0].tolist(), [a.tolist() for a in cen.read_repeats(S, 3)],
               cen.mask_probes(buf.data_ptr(), buf.numel(), 3), np.sort(buf.cpu().numpy()).tolist())
        cen.close()
        return out

    first = once()
    kept = ctx.kept_bytes()
    for byte in (0x00, 0xFF, 0x5A):
        ctx.scribble(byte)
        assert once() == first, byte
    assert ctx.kept_bytes() == kept
