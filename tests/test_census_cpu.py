"""tests/census_ref.py judged without a GPU: the census pinned by hand on a 40-base text in both modes, the cutoff on hand-made
histograms (pba_census_cutoff is host arithmetic and is held to the same answers through the library), the refusals that need
no device, and -- with the oracle -- the conditions of the planted read set, so that tests/test_gpu_census.py cannot pass
vacuously: masking takes probes out on both strands and leaves every read some, the rows change, fewer seeds match, a first
success moves, and what is lost is lost where a read's end lies inside a planted copy."""
import ctypes as C

import numpy as np
import pytest

import census_ref as cr
import index_ref as ir
import overlap_ref as orf
from pacbioassembly_amd import _lib

# ----------------------------------------------------------------------------- the census by hand
TEXT40 = b"ACGTACGTACGTACGTTTTTTTTTTTTTTTTTAAAAAAAA"      # 16 of period 4, 16 T, 8 A
M_FIRST = orf.mask_of("1" + "*" * 15)                     # the window's first base alone: key = code << 6


def test_hand_census_both_modes():
    assert len(TEXT40) == 40
    # mode "all": every position 0 .. 39; the key is the base's code at bits 7:6; A (code 0) is a zero key
    codes = [0, 1, 2, 3] * 4 + [3] * 16 + [0] * 8
    all_ = cr.census([TEXT40], M_FIRST, "all")
    assert all_["count"] == {1 << 6: 4, 2 << 6: 4, 3 << 6: 20} and all_["n_visited"] == 40
    assert (all_["n_counted"], all_["n_zero_keys"]) == (28, 12) and codes.count(0) == 12
    # mode "head_tail": the head 0 .. len - 17 = 0 .. 23, no tail below 20 017 bases
    assert cr.visited(40, "head_tail").tolist() == list(range(24))
    ht = cr.census([TEXT40], M_FIRST, "head_tail")
    assert ht["count"] == {1 << 6: 4, 2 << 6: 4, 3 << 6: 12} and (ht["n_visited"], ht["n_counted"], ht["n_zero_keys"]) == (24, 20, 4)
    # the last base of the window alone: mode "all" pads the windows past the end with code 3
    m_last = orf.mask_of("*" * 15 + "1")
    last = cr.census([TEXT40], m_last, "all")
    # window p ends at base p + 15: p = 0 -> T(15); 1 .. 16 -> T; 17 .. 24 -> A (bases 32 .. 39); 25 .. 39 -> padding (3)
    assert last["count"] == {3 << 24: 17 + 15} and last["n_zero_keys"] == 8
    # two texts add up; a text shorter than a window visits nothing in head_tail and every position in "all"
    both = cr.census([TEXT40, b"ACG"], M_FIRST, "head_tail")
    assert both["count"] == ht["count"] and both["n_visited"] == 24 and both["n_seqs"] == 2
    assert cr.census([b"ACG"], M_FIRST, "all")["count"] == {1 << 6: 1, 2 << 6: 1}
    assert cr.merged(ht, all_)["count"] == {1 << 6: 8, 2 << 6: 8, 3 << 6: 32}
    assert cr.lookup(all_, [3 << 6, (3 << 6) | 5, 0, 5], M_FIRST).tolist() == [20, 20, 0, 0]


def test_visited_is_the_index_rule_at_its_edges():
    for n, want in ((0, 0), (15, 0), (16, 0), (17, 1), (20016, 20000), (20017, 20001), (40016, 40000), (40100, 40000)):
        assert cr.visited(n, "head_tail").size == want, n
        assert cr.visited(n, "all").size == n
    v = cr.visited(40100, "head_tail")
    assert v[:3].tolist() == [0, 1, 2] and v[20000:20003].tolist() == [40084, 40083, 40082] and np.unique(v).size == v.size


def test_hand_histogram_and_repeats():
    cen = dict(count={5: 1, 6: 1, 7: 3, 9: 70000}, n_visited=70005, n_counted=70005, n_zero_keys=0, n_seqs=1)
    h, nd, mx = cr.histogram(cen, 0xF, 5)
    assert h.tolist() == [12, 2, 0, 1, 1] and (nd, mx) == (4, 70000)
    h, _, _ = cr.histogram(cen, 0xF, 2)
    assert h.tolist() == [12, 4]
    ht = cr.census([TEXT40], M_FIRST, "head_tail")
    over, vis = cr.read_repeats(ht, [TEXT40, b"TTTTTTTTTTTTTTTTTT", b""], M_FIRST, "head_tail", 4)
    assert over.tolist() == [12, 2, 0] and vis.tolist() == [24, 2, 0]      # only T (count 12) is above 4
    over, _ = cr.read_repeats(ht, [TEXT40], M_FIRST, "head_tail", cr.U32_MAX)
    assert over.tolist() == [0]
    e = np.array([(3 << 6) << 32 | 7, (1 << 6) << 32 | 9, 0xFFFFFFFFFFFFFFFF, (3 << 6) << 32 | 1], np.uint64)
    kept, n = cr.masked_entries(e, ht, 4)
    assert kept.tolist() == [(1 << 6) << 32 | 9] and n == 2
    assert cr.masked_entries(e, ht, 12)[1] == 0


# ----------------------------------------------------------------------------- the cutoff
#           (hist, fraction, floor, answer; None = PBA_E_TOOLONG)
CUTOFFS = [([0, 10, 5, 3, 2], 0.0, 1, None),       # 20 keys, budget 0: 2 keys sit in the lumped slot, nobody can say how high
           ([0, 10, 5, 3, 0], 0.0, 1, 3),          # ... and with it empty: nothing above 3
           ([0, 10, 5, 3, 2], 0.1, 1, 3),          # budget 2: above(3) = 2
           ([0, 10, 5, 3, 2], 0.25, 1, 2),         # budget 5: above(2) = 5
           ([0, 10, 5, 3, 2], 0.2499, 1, 3),       # budget int(4.998) = 4: the product is truncated, not rounded
           ([0, 10, 5, 3, 2], 1.0, 1, 1),
           ([0, 10, 5, 3, 2], 1.0, 3, 3),          # the floor
           ([0, 10, 5, 3, 2], 1.0, 4, None),       # a floor beyond cap - 2
           ([0, 10, 5, 3, 2], 1.0, 0, 1),          # floor 0 is floor 1
           ([7, 0, 0, 0], 0.5, 1, 1),              # no key at all
           ([0, 3], 1.0, 1, None),                 # cap 2: no c in [1, 0]
           ([0, 0, 0, 1000, 0, 0, 0, 0, 0, 1], 0.001, 1, 3)]   # budget 1: the one key at >= 9 may stay above


@pytest.mark.parametrize("hist, fraction, floor, want", CUTOFFS)
def test_cutoff_by_hand(lib, hist, fraction, floor, want):
    assert cr.cutoff(hist, fraction, floor) == want
    h = np.array(hist, np.uint64)
    out = C.c_uint32(12345)
    st = lib.pba_census_cutoff(h.ctypes.data, h.size, fraction, floor, C.byref(out))
    assert (st, out.value) == ((_lib.PBA_OK, want) if want is not None else (_lib.PBA_E_TOOLONG, 12345))


def test_host_refusals(lib):
    """what is decided without a device: the cutoff's arguments and the NULLs of every entry point"""
    h = np.array([0, 1, 1], np.uint64)
    out = C.c_uint32()
    for frac in (-0.01, 1.01, float("nan"), float("inf")):
        assert lib.pba_census_cutoff(h.ctypes.data, 3, frac, 1, C.byref(out)) == _lib.PBA_E_INVALID
    assert lib.pba_census_cutoff(h.ctypes.data, 1, 0.5, 1, C.byref(out)) == _lib.PBA_E_INVALID
    assert lib.pba_census_cutoff(None, 3, 0.5, 1, C.byref(out)) == _lib.PBA_E_INVALID
    assert lib.pba_census_cutoff(h.ctypes.data, 3, 0.5, 1, None) == _lib.PBA_E_INVALID
    p = C.c_void_p()
    n = C.c_uint64()
    assert lib.pba_census_create(None, None, 0, 0, 0xFF, 1, C.byref(p)) == _lib.PBA_E_INVALID and not p.value
    assert lib.pba_census_add(None, None, None, 0, 0) == _lib.PBA_E_INVALID
    assert lib.pba_census_lookup(None, None, None, 0, None) == _lib.PBA_E_INVALID
    assert lib.pba_census_histogram(None, None, h.ctypes.data, 3, None, None) == _lib.PBA_E_INVALID
    assert lib.pba_census_read_repeats(None, None, None, 0, None, None, 0) == _lib.PBA_E_INVALID
    assert lib.pba_census_mask_probes(None, None, None, 0, 0xFF, 0, C.byref(n)) == _lib.PBA_E_INVALID
    assert lib.pba_overlap_strands_masked(None, None, None, 0, 0, 0xFF, 0.2, 8, 64, 0, 3, None, 0, None, 0, C.byref(n), None, None) == _lib.PBA_E_INVALID
    assert lib.pba_census_last_stats(None, None) == _lib.PBA_E_INVALID
    lib.pba_census_destroy(None)


def test_inputs_are_what_they_claim():
    L = cr.edge_lengths()
    assert len(L) == 23 and {0, 16, 1025, 4097, 16399, 20017, 40016, 40100} <= set(L)
    for shape in cr.SHAPES:
        assert [len(t) for t in cr.edge_texts(shape)] == L
    m = cr.MASKS["w12"]
    assert set(cr.census(cr.edge_texts("all_t"), m, "head_tail")["count"]) == {m}                  # all T: the key is the mask itself
    assert cr.census(cr.edge_texts("all_a"), m, "head_tail")["count"] == {}                        # all A: only zero keys ...
    assert cr.census(cr.edge_texts("all_a"), m, "all")["n_counted"] == 15 * sum(n >= 15 for n in L) + sum(n for n in L if n < 15)  # ... but for the padded windows
    assert len(cr.census(cr.edge_texts("period2"), m, "all")["count"]) > 2 > 0
    assert len(cr.census(cr.edge_texts("period7"), m, "head_tail")["count"]) == 7
    assert cr.MASKS["w12"] == orf.mask_of("111*11*11*1*1111")


# ----------------------------------------------------------------------------- the planted set's conditions
@pytest.fixture(scope="module")
def planted(oracle):
    comps, cen = cr.planted_compositions(oracle)
    return comps, cen


def test_planted_set_shape_and_cutoff():
    texts, meta = cr.planted_reads()
    assert len(texts) == 40 and all(430 <= len(t) <= 1300 for t in texts) and sum(1 for m in meta if m[2] < 0) == 20
    inside = lambda p: any(s <= p < e for s, e in cr.repeat_intervals())
    assert sum(inside(s) for s, _, _ in meta) >= 4 and sum(inside(e - 1) for _, e, _ in meta) >= 4      # reads that start / end inside a copy
    cen = cr.census(texts, cr.MASKS["w12"], "head_tail")
    hist, nd, mx = cr.histogram(cen, cr.MASKS["w12"], 200)
    assert mx >= 25 and nd > 20000
    assert cr.cutoff(hist, 0.01) == cr.PLANTED["max_occ"] == 3          # the cutoff the tests mask at: one key in a hundred given up
    assert cr.cutoff(hist, 0.0) == mx and cr.cutoff(hist, 1.0) == 1


def test_planted_set_conditions(planted):
    comps, cen = planted
    texts, meta = cr.planted_reads()
    P, mask = cr.PLANTED, cr.MASKS["w12"]
    for s, qtexts in ((1, texts), (-1, [orf.comp(t) for t in texts])):
        u, m = comps[s]
        # at least one probe entry is masked on each strand, at least one is kept for every read
        assert m["n_masked"] >= 5 and u["n_masked"] == 0 and m["n_probe_entries"] + m["n_masked"] == u["n_probe_entries"]
        kept = [0] * len(texts)
        for key, v in orf.ProbeTable(qtexts, mask, P["max_trial"]).by_key.items():
            if cen["count"].get(key, 0) <= P["max_occ"]:
                for q, _ in v:
                    kept[q] += 1
        assert min(kept) >= 1 and sum(kept) == m["n_probe_entries"]
        assert m["n_match"] < u["n_match"] and m["pairs"] < u["pairs"]          # fewer seeds match, fewer pairs are aligned
        assert len(m["rows"]) < len(u["rows"]) and set(m["rows"]) != set(u["rows"]) and len(m["rows"]) >= 20
    U, M = cr.strand_rows(comps, 0), cr.strand_rows(comps, 1)
    du, dm = {r[:3]: r for r in U}, {r[:3]: r for r in M}
    assert len(du) == len(U) and len(dm) == len(M) and set(dm) <= set(du)        # masking adds no (target, query, strand)
    # a first success moved: the pair keeps a row, found from a later probe
    moved = [k for k in dm if dm[k][3] != du[k][3]]
    assert len(moved) >= 2 and all(dm[k][3] > du[k][3] or dm[k][4] != du[k][4] for k in moved)
    # a row whose own probe was not masked is the masked call's row too: the candidates tried before it are a subset of those
    # that failed before it
    probe_key = lambda r: int(ir.np_keys(texts[r[1]] if r[2] > 0 else orf.comp(texts[r[1]]))[r[3] if r[4] > 0 else len(texts[r[1]]) - r[3] - 16]) & mask
    for k, r in du.items():
        if cen["count"].get(probe_key(r), 0) <= P["max_occ"]:
            assert dm.get(k) == r, r
    # the rows between two reads that share 200 bases or more of unique genome: all still there, but for queries with an end
    # inside a planted copy -- the probes of that end are the repeat's, which is what the cutoff gives up
    inside = lambda p: any(s <= p < e for s, e in cr.repeat_intervals())
    solid = [k for k in du if cr.unique_overlap(meta[k[0]], meta[k[1]]) >= 200]
    lost = [k for k in solid if k not in dm]
    assert len(solid) >= 40 and len(solid) - len(lost) >= 35
    for t, q, s in lost:
        assert inside(meta[q][0]) or inside(meta[q][1] - 1), (t, q, s)
    # and what the masking is for: fewer rows between reads that share no unique base
    false_u = sum(1 for k in du if cr.unique_overlap(meta[k[0]], meta[k[1]]) <= 0)
    false_m = sum(1 for k in dm if cr.unique_overlap(meta[k[0]], meta[k[1]]) <= 0)
    assert false_m < false_u


def test_planted_set_without_a_cutoff_and_with_cutoff_zero(oracle, planted):
    """max_occ = UINT32_MAX is walk_composition itself; max_occ = 0 leaves only probes whose key no read's index visits -- the
    backward probe at j = 0 of a read below 20 017 bases looks at position len - 16, which get_seedmap does not visit, and the
    probes of rc(q) need a read of the other orientation over the same bases -- and those match nothing"""
    comps, cen = planted
    texts, _ = cr.planted_reads()
    P, mask = cr.PLANTED, cr.MASKS["w12"]
    W = orf.walk_composition(oracle, texts, None, P["R"], mask, P["max_trial"], P["overlap_min"])
    u = comps[1][0]
    assert (u["rows"], u["n_match"], u["pairs"], u["pairs_by"], u["n_probe_entries"]) == (W["rows"], W["n_match"], W["pairs"], W["pairs_by"], W["n_probe_entries"])
    zero, _ = cr.planted_compositions(oracle, 0)
    for s in (1, -1):
        z = zero[s][1]
        assert z["rows"] == [] and z["n_match"] == 0 and z["pairs"] == 0 and 0 < z["n_probe_entries"] < comps[s][0]["n_probe_entries"]
    t2 = 2 * P["max_trial"]
    left = cr.masked_entries(orf.probe_entries(texts, mask, P["max_trial"]), cen, 0)[0]
    assert left.size == zero[1][1]["n_probe_entries"] and all(int(e) % t2 == 1 for e in left)      # forward strand: only jd = 1
