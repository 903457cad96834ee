"""What a call finds in a buffer the context kept from an earlier call is undefined (csrc/pba_host.h: pool_reserve,
scratch_reserve, IxCache, d_queue, the pinned staging buffer; DESIGN §3.2 is the audit).  This is the list of cases
tests/test_gpu_stale_buffers.py runs in five states -- fresh, and after a DECOY call followed by Context.scribble(0x00 / 0xFF /
0x5A) or by nothing -- and tests/test_stale_cases_cpu.py judges without a GPU.

A case names the kept buffers it claims to exercise (SLOTS: _lib.POOL_SLOTS names, "scratch", "ix_ent", "ix_off", "ix_ent2",
"queue", "stage"), the existing checker that holds it to its reference (CHECKER: "module:function", imported by the CPU test),
and three callables:
  sizes()             {slot: (decoy, case)} in the quantity that sizes the slot (reads, rows, bases, bytes ...: DESIGN §3.2), from
                      the inputs alone; the decoy's must be strictly larger, so that the case runs inside the decoy's buffer
  decoy(ctx, oracle)  a different, larger call of the same entry points (or of the other entry point that shares the slot);
                      nothing of it is checked but what makes it the decoy it claims to be
  run(ctx, oracle)    the module's smallest hand case through the module's own checker: no reference is built here
References are computed once per session (_REF) and never modified.  No GPU is touched at import."""
import functools
import importlib

import numpy as np

import align_rings as ar
import cigar_ref as cr
import clip_ref
import fastx_inputs as fi
import fastx_ref as fr
import hpc_ref
import index_ref as ir
import layout_ref
import map_ref
import map_stream_inputs as msi
import overlap_edge_inputs as oi
import overlap_ref as orf
import place_ref
import rowsweep_inputs as ri
import votebox_inputs as vb
import walk_ring_inputs as wi
from conftest import MASK_PAT
from correct_helpers import mixed_reads, oracle_correct, oracle_rows
from pacbioassembly_amd import _lib
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import (MAP_ROW_DTYPE, PAIR_DTYPE, PBA_INDEX_ALL, PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP,
                                       STRAND_OVERLAP_DTYPE)
from polish_helpers import oracle_polish_round
from test_align_rings_cpu import excursion_case

KERNELS = (PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP)
ALL_SLOTS = tuple(_lib.POOL_SLOTS) + ("scratch",) + tuple(_lib.IX_CACHE_SLOTS) + ("queue", "stage")
FIXED_SLOTS = ("queue",)          # 64 bytes for the life of the ctx: no decoy can make it larger
STATES = ("fresh", "scribble_00", "scribble_ff", "scribble_5a", "leftovers")
SCRIBBLE = {"scribble_00": 0x00, "scribble_ff": 0xFF, "scribble_5a": 0x5A}

_REF = {}


def ref(key, make):
    """a reference, computed once per session"""
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def mod(name):
    """a sibling GPU test module, for its check helpers (imported late: they pull in torch-sized things)"""
    return importlib.import_module(name)


def mask():
    return eng.mask_from_pattern(MASK_PAT)


def texts_of(S):
    return [S.get_text(i) for i in range(S.count)]


def pairs_of(B):
    return np.array(B.pairs, PAIR_DTYPE)


def workgroups(n_pairs):
    """workgroups of four wavefronts a traced launch over n_pairs asks for (persistent_grid; far below the chip's cap here)"""
    return (n_pairs + 3) // 4


def widest(B):
    return max(p[2] + p[5] for p in B.pairs)


class Case:
    def __init__(self, name, slots, checker, sizes, decoy, run):
        self.name, self.slots, self.checker, self.sizes, self.decoy, self.run = name, tuple(slots), checker, sizes, decoy, run

    def __repr__(self):
        return self.name


# ----------------------------------------------------------------------------- 1. the seed index in recycled arrays
B2 = ir.first_n_with_levels(2)
IX_SIZES = (17, ir.PART_AVG + 1, 30000, B2)       # logP 0; logP 1; one level of LVL_BITS (the locate's target); two levels
IX_DECOY = 1_100_000                               # two levels, one more bit of partitions than B2
LOC_R, LOC_READS, LOC_DECOY_READS = 0.30, 24, 96


@functools.lru_cache(maxsize=None)
def index_inputs():
    tig = mod("test_gpu_index")
    texts = {n: tig.rand_text(n, n % 1000 + 1) for n in IX_SIZES}
    g = np.frombuffer(texts[30000], np.uint8)
    reads, offs, _ = eng.synth_reads(102, g, LOC_DECOY_READS, 800)
    return dict(texts=texts, g=g, reads=reads, offs=offs, decoy=tig.rand_text(IX_DECOY, 7))


def index_sizes():
    big, parts = max(IX_SIZES), lambda n: 1 << ir.logp_of(n)
    assert ir.levels_of(big) == 2 == ir.levels_of(IX_DECOY)
    assert sorted({(ir.logp_of(n), ir.levels_of(n)) for n in IX_SIZES}) == [(0, 1), (1, 1), (ir.logp_of(30000), 1), (ir.LVL_BITS + 1, 2)]
    return {"ix_ent": (IX_DECOY, big), "ix_ent2": (IX_DECOY, big), "ix_off": (parts(IX_DECOY), parts(big)),
            "POOL_IX_OFFS": (parts(IX_DECOY), parts(big)), "POOL_IX_WORK": (parts(IX_DECOY), parts(big)),
            "POOL_LOC_ROWS": (LOC_DECOY_READS, LOC_READS), "POOL_LOC_AUX": (LOC_DECOY_READS, LOC_READS)}


def locate_sets(ctx, n_reads):
    I = index_inputs()
    T = ctx.seqs_from_text(I["g"], np.array([0, I["g"].size], np.uint64), strict_acgt=True)
    end = int(I["offs"][n_reads])
    return T, ctx.seqs_from_text(I["reads"][:end], I["offs"][:n_reads + 1], strict_acgt=True)


def index_decoy(ctx, oracle):
    S = ctx.seqs_from_list([index_inputs()["decoy"]])
    ctx.index_build(S, 0, mask(), PBA_INDEX_ALL).close()          # its three arrays go to the ctx's cache
    T, Rd = locate_sets(ctx, LOC_DECOY_READS)
    ix = ctx.index_build(T, 0, mask(), PBA_INDEX_ALL)
    _, st = ctx.locate(ix, T, 0, Rd, LOC_R, 50, 500)
    assert st["n_located"] > LOC_READS                             # more reads left a found row and counters than the case has
    ix.close()


def index_run(ctx, oracle):
    tig, I = mod("test_gpu_index"), index_inputs()
    for n in IX_SIZES:
        want = ref(("index", n), lambda: ir.np_index(I["texts"][n], mask(), "all"))
        S = ctx.seqs_from_list([I["texts"][n]])
        ix = ctx.index_build(S, 0, mask(), PBA_INDEX_ALL)
        try:
            tig.check_index(ix, want, mask(), f"stale/n{n}")
            if n == 30000:                                         # one pba_locate through the index in the recycled arrays
                T, Rd = locate_sets(ctx, LOC_READS)
                end = int(I["offs"][LOC_READS])
                wrows, wst = ref("locate", lambda: oracle.locator(I["g"], mask(), LOC_R, I["reads"][:end], I["offs"][:LOC_READS + 1], 50, 500,
                                                                   nthreads=4))
                for kernel in KERNELS:
                    rows, st = ctx.locate(ix, T, 0, Rd, LOC_R, 50, 500, kernel=kernel)
                    for c in ("nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs"):
                        assert (rows[c] == wrows[c]).all(), (kernel, c)
                    assert st == wst and wst["n_located"] > LOC_READS // 2, (st, wst)
        finally:
            ix.close()


# ----------------------------------------------------------------------------- 2. the aligners of a batch
EXC_KEEP = (0, 2, 5, 6, 12, 14)                    # three accepted and three "late" pairs: the late ones cannot be certified narrow


@functools.lru_cache(maxsize=None)
def exc_inputs():
    B, _, _ = excursion_case()
    return B, B.subset(list(EXC_KEEP))


def exc_redo_sizes():
    B, Bc = exc_inputs()
    assert sum(m["kind"] == "late" for m in Bc.meta) == 3
    # (the whole set re-runs len // 2 + 6 pairs at least: tests/test_gpu_align_rings.py: test_certificate_excursions; the case at
    # most all of its own)
    return {"POOL_REDO_IDS": (len(B.pairs) // 2 + 6, len(Bc.pairs))}


def exc_trace_sizes():
    B, Bc = exc_inputs()
    assert widest(B) >= widest(Bc)
    return dict(exc_redo_sizes(), scratch=(workgroups(len(B.pairs)) * widest(B), workgroups(len(Bc.pairs)) * widest(Bc)))


def align_batch_decoy(ctx, oracle):
    B, _ = exc_inputs()
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    ctx.align_batch(S, S, pairs_of(B), ar.EXC_R, kernel=PBA_KERNEL_BITVEC)
    assert ctx.last_profile()["n_redo"] > len(EXC_KEEP)


def align_batch_run(ctx, oracle):
    """k_align_pairs in ring 1 with its re-run in ring 2, and the row sweep, on the same pairs"""
    tar = mod("test_gpu_align_rings")
    _, Bc = exc_inputs()
    prof = tar.check_batch(ctx, oracle, Bc, ar.EXC_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == 1 and prof["nb_redo"] == 2 and 3 <= prof["n_redo"] <= len(Bc.pairs), prof
    assert tar.check_batch(ctx, oracle, Bc, ar.EXC_R, PBA_KERNEL_ROWSWEEP)["nb_first"] == 0


def align_trace_decoy(ctx, oracle):
    B, _ = exc_inputs()
    S = ctx.seqs_from_list(B.seqs, strict_acgt=True)
    ctx.align_batch_trace(S, S, pairs_of(B), ar.EXC_R, kernel=PBA_KERNEL_BITVEC)
    assert ctx.last_profile()["n_redo"] > len(EXC_KEEP)


def align_trace_run(ctx, oracle):
    tar = mod("test_gpu_align_rings")
    _, Bc = exc_inputs()
    prof = tar.check_batch(ctx, oracle, Bc, ar.EXC_R, PBA_KERNEL_BITVEC, scripts=True)
    assert prof["nb_first"] == 1 and prof["nb_redo"] == 2 and prof["n_redo"] >= 3, prof


@functools.lru_cache(maxsize=None)
def cigar_inputs():
    tgc = mod("test_gpu_cigar")
    D = ar.Batch()
    rng = np.random.RandomState(1)
    for tag, a, b, _ in cr.planted_pairs():                       # (the batch of test_group_edges_of_the_sink)
        D.add_pair(D.place(rng, a, False, 0), D.place(rng, b, False, 1), False, False, tag=tag)
    return D, tgc.flags_case()


def cigar_sizes():
    D, Bc = cigar_inputs()
    assert widest(D) > widest(Bc) and len(D.pairs) > len(Bc.pairs)
    return {"scratch": (workgroups(len(D.pairs)) * widest(D), workgroups(len(Bc.pairs)) * widest(Bc))}


def cigar_decoy(ctx, oracle):
    D, _ = cigar_inputs()
    S = ctx.seqs_from_list(D.seqs, strict_acgt=True)
    ctx.align_batch_cigar(S, S, pairs_of(D), cr.PLANT_R)


def cigar_run(ctx, oracle):
    tgc = mod("test_gpu_cigar")
    _, Bc = cigar_inputs()
    for flags in (0, cr.REVERSED | cr.B_IS_QUERY):
        assert tgc.check_batch(ctx, oracle, Bc, cr.PLANT_R, flags)["nb_first"] == 1


# ----------------------------------------------------------------------------- 3. the one-pair text entry points
TEXT_CLASS, TEXT_DECOY_CLASS = "accept_eq", "group:W193"


def band_cells(c):
    la, lb = len(c.a), len(c.b)
    m = min(la, lb)
    md = 1 + int(m * c.R)
    return (min(la, m + md) + 1) * (2 * md + 1)                   # (len_a + 1) * (2 max_dst + 1) after the clip of seq_aligner.h:94-102


def text_sizes():
    d, cs = ri.of_class(TEXT_DECOY_CLASS)[0], ri.of_class(TEXT_CLASS)
    small = max(len(c.a) + len(c.b) for c in cs)
    both = (len(d.a) + len(d.b), small)
    cells = (band_cells(d), max(band_cells(c) for c in cs))
    return {"POOL_TXT_IN": both, "POOL_TXT_OUT": both, "stage": both, "scratch": both, "POOL_TXT_PAR": cells, "POOL_TXT_CST": cells}


def text_decoy(ctx, oracle):
    d = ri.of_class(TEXT_DECOY_CLASS)[0]
    for t in (d, d.translated()):                                  # ACGT: the bit-vector array; other bytes: the row sweep
        ctx.align_text(t.mem_a(), t.mem_b(), t.R, not t.fa, not t.fb)
        ctx.align_text_trace(t.mem_a(), t.mem_b(), t.R, not t.fa, not t.fb)
        ctx.align_text_matrix(t.mem_a(), t.mem_b(), t.R, not t.fa, not t.fb)


def text_run(ctx, oracle):
    trs = mod("test_gpu_rowsweep")
    for form in ("acgt", "bytes"):
        trs.test_text_entry_points(ctx, oracle, form, TEXT_CLASS)
    trs.test_text_matrix(ctx, oracle, TEXT_CLASS)


# ----------------------------------------------------------------------------- 4. locate / map: a subset walk, a stream, spaced rounds
MAP_READS, STREAM_READS = 40, (40, 60)


@functools.lru_cache(maxsize=None)
def map_inputs():
    contigs, reads, flipped = msi.world()
    # the decoy: every read of the two real contigs long enough to be kept, turned so that only its reverse complement maps --
    # the + walk finds nothing and the - walk takes every read
    decoy = [x if f else map_ref.rc(x) for i, (x, f) in enumerate(zip(reads, flipped)) if i % 10 != 4 and len(x) >= msi.MIN_LEN]
    return contigs, reads[:MAP_READS], reads[STREAM_READS[0]:STREAM_READS[1]], decoy


def map_sizes():
    _, case, batch, decoy = map_inputs()
    n = max(len(case), len(batch))
    assert all(len(x) >= msi.MIN_LEN for x in decoy)
    return {s: (len(decoy), n) for s in ("POOL_LOC_ROWS", "POOL_LOC_AUX", "POOL_LOC_CTG", "POOL_LOC_IDS")}


def map_target(ctx):
    contigs = map_inputs()[0]
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    return T, ctx.index_build_set(T, mask())


def map_decoy(ctx, oracle):
    decoy = map_inputs()[3]
    T, ix = map_target(ctx)
    Rd = ctx.seqs_from_list(decoy, strict_acgt=True)
    rows, st = ctx.map_reads(ix, T, Rd, msi.R, msi.TRIALS, msi.MIN_LEN, strands=3)
    ix.close()
    # every read walked on -, and more of them found there than the case has reads: no entry of the kept rows / counters /
    # contigs / ids that the case's unwalked reads could hide behind is a zero
    assert st["n_second_walk"] == len(decoy) and st["strand"][1]["n_located"] > MAP_READS and not (rows["strand"] == 1).any()


def map_ref_rows(oracle, which):
    contigs, case, batch, _ = map_inputs()
    reads = case if which == "case" else batch
    return ref(("map", which), lambda: map_ref.map_reads_ref(oracle, contigs, reads, mask(), msi.R, msi.TRIALS, msi.MIN_LEN, strands=3)[:2])


def map_run(ctx, oracle):
    tgm = mod("test_gpu_map")
    _, case, batch, _ = map_inputs()
    want, wst = map_ref_rows(oracle, "case")
    assert 0 < wst[1]["n_reads_kept"] < wst[0]["n_reads_kept"] < len(case)      # the - walk is a strict subset, and reads below min_len exist
    T, ix = map_target(ctx)
    Rd = ctx.seqs_from_list(case, strict_acgt=True)
    for kernel in KERNELS:
        got, gst = ctx.map_reads(ix, T, Rd, msi.R, msi.TRIALS, msi.MIN_LEN, kernel=kernel, strands=3)
        tgm.same_rows(got, want)
        tgm.same_stats(gst, wst)
        assert [gst["strand"][k]["n_reads_kept"] for k in (0, 1)] == [wst[k]["n_reads_kept"] for k in (0, 1)]
        assert gst["n_second_walk"] == wst[1]["n_reads_kept"]
    # one small batch through pba_map_stream
    want, wst = map_ref_rows(oracle, "batch")
    st = ctx.map_stream(ix, T, msi.R, msi.TRIALS, msi.MIN_LEN, strands=3, slot_bytes=64 * 1400, slot_reads=64)
    st.submit_reads(batch)
    got, gst = st.collect()
    st.close()
    tgm.same_rows(got, want)
    tgm.same_stats(gst, wst)
    assert gst["n_second_walk"] == wst[1]["n_reads_kept"] > 0
    ix.close()


SPACED_DECOY = 200_000


def spaced_sizes():
    parts = lambda n: 1 << ir.logp_of(n)
    head_tail = 40000                                              # a PBA_INDEX_HEAD_TAIL index visits 2 x 20 000 positions at most
    return {"ix_ent": (SPACED_DECOY, head_tail), "ix_off": (parts(SPACED_DECOY), parts(head_tail)),
            "POOL_IX_OFFS": (parts(SPACED_DECOY), parts(head_tail)), "POOL_IX_WORK": (parts(SPACED_DECOY), parts(head_tail))}


def spaced_decoy(ctx, oracle):
    S = ctx.seqs_from_list([mod("test_gpu_index").rand_text(SPACED_DECOY, 9)])
    ctx.index_build(S, 0, mask(), PBA_INDEX_ALL).close()


def spaced_run(ctx, oracle):
    """pba_spaced_multi: an index built in the recycled arrays and dropped per round, every round after the first over the
    subset of reads not found yet"""
    mod("test_gpu_parity").test_spaced_multi_golden(ctx)


# ----------------------------------------------------------------------------- 5. all-vs-all
OVL_CASE = ("short", oi.SHORT_PATS[0])
OVL_DECOY_READS = 120


@functools.lru_cache(maxsize=None)
def ovl_decoy_texts():
    """120 reads of 300 bases, 25 apart on one text: ten times the case's reads, under the case's mask"""
    S = oi.Set(4343)
    G = S.rand(25 * OVL_DECOY_READS + 300)
    return [G[25 * i:25 * i + 300] for i in range(OVL_DECOY_READS)]


def ovl_sizes():
    S, _, pat, mt, om = oi.case_params(OVL_CASE)
    m = orf.mask_of(pat)
    n, nd = len(S.texts), OVL_DECOY_READS
    cand = orf.candidates(S.texts, None, m, mt, om)[1]
    dcand = orf.candidates(ovl_decoy_texts(), None, m, mt, om)[1]
    return {"POOL_OVL_SMALL": (nd, n), "POOL_OVL_TMP": (nd, n), "POOL_OVL_OUT": (nd * (nd - 1), n * (n - 1)),
            "POOL_OVL_CAND": (dcand, cand), "POOL_OVL_ITEMS": (dcand, cand), "POOL_OVL_REDO": (max(1024, dcand), max(1024, cand))}


def ovl_decoy(ctx, oracle):
    _, R, pat, mt, om = oi.case_params(OVL_CASE)
    S = ctx.seqs_from_list(ovl_decoy_texts(), strict_acgt=True)
    for kernel in KERNELS:
        _, st = ctx.overlap_all(S, orf.mask_of(pat), R, mt, om, kernel=kernel)
        assert st["n_listed"] > 0 and st["n_overlaps"] > OVL_DECOY_READS
        ctx.overlap_strands(S, orf.mask_of(pat), R, mt, om, strands=3, kernel=kernel)


def ovl_mixed(oracle):
    """the case's reads with every second one reverse-complemented, and the model of both passes of pba_overlap_strands over
    them: the +1 pass (queries as they are) and the -1 pass (the queries' reverse complements), as oi.expected composes a view"""
    S, R, pat, mt, om = oi.case_params(OVL_CASE)
    m = orf.mask_of(pat)
    mixed = [orf.comp(x) if i % 2 else x for i, x in enumerate(S.texts)]

    def make():
        out = []
        for qtexts in (mixed, [orf.comp(x) for x in mixed]):
            W = orf.walk_composition(oracle, mixed, qtexts, R, m, mt, om)
            W.update(texts=mixed, qtexts=qtexts, mask=m, R=R, max_trial=mt, overlap_min=om)
            out.append(W)
        return out
    return ref("ovl_mixed", make)


def ovl_run(ctx, oracle):
    """pba_overlap_all, the table / probes form in ranges of seven targets, and both passes of pba_overlap_strands over the
    reads with every second one turned round, both kernels, against the model"""
    toe = mod("test_gpu_overlap_edges")
    W, (P, M) = oi.expected(oracle, OVL_CASE), ovl_mixed(oracle)
    assert min(len(W["rows"]), len(P["rows"]), len(M["rows"])) >= 10
    S = ctx.seqs_from_list(W["texts"], strict_acgt=True)
    Sm = ctx.seqs_from_list(P["texts"], strict_acgt=True)
    for kernel in KERNELS:
        got, st = ctx.overlap_all(S, W["mask"], W["R"], W["max_trial"], W["overlap_min"], kernel=kernel)
        toe.check(got, st, W, kernel, "stale short")
        got, st = ctx.overlap_all_sharded(S, W["mask"], W["R"], W["max_trial"], W["overlap_min"], targets_per_call=7, kernel=kernel)
        toe.check(got, st, W, kernel, "stale short sharded")
        got, sts = ctx.overlap_strands(Sm, P["mask"], P["R"], P["max_trial"], P["overlap_min"], strands=3, kernel=kernel)
        assert set(got["strand"].tolist()) == {1, -1}
        toe.check(got[got["strand"] == 1], sts[0], P, kernel, "stale short mixed +")
        toe.check(got[got["strand"] == -1], sts[1], M, kernel, "stale short mixed -")


PARK_CASE, PARK_DECOY = "slot0", "two_in_item"


def park_sizes():
    return {"POOL_OVL_REDO_IN": (len(wi.parked_set(PARK_DECOY)["parked"]), len(wi.parked_set(PARK_CASE)["parked"]))}


def park_call(ctx, C):
    S = ctx.seqs_from_list(C["texts"], strict_acgt=True)
    return ctx.overlap_all(S, wi.MASK, C["R"], C["max_trial"], C["overlap_min"], t_lo=C["t_lo"], t_hi=C["t_hi"], kernel=PBA_KERNEL_BITVEC)


def park_decoy(ctx, oracle):
    C = wi.parked_set(PARK_DECOY)
    _, st = park_call(ctx, C)
    assert st["n_redo"] == len(C["parked"])


def park_run(ctx, oracle):
    """a run parked by the narrow ring and resumed from the copied list of parked runs"""
    toe = mod("test_gpu_overlap_edges")
    C = wi.parked_set(PARK_CASE)
    W = wi.model(oracle, C)
    got, st = park_call(ctx, C)
    toe.check(got, st, W, PBA_KERNEL_BITVEC, C["name"])
    assert st["n_redo"] == len(C["parked"]) == 1 and ctx.last_profile()["nb_redo"] == 2


BIG_PLANTS, BIG_DECOY_PLANTS, BIG_MEMBERS = 40, 60, 520


@functools.lru_cache(maxsize=None)
def big_target_set(plants):
    """One target with one 16-base window planted `plants` times, 48 bases apart, and 520 queries that end with that window
    (a bucket of 520 backward probes; a query's own last window is not a position it visits as a target): 520 x plants
    candidates on one target -- with 40 plants more than one LDS sort takes (PBA_IX_LDS_SORT_CAP), so the row-sweep form cuts the
    slice into pieces through the second candidate buffer.  Three members copy the target in front of the middle plant."""
    S = oi.Set(777)
    w = S.window()
    at = [(40 + 48 * i, w) for i in range(plants)]
    T = S.target("big", 40 + 48 * plants + 40, at)
    for i in range(BIG_MEMBERS):
        S.bwd(w, T if i in (0, BIG_MEMBERS // 2, BIG_MEMBERS - 1) else None, at[plants // 2][0])
    return S


def big_sizes():
    cand = [orf.candidates(big_target_set(k).texts, None, wi.MASK, 1, oi.RUN_MIN)[1] for k in (BIG_DECOY_PLANTS, BIG_PLANTS)]
    assert cand[1] > ir.define("PBA_IX_LDS_SORT_CAP") and BIG_MEMBERS * BIG_PLANTS > ir.define("PBA_IX_LDS_SORT_CAP")
    return {"POOL_OVL_TMP": (cand[0], cand[1])}


def big_decoy(ctx, oracle):
    S = ctx.seqs_from_list(big_target_set(BIG_DECOY_PLANTS).texts, strict_acgt=True)
    _, st = ctx.overlap_all(S, wi.MASK, oi.RUN_R, 1, oi.RUN_MIN, kernel=PBA_KERNEL_ROWSWEEP)
    assert st["n_big_targets"] == 1 and st["n_candidates"] >= BIG_MEMBERS * BIG_DECOY_PLANTS


def big_run(ctx, oracle):
    """the u64 user of POOL_OVL_TMP: a slice beyond one LDS sort, split into pieces and sorted piece by piece (row sweep); the
    bit-vector form on the same set cross-checks the input"""
    toe = mod("test_gpu_overlap_edges")
    texts = big_target_set(BIG_PLANTS).texts

    def make():
        W = orf.walk_composition(oracle, texts, texts, oi.RUN_R, wi.MASK, 1, oi.RUN_MIN)
        W.update(texts=texts, qtexts=texts, mask=wi.MASK, R=oi.RUN_R, max_trial=1, overlap_min=oi.RUN_MIN)
        return W
    W = ref("ovl_big", make)
    assert len(W["rows"]) >= 3 and W["pairs"] > ir.define("PBA_IX_LDS_SORT_CAP")
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    got, st = ctx.overlap_all(S, wi.MASK, oi.RUN_R, 1, oi.RUN_MIN, kernel=PBA_KERNEL_ROWSWEEP)
    toe.check(got, st, W, PBA_KERNEL_ROWSWEEP, "stale big target")
    assert st["n_big_targets"] == 1
    got, st = ctx.overlap_all(S, wi.MASK, oi.RUN_R, 1, oi.RUN_MIN, kernel=PBA_KERNEL_BITVEC)
    toe.check(got, st, W, PBA_KERNEL_BITVEC, "stale big target")


# ----------------------------------------------------------------------------- 6. pile-ups
def pile_sizes():
    _, _, rows = vb.pile_case()
    return {"scratch": (workgroups(4 * len(rows)), workgroups(len(rows)))}


def pile_decoy(ctx, oracle):
    contigs, reads, rows = vb.pile_case()
    S = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    _, n_voted = eng.Pileup(ctx, S).vote_mapped(Rd, np.concatenate([rows] * 4), vb.R, vb.OVERLAP_MIN)
    assert n_voted == 4 * len(rows)


def pile_run(ctx, oracle):
    mod("test_gpu_votebox").test_pileup_per_target_edges(ctx, oracle)


@functools.lru_cache(maxsize=None)
def correct_inputs():
    return mixed_reads(411, 412, 16, 1200, 3000, rl_min=800, extra=1)[0], mixed_reads(421, 422, 60, 1200, 6000, rl_min=800)[0]


def correct_sizes():
    case, decoy = correct_inputs()
    return {"POOL_OVL_SMALL": (len(decoy), len(case))}


def correct_decoy(ctx, oracle):
    S = ctx.seqs_from_list(correct_inputs()[1], strict_acgt=True)
    ctx.correct_reads(S, mask(), 0.30, 32, 64)


def correct_run(ctx, oracle):
    """pba_correct_reads == the oracle's rows voted and evolved by the oracle's pieces, target by target"""
    tgc = mod("test_gpu_correct")
    texts = correct_inputs()[0]

    def make():
        rows = oracle_rows(oracle, texts, mask(), 0.30, 32, 64, nthreads=4)
        per = tgc.rows_by_target(rows, len(texts))
        return [oracle_correct(oracle, texts, t, per[t], 1, 0.30)[3] for t in range(len(texts))], [len(p) for p in per]
    want, n_rows = ref("correct", make)
    assert sum(w != t for w, t in zip(want, texts)) * 2 >= len(texts) and n_rows[-1] == 0
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    out, crows, _ = ctx.correct_reads(S, mask(), 0.30, 32, 64)
    assert texts_of(out) == want
    assert [int(x) for x in crows["n_rows"]] == n_rows and [int(x) for x in crows["len_out"]] == [len(w) for w in want]


def polish_run(ctx, oracle):
    """one round of pba_polish_contigs == the restatement's rows voted and evolved by the oracle, contig by contig"""
    contigs, reads, _, _ = map_inputs()
    ref_rows, _ = map_ref_rows(oracle, "case")

    def make():
        rows = np.zeros(len(ref_rows), MAP_ROW_DTYPE)
        for f in ref_rows.dtype.names:
            rows[f] = ref_rows[f]
        return oracle_polish_round(oracle, contigs, reads, rows)
    want, voted = ref("polish", make)
    assert sum(voted) > 10 and sum(w != c for w, c in zip(want, contigs)) >= 2
    T = ctx.seqs_from_list(contigs, strict_acgt=True)
    Rd = ctx.seqs_from_list(reads, strict_acgt=True)
    out, rows_out, log = ctx.polish_contigs(T, Rd, mask(), msi.R, msi.TRIALS, msi.MIN_LEN, strands=3, overlap_min=64, weight=1, rounds=1)
    assert texts_of(out) == want and texts_of(T) == contigs
    assert [int(x) for x in rows_out["n_rows"]] == voted and int(log[0]["n_voted"]) == sum(voted)


# ----------------------------------------------------------------------------- 7. layout, place, stitch, consensus
LAY_DECOY_READS, LAY_DECOY_ROWS = 300, 3000


@functools.lru_cache(maxsize=None)
def layout_decoy_inputs():
    """the 2 000-read fuzz shape of tests/test_gpu_layout.py, shrunk: 300 reads of 50 - 300 bases, 3 000 random valid rows"""
    rng = np.random.default_rng(303)
    lens = [int(n) for n in rng.integers(50, 301, LAY_DECOY_READS)]
    texts = [rng.choice(layout_ref.ACGT, n).tobytes() for n in lens]
    return texts, place_ref.fuzz_rows(rng, lens, LAY_DECOY_ROWS)


def layout_decoy(ctx, oracle):
    texts, rows = layout_decoy_inputs()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    lay = ctx.layout(S, rows, 64, 2)
    lay.stitch(S)
    lay.place(S, rows)
    assert lay.stats["n_contigs"] > 3 and lay.place_stats["n_found"] > 20
    lay.close()


def layout_sizes():
    case = layout_ref.HAND_CASES[0]
    n = max(len(case["lens"]) if "lens" in case else len(layout_ref.hand_texts(case)), len(place_ref.HAND_LENS))
    rows = max(len(case["rows"]), len(place_ref.HAND_LAY_ROWS), max(len(c["rows"]) for c in place_ref.HAND_PLACE))
    return {"POOL_LAY_WORK": (LAY_DECOY_READS, n), "POOL_LAY_ROWS": (LAY_DECOY_ROWS, rows)}


def place_hand(ctx):
    tgp = mod("test_gpu_place")
    S = ctx.seqs_from_list(place_ref.hand_texts(), strict_acgt=True)
    lay = ctx.layout(S, layout_ref.make_rows(place_ref.HAND_LAY_ROWS), 64, 2)
    assert tgp.as_tuples(lay.rows(), layout_ref.ROW_FIELDS) == place_ref.HAND_TABLE
    for case in place_ref.HAND_PLACE:
        tgp.test_hand_cases(ctx, (S, lay), case)
    lay.close()


def layout_run(ctx, oracle):
    mod("test_gpu_layout").test_hand_rows(ctx, layout_ref.HAND_CASES[0])      # layout and stitch
    place_hand(ctx)


def laycons_sizes():
    return {"POOL_LAY_WORK": (LAY_DECOY_READS, 2 + 9 + 30), "POOL_LAY_ROWS": (LAY_DECOY_ROWS, 1 + 8 + 29)}


def laycons_run(ctx, oracle):
    mod("test_gpu_place").test_consensus_of_an_error_free_tiling_is_the_stitched_set(ctx)


# ----------------------------------------------------------------------------- 8. clip
CLIP_DECOY_READS, CLIP_DECOY_ROWS = 300, 3000


@functools.lru_cache(maxsize=None)
def clip_decoy_inputs():
    rng = np.random.default_rng(404)
    lens = [int(x) for x in rng.integers(40, 400, CLIP_DECOY_READS)]
    texts = [rng.choice(clip_ref.ACGT, n).tobytes() for n in lens]
    return texts, place_ref.fuzz_rows(rng, lens, CLIP_DECOY_ROWS)


def clip_sizes():
    case = clip_ref.HAND_CASES[0]
    dl = [len(t) for t in clip_decoy_inputs()[0]]
    return {"POOL_CLIP_ARENA": (sum(clip_ref.entries(n) for n in dl), sum(clip_ref.entries(n) for n in case["lens"])),
            "POOL_CLIP_WORK": (len(dl), len(case["lens"])), "POOL_LAY_ROWS": (CLIP_DECOY_ROWS, len(case["rows"])),
            # offsets and gathered text: the decoy's at least its offsets, the case's at most its offsets and every base
            "POOL_CLIP_TEXT": (8 * (len(dl) + 1), 8 * (len(case["lens"]) + 1) + sum(case["lens"]))}


def clip_decoy(ctx, oracle):
    texts, rows = clip_decoy_inputs()
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    cl = ctx.clip(S, rows, 12, 2)
    cl.apply(S)
    assert cl.stats["n_bases_out"] > 1000
    ctx.clip_coverage(S, rows, int(np.argmax([len(t) for t in texts])), 12)   # ... and the arena of the longest read alone
    cl.close()


def clip_run(ctx, oracle):
    """clip, clip_coverage of every (short) read and apply on the first hand case"""
    mod("test_gpu_clip").test_hand_rows(ctx, clip_ref.HAND_CASES[0])


# ----------------------------------------------------------------------------- 9. homopolymer compression
@functools.lru_cache(maxsize=None)
def hpc_inputs():
    reads, contigs = hpc_ref.biased_set(531, 8, 50, 200), hpc_ref.biased_set(532, 3, 300, 600)
    hr, hc = [hpc_ref.hpc(t) for t in reads], [hpc_ref.hpc(t) for t in contigs]
    rows = hpc_ref.random_map_rows(np.random.default_rng(533), [len(c) for c, _ in hr], [len(c) for c, _ in hc], 20)
    return reads, contigs, hr, hc, rows


@functools.lru_cache(maxsize=None)
def hpc_decoy_inputs():
    reads = hpc_ref.biased_set()
    contigs = hpc_ref.biased_set(521, 6, 500, 4000) + [b"T" * 100]
    hr, hc = [len(hpc_ref.hpc(t)[0]) for t in reads], [len(hpc_ref.hpc(t)[0]) for t in contigs]
    return reads, contigs, hr, hc, hpc_ref.random_overlap_rows(np.random.default_rng(534), hr, 257), \
        hpc_ref.random_map_rows(np.random.default_rng(535), hr, hc, 257)


def hpc_sizes():
    reads, contigs, hr, hc, rows = hpc_inputs()
    dreads, _, dhr, _, _, _ = hpc_decoy_inputs()
    touching = hpc_ref.touching_set()
    n = max(len(touching), len(hpc_ref.HAND_TEXTS), len(reads) + len(contigs))
    H = max(sum(len(hpc_ref.hpc(t)[0]) for t in touching), sum(len(c) for c, _ in hr), sum(len(c) for c, _ in hc))
    lifted = max(STRAND_OVERLAP_DTYPE.itemsize * len(hpc_ref.hand_rows()[0]), MAP_ROW_DTYPE.itemsize * len(rows))
    return {"POOL_HPC_WORK": (len(dreads), n), "POOL_HPC_TEXT": (sum(dhr), H), "POOL_LAY_ROWS": (MAP_ROW_DTYPE.itemsize * 257, lifted)}


def hpc_decoy(ctx, oracle):
    reads, contigs, _, _, orows, mrows = hpc_decoy_inputs()
    cr_, mr = ctx.seqs_hpc(ctx.seqs_from_list(reads, strict_acgt=True))
    cc, mc = ctx.seqs_hpc(ctx.seqs_from_list(contigs, strict_acgt=True))
    mr.lift_overlaps(orows)
    mr.lift_map_rows(mrows, mc)
    for x in (cr_, cc, mr, mc):
        x.close()


def hpc_run(ctx, oracle):
    """seqs_hpc on a set with empty sequences between non-empty ones (first[] has holes), lift_overlaps on the hand rows,
    lift_map_rows on twenty rows through two small maps"""
    tgh = mod("test_gpu_hpc")
    tgh.test_touching_and_empty_sequences(ctx)
    tgh.test_lift_hand_rows(ctx)
    reads, contigs, hr, hc, rows = hpc_inputs()
    want = hpc_ref.lift_map_rows(rows, [s for _, s in hr], [len(t) for t in reads], [s for _, s in hc])
    cr_, mr = ctx.seqs_hpc(ctx.seqs_from_list(reads, strict_acgt=True))
    cc, mc = ctx.seqs_hpc(ctx.seqs_from_list(contigs, strict_acgt=True))
    assert np.array_equal(mr.lift_map_rows(rows, mc), want) and int(rows["found"].sum()) >= 10
    for x in (cr_, cc, mr, mc):
        x.close()


# ----------------------------------------------------------------------------- 10. leftovers of another element type
def cross_rows_sizes():
    small = STRAND_OVERLAP_DTYPE.itemsize * max(len(layout_ref.HAND_CASES[0]["rows"]), len(clip_ref.HAND_CASES[0]["rows"]),
                                                len(place_ref.HAND_LAY_ROWS), max(len(c["rows"]) for c in place_ref.HAND_PLACE))
    return {"POOL_LAY_ROWS": (MAP_ROW_DTYPE.itemsize * 257, small)}


def cross_rows_decoy(ctx, oracle):
    """257 pba_map_row rows of 68 bytes where layout, clip and place then put pba_strand_overlap rows of 52"""
    reads, contigs, _, _, _, mrows = hpc_decoy_inputs()
    cr_, mr = ctx.seqs_hpc(ctx.seqs_from_list(reads, strict_acgt=True))
    cc, mc = ctx.seqs_hpc(ctx.seqs_from_list(contigs, strict_acgt=True))
    assert mr.lift_map_rows(mrows, mc).size == 257
    for x in (cr_, cc, mr, mc):
        x.close()


def cross_rows_run(ctx, oracle):
    mod("test_gpu_layout").test_hand_rows(ctx, layout_ref.HAND_CASES[0])
    mod("test_gpu_clip").test_hand_rows(ctx, clip_ref.HAND_CASES[0])
    place_hand(ctx)


FX_DECOY, FX_CASES = "fa_300rec", ("fa_2rec", "fq_plus_name")


def fx_want(name):
    c = fi.by_name(name)
    return c, ref(("fastx", name), lambda: fr.parse(c["data"], c["format"], c["keep"]))


def cross_recs_sizes():
    two = 2
    return {"POOL_FX_RECS": (40 * 300 + 4 * 301, max(16 * (two + 1), 40 * two + 4 * (two + 1)))}


def cross_recs_decoy(ctx, oracle):
    c = fi.by_name(FX_DECOY)
    S, ix = ctx.seqs_from_fastx(c["data"], c["format"])
    assert len(ix) == 300
    S.close()


def cross_recs_run(ctx, oracle):
    """300 records, then the writer's two u64 prefix arrays of a 2-sequence set, then 2 records: one slot, three element types"""
    tgf = mod("test_gpu_fastx")
    c, w = fx_want("fa_2rec")
    names = [x["name"] for x in w["records"]]
    S = ctx.seqs_from_list(w["seqs"])
    assert S.write_fasta(names, 60) == fr.format_fasta(names, w["seqs"], 60)
    tgf.check_parse(ctx, c, w)[0].close()


# ----------------------------------------------------------------------------- 11. FASTA / FASTQ
def fx_sizes():
    d, wd = fx_want(FX_DECOY)
    small = [fx_want(n) for n in FX_CASES]
    data = max(len(c["data"]) for c, _ in small)
    return {"POOL_FX_FILE": (len(d["data"]), data), "POOL_FX_TILES": ((len(d["data"]) + 4095) // 4096, (data + 4095) // 4096),
            "POOL_FX_LINES": (wd["n_lines"], max(w["n_lines"] for _, w in small)),
            "POOL_FX_RECS": (len(wd["records"]), max(len(w["records"]) for _, w in small)),
            "POOL_FX_IMG": (sum(len(s) for s in wd["seqs"]), max(len(c["data"]) for c, _ in small) + 64)}


def fx_decoy(ctx, oracle):
    c, w = fx_want(FX_DECOY)
    S, ix = ctx.seqs_from_fastx(c["data"], c["format"])            # one piece: the whole file in every slot
    assert ix.stats["n_pieces"] == 1
    q = fi.by_name("fq_300rec")
    ctx.seqs_from_fastx(q["data"], q["format"])[0].close()
    assert len(S.write_fasta([x["name"] for x in w["records"]], 60)) > len(c["data"]) // 2
    S.close()


def fx_run(ctx, oracle):
    """a FASTA and a FASTQ file cut into two pieces and more, and the writer, in buffers that held 300 records"""
    tgf = mod("test_gpu_fastx")
    for name in FX_CASES:
        c, w = fx_want(name)
        S, ix = tgf.check_parse(ctx, c, w, tgf.largest_record(w, len(c["data"])))
        assert ix.stats["n_pieces"] >= 2
        names = [x["name"] for x in w["records"]]
        for width in (0, 16, 60):
            assert S.write_fasta(names, width) == fr.format_fasta(names, w["seqs"], width), (name, width)
        S.close()


# ----------------------------------------------------------------------------- the list
CASES = [
    Case("index_regimes", ("ix_ent", "ix_off", "ix_ent2", "POOL_IX_OFFS", "POOL_IX_WORK", "POOL_LOC_ROWS", "POOL_LOC_AUX", "queue"),
         "test_gpu_index:check_index", index_sizes, index_decoy, index_run),
    Case("align_batch", ("POOL_REDO_IDS", "queue"), "test_gpu_align_rings:check_batch", exc_redo_sizes, align_batch_decoy, align_batch_run),
    Case("align_batch_trace", ("scratch", "POOL_REDO_IDS", "queue"), "test_gpu_align_rings:check_batch", exc_trace_sizes, align_trace_decoy,
         align_trace_run),
    Case("align_batch_cigar", ("scratch", "queue"), "test_gpu_cigar:check_batch", cigar_sizes, cigar_decoy, cigar_run),
    Case("text_entry_points", ("POOL_TXT_IN", "POOL_TXT_OUT", "POOL_TXT_PAR", "POOL_TXT_CST", "stage", "scratch", "queue"),
         "test_gpu_rowsweep:test_text_matrix", text_sizes, text_decoy, text_run),
    Case("map_subset_and_stream", ("POOL_LOC_ROWS", "POOL_LOC_AUX", "POOL_LOC_CTG", "POOL_LOC_IDS", "queue"), "test_gpu_map:same_stats",
         map_sizes, map_decoy, map_run),
    Case("spaced_multi", ("ix_ent", "ix_off", "POOL_IX_OFFS", "POOL_IX_WORK", "queue"), "test_gpu_parity:test_spaced_multi_golden",
         spaced_sizes, spaced_decoy, spaced_run),
    Case("overlap_forms", ("POOL_OVL_CAND", "POOL_OVL_TMP", "POOL_OVL_ITEMS", "POOL_OVL_REDO", "POOL_OVL_OUT", "POOL_OVL_SMALL", "queue"),
         "test_gpu_overlap_edges:check", ovl_sizes, ovl_decoy, ovl_run),
    Case("overlap_parked_run", ("POOL_OVL_REDO_IN", "queue"), "test_gpu_overlap_edges:check", park_sizes, park_decoy, park_run),
    Case("overlap_big_target", ("POOL_OVL_TMP", "queue"), "test_gpu_overlap_edges:check", big_sizes, big_decoy, big_run),
    Case("pileup_vote_evolve", ("scratch", "queue"), "test_gpu_votebox:test_pileup_per_target_edges", pile_sizes, pile_decoy, pile_run),
    Case("correct_reads", ("POOL_OVL_SMALL", "queue"), "correct_helpers:oracle_correct", correct_sizes, correct_decoy, correct_run),
    Case("polish_contigs", ("POOL_LOC_ROWS", "POOL_LOC_AUX", "POOL_LOC_CTG", "POOL_LOC_IDS", "queue"), "polish_helpers:oracle_polish_round",
         map_sizes, map_decoy, polish_run),
    Case("layout_place_stitch", ("POOL_LAY_WORK", "POOL_LAY_ROWS"), "test_gpu_layout:check_against_ref", layout_sizes, layout_decoy, layout_run),
    Case("layout_consensus", ("POOL_LAY_WORK", "POOL_LAY_ROWS"), "test_gpu_place:test_consensus_of_an_error_free_tiling_is_the_stitched_set",
         laycons_sizes, layout_decoy, laycons_run),
    Case("clip", ("POOL_CLIP_ARENA", "POOL_CLIP_WORK", "POOL_CLIP_TEXT", "POOL_LAY_ROWS"), "test_gpu_clip:check_against_ref", clip_sizes,
         clip_decoy, clip_run),
    Case("hpc", ("POOL_HPC_WORK", "POOL_HPC_TEXT", "POOL_LAY_ROWS"), "test_gpu_hpc:check_against_ref", hpc_sizes, hpc_decoy, hpc_run),
    Case("cross_type_lay_rows", ("POOL_LAY_ROWS",), "test_gpu_place:check_place", cross_rows_sizes, cross_rows_decoy, cross_rows_run),
    Case("cross_type_fx_recs", ("POOL_FX_RECS",), "test_gpu_fastx:check_parse", cross_recs_sizes, cross_recs_decoy, cross_recs_run),
    Case("fastx", ("POOL_FX_FILE", "POOL_FX_TILES", "POOL_FX_LINES", "POOL_FX_RECS", "POOL_FX_IMG"), "test_gpu_fastx:check_parse", fx_sizes,
         fx_decoy, fx_run),
]
