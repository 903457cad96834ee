"""Both strands in the all-vs-all overlapper: the device reverse complement of a read set (pba_seqs_revcomp) and the
strand-aware overlap entry points (pba_overlap_strands / _table).  Strand +1 rows are pba_overlap_all's; strand -1 rows
are the same computation with every query replaced by its reverse complement, checked against the CPU oracle's locked
spaced_seed round over a file of reverse-complemented reads, and independently through rc(rc(x)) == x.  Needs a real
MI355X (-m gpu)."""
import numpy as np
import pytest

from conftest import MASK_PAT
from pacbioassembly_amd import ProbeTable
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP, PbaError

pytestmark = pytest.mark.gpu
KERNELS = [PBA_KERNEL_ROWSWEEP, PBA_KERNEL_BITVEC]
OV_FIELDS = ("target", "query", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
ACGT = np.frombuffer(b"ACGT", np.uint8)


def rc(x: bytes) -> bytes:
    return x.translate(_COMP)[::-1]


def ov_tuples(rows):
    return [tuple(int(r[f]) for f in OV_FIELDS) for r in rows]


def exported(ctx, S):
    """The packed arena of a set (pba_seqs_export) and its offsets, on the host."""
    import torch
    buf = torch.zeros(max(S.packed_bytes, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()                  # the fill runs on torch's stream, the export on the engine's
    offs = S.export(buf.data_ptr(), buf.numel())
    torch.cuda.synchronize()
    return buf.cpu().numpy()[:S.packed_bytes].tobytes(), offs.tolist()


def same_set(ctx, got, want):
    assert got.count == want.count and got.max_len == want.max_len
    assert got.lengths().tolist() == want.lengths().tolist()
    for i in range(want.count):
        assert got.get_text(i) == want.get_text(i), i
    assert exported(ctx, got) == exported(ctx, want)          # byte for byte, pad bits and layout included


def edit_distance(a: bytes, b: bytes) -> int:
    """Global edit distance (Myers / Hyyro bit-vector over Python integers): a independent host check of a row's cost."""
    m = len(a)
    if m == 0:
        return len(b)
    peq = {}
    for i, c in enumerate(a):
        peq[c] = peq.get(c, 0) | (1 << i)
    full, top = (1 << m) - 1, 1 << (m - 1)
    pv, mv, score = full, 0, m
    for c in b:
        eq = peq.get(c, 0)
        xv = eq | mv
        xh = (((eq & pv) + pv) ^ pv) | eq
        ph = mv | (~(xh | pv) & full)
        mh = pv & xh
        if ph & top:
            score += 1
        elif mh & top:
            score -= 1
        ph = ((ph << 1) | 1) & full
        mh = (mh << 1) & full
        pv = mh | (~(xv | ph) & full)
        mv = ph & xv
    return score


def test_edit_distance_helper():
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = rng.choice(ACGT, rng.integers(0, 12)).tobytes()
        b = rng.choice(ACGT, rng.integers(0, 12)).tobytes()
        d = list(range(len(b) + 1))
        for i in range(1, len(a) + 1):
            prev, d[0] = d[0], i
            for k in range(1, len(b) + 1):
                prev, d[k] = d[k], min(d[k] + 1, d[k - 1] + 1, prev + (a[i - 1] != b[k - 1]))
        assert edit_distance(a, b) == d[len(b)], (a, b)


# ----------------------------------------------------------------------------- reverse complement of a set
RAGGED = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 64, 4002, 15000)


def random_texts(seed, lengths):
    rng = np.random.default_rng(seed)
    return [rng.choice(ACGT, n).tobytes() for n in lengths]


def test_seqs_revcomp_is_exact(ctx):
    texts = random_texts(11, RAGGED)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    R = ctx.seqs_revcomp(S)
    same_set(ctx, R, ctx.seqs_from_list([rc(x) for x in texts]))
    same_set(ctx, ctx.seqs_revcomp(R), S)                                   # rc(rc(S)) == S
    flip = np.random.default_rng(12).integers(0, 2, len(texts)).astype(np.uint8)
    flip[:2] = (1, 0)
    M = ctx.seqs_revcomp(S, flip)
    same_set(ctx, M, ctx.seqs_from_list([rc(x) if f else x for x, f in zip(texts, flip)]))
    same_set(ctx, ctx.seqs_revcomp(S, np.zeros(len(texts), np.uint8)), S)   # nothing flipped: a copy


def test_seqs_revcomp_of_a_binary_read_file(ctx):
    """Records of a binary read file are byte-aligned after 4-byte headers: the result is in pba_seqs_from_text's layout."""
    texts = random_texts(13, [n for n in RAGGED if n] + [7, 999, 1001])
    S = ctx.seqs_from_records(b"".join(eng.text2bin(t) for t in texts), 0, 1 << 30)
    assert S.count == len(texts)
    same_set(ctx, ctx.seqs_revcomp(S), ctx.seqs_from_list([rc(x) for x in texts]))
    flip = (np.arange(len(texts)) % 3 == 1).astype(np.uint8)
    same_set(ctx, ctx.seqs_revcomp(S, flip), ctx.seqs_from_list([rc(x) if f else x for x, f in zip(texts, flip)]))


def test_seqs_revcomp_refuses_non_acgt(ctx):
    S = ctx.seqs_from_list([b"ACGT", b"ACNT"])
    with pytest.raises(PbaError) as e:
        ctx.seqs_revcomp(S)
    assert e.value.status == -6
    with pytest.raises(ValueError):
        ctx.seqs_revcomp(ctx.seqs_from_list([b"ACGT"]), np.ones(2, np.uint8))


# ----------------------------------------------------------------------------- overlaps on both strands
@pytest.fixture(params=["census_then_exact_slices", "equal_room", "equal_room_overflows"])
def room(request, monkeypatch):
    """The three ways the scan of the bit-vector kernels sizes the survivors' slices (as tests/test_gpu_parity.py: prekeep)."""
    if request.param == "equal_room":
        monkeypatch.setenv("PBA_OVL_ROOM", "16384")
    if request.param == "equal_room_overflows":
        monkeypatch.setenv("PBA_OVL_ROOM", "4")
    return request.param


def check_intervals(rows, lens, texts=None, sample=0, seed=0):
    """Every row's intervals lie in its reads and span its match lengths; on a sample, the host edit distance between the
    target interval and the (for strand -1, reverse-complemented) query interval is at most the row's cost."""
    for r in rows:
        tl, ql = int(lens[r["target"]]), int(lens[r["query"]])
        assert 0 <= r["t_beg"] < r["t_end"] <= tl and 0 <= r["q_beg"] < r["q_end"] <= ql, r
        assert r["t_end"] - r["t_beg"] == r["matlen_a"] and r["q_end"] - r["q_beg"] == r["matlen_b"], r
    if texts is None or not sample or len(rows) == 0:
        return
    pick = np.random.default_rng(seed).choice(len(rows), min(sample, len(rows)), replace=False)
    for i in pick:
        r = rows[i]
        a = texts[r["target"]][r["t_beg"]:r["t_end"]]
        b = texts[r["query"]][r["q_beg"]:r["q_end"]]
        if r["strand"] < 0:
            b = rc(b)
        assert edit_distance(a, b) <= r["cost"], r


def mixed_set(seed_g, seed_r, n, rl, glen):
    g = eng.synth_genome(seed_g, glen)
    reads, offs, starts = eng.synth_reads(seed_r, g, n, rl)
    texts = [reads[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(n)]
    return texts, starts


@pytest.mark.parametrize("kernel", KERNELS)
def test_overlap_strands_vs_oracle_composition(ctx, oracle, kernel, room):
    """On a mixed-strand set: the -1 rows == the oracle's locked spaced_seed round of every target against the file of
    reverse-complemented reads (q != t), field for field, with the oracle's pair count; the +1 rows and stats == overlap_all;
    strands=1 == overlap_all; the target ranges and the exchange form concatenate to the same rows."""
    texts, _ = mixed_set(71, 72, 64, 1300, 9000)
    texts[5] = texts[5][:700]            # ragged: a short read, and one shorter than OVERLAP_MIN + 16
    texts[9] = texts[9][:70]
    flip = np.random.default_rng(73).integers(0, 2, len(texts)).astype(bool)
    texts = [rc(x) if f else x for x, f in zip(texts, flip)]
    n = len(texts)
    rc_texts = [rc(x) for x in texts]
    rc_file = b"".join(eng.text2bin(t) for t in rc_texts)
    rc_offs = np.cumsum([0] + [4 + (len(t) + 3) // 4 for t in rc_texts[:-1]]).astype(np.uint64)
    mask = eng.mask_from_pattern(MASK_PAT)
    want_rc, pairs_rc = [], 0
    for t in range(n):
        rows = oracle.spaced_round(texts[t], mask, 0.30, rc_file, rc_offs, 32, 64, buggy=False, nthreads=8)
        pairs_rc += int(rows["n_pairs"].sum()) - int(rows["n_pairs"][t])
        for q in range(n):
            if q != t and rows["found"][q]:
                want_rc.append((t, q, int(rows["j"][q]), int(rows["dir"][q]), int(rows["ref_pos"][q]), int(rows["cost"][q]),
                                int(rows["matlen_a"][q]), int(rows["matlen_b"][q])))
    assert len(want_rc) > 50
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    want_fwd, wst = ctx.overlap_all(S, mask, 0.30, 32, 64, kernel=kernel)
    assert len(want_fwd) > 50
    got, st = ctx.overlap_strands(S, mask, 0.30, 32, 64, strands=3, kernel=kernel)
    assert ov_tuples(got[got["strand"] < 0]) == want_rc
    assert ov_tuples(got[got["strand"] > 0]) == ov_tuples(want_fwd)
    assert {k: v for k, v in st[0].items() if not k.endswith("_ms")} == {k: v for k, v in wst.items() if not k.endswith("_ms")}
    assert st[1]["n_overlaps"] == len(want_rc) and st[1]["n_pairs"] == pairs_rc
    keys = [(int(r["target"]), int(r["query"]), -int(r["strand"])) for r in got]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)              # (target, query, strand), +1 before -1
    check_intervals(got, [len(x) for x in texts], texts, sample=40, seed=1)
    # one strand at a time; the rc set handed in
    one, st1 = ctx.overlap_strands(S, mask, 0.30, 32, 64, strands=1, kernel=kernel)
    assert ov_tuples(one) == ov_tuples(want_fwd) and (one["strand"] == 1).all() and st1[1]["n_overlaps"] == 0
    Src = ctx.seqs_revcomp(S)
    two, _ = ctx.overlap_strands(S, mask, 0.30, 32, 64, strands=2, kernel=kernel, reads_rc=Src)
    assert ov_tuples(two) == want_rc and (two["strand"] == -1).all()
    # target ranges concatenate to the one-call answer
    parts = [ctx.overlap_strands(S, mask, 0.30, 32, 64, t_lo=a, t_hi=b, kernel=kernel, reads_rc=Src)[0]
             for a, b in ((0, 20), (20, 21), (21, 64))]
    assert np.array_equal(np.concatenate(parts), got)
    # exchange form: every "rank" emits the probes of its shard of the rc queries (and of the forward ones), the padded
    # buffers are concatenated, the gathered lists build the two tables, target ranges go through against them
    import torch
    shards, cap = ((0, 22), (22, 43), (43, 64)), 22 * 64
    tabs = []
    for Q in (S, Src):
        gathered = torch.full((len(shards) * cap,), -1, dtype=torch.int64, device="cuda")
        for k, (a, b) in enumerate(shards):
            ctx.overlap_probes(Q, a, b, mask, 32, gathered[k * cap:(k + 1) * cap].data_ptr(), cap)
        torch.cuda.synchronize()
        tabs.append(ProbeTable(ctx, gathered.data_ptr(), gathered.numel(), mask, 32))
        del gathered
    assert tabs[0].entries == st[0]["n_probe_entries"] and tabs[1].entries == st[1]["n_probe_entries"]
    parts = [ctx.overlap_strands_table(S, Src, tabs[0], tabs[1], 0.30, 64, a, b, kernel=kernel)[0]
             for a, b in ((0, 5), (5, 6), (6, 40), (40, 64))]
    assert np.array_equal(np.concatenate(parts), got)
    rc_only = ctx.overlap_strands_table(S, Src, None, tabs[1], 0.30, 64, kernel=kernel)[0]
    assert ov_tuples(rc_only) == want_rc
    got3, st3 = ctx.overlap_strands_sharded(S, mask, 0.30, 32, 64, targets_per_call=17, kernel=kernel)
    assert np.array_equal(got3, got) and st3[1]["n_pairs"] == pairs_rc and st3[0]["n_pairs"] == wst["n_pairs"]


def flip_equivalence(ctx, texts, ranges, seed, kernel=eng.PBA_KERNEL_AUTO):
    """Targets that were not flipped: their rows on strand (flip[q] ? -1 : +1) over the mixed set == overlap_all's rows over
    the original set (rc(rc(x)) == x).  Returns the mixed set's rows."""
    n = len(texts)
    flip = np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(texts, strict_acgt=True)
    M = ctx.seqs_revcomp(S, flip)
    all_rows, checked = [], 0
    for a, b in ranges:
        want, _ = ctx.overlap_all(S, mask, 0.30, 32, 64, t_lo=a, t_hi=b, kernel=kernel)
        got, st = ctx.overlap_strands(M, mask, 0.30, 32, 64, t_lo=a, t_hi=b, kernel=kernel)
        assert st[0]["n_overlaps"] + st[1]["n_overlaps"] == len(got)
        sel = np.array([not flip[int(r["target"])] and int(r["strand"]) == (-1 if flip[int(r["query"])] else 1) for r in got], bool)
        keep = np.array([not flip[int(r["target"])] for r in want], bool)
        assert ov_tuples(got[sel]) == ov_tuples(want[keep])
        checked += int(keep.sum())
        all_rows.append(got)
    assert checked > 20
    mixed = [rc(x) if f else x for x, f in zip(texts, flip)]
    return np.concatenate(all_rows), mixed


@pytest.mark.parametrize("kernel", KERNELS)
def test_overlap_strands_flip_equivalence_1300(ctx, kernel):
    texts, _ = mixed_set(81, 82, 160, 1300, 16000)
    rows, mixed = flip_equivalence(ctx, texts, [(0, 160)], 83, kernel)
    check_intervals(rows, [len(x) for x in mixed], mixed, sample=60, seed=2)


def test_overlap_strands_flip_equivalence_15kb(ctx):
    texts, _ = mixed_set(91, 92, 240, 15000, 180000)                       # 20x
    rows, mixed = flip_equivalence(ctx, texts, [(0, 12), (100, 112), (228, 240)], 93)
    check_intervals(rows, [len(x) for x in mixed], mixed, sample=6, seed=3)


def test_overlap_strands_argument_checks(ctx):
    texts, _ = mixed_set(61, 62, 12, 900, 4000)
    mask = eng.mask_from_pattern(MASK_PAT)
    S = ctx.seqs_from_list(texts, strict_acgt=True)

    def status(**kw):
        with pytest.raises(PbaError) as e:
            ctx.overlap_strands(S if "reads" not in kw else kw.pop("reads"), mask, 0.30, 32, 64, **kw)
        return e.value.status

    assert status(reads_rc=ctx.seqs_from_list([rc(x) for x in texts[:-1]])) == -1              # another count
    assert status(reads_rc=ctx.seqs_from_list([rc(x) for x in texts[:-1]] + [texts[-1][:-1]])) == -1   # another length
    assert status(strands=0) == -1 and status(strands=4) == -1
    assert status(reads=ctx.seqs_from_list([x[:-1] + b"N" for x in texts])) == -6
    assert status(reads_rc=ctx.seqs_from_list([x[:-1] + b"N" for x in texts])) == -6
    Src = ctx.seqs_revcomp(S)
    import torch
    probes = torch.full((12 * 64,), -1, dtype=torch.int64, device="cuda")
    ctx.overlap_probes(Src, 0, 12, mask, 32, probes.data_ptr(), probes.numel())
    torch.cuda.synchronize()
    tab = ProbeTable(ctx, probes.data_ptr(), probes.numel(), mask, 32)
    for args in ((S, None, None, tab), (S, Src, None, None)):                # tab_rc without reads_rc; no table at all
        with pytest.raises(PbaError) as e:
            ctx.overlap_strands_table(*args, 0.30, 64)
        assert e.value.status == -1
    # a mismatched rc set of the same lengths is not detected: it gives the -1 rows of what it holds
    got, _ = ctx.overlap_strands(S, mask, 0.30, 32, 64, strands=2, reads_rc=S)
    want, _ = ctx.overlap_all(S, mask, 0.30, 32, 64)
    assert ov_tuples(got) == ov_tuples(want)
