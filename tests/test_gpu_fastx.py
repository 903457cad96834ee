"""pba_seqs_from_fastx and pba_seqs_write_fasta on the device against the restatement of the rules (fastx_ref.py), on every case
of fastx_inputs.py: the set byte for byte what seqs_from_list makes of the restatement's sequences, the index field by field, the
stats; every refusal with its line number; the answer under every cut into pieces; the writer against plain formatting; and
map_reads on parsed files.  All comparisons exact.  test_fastx_cpu.py proves what the cases are.  Needs a real MI355X (-m gpu)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fastx_inputs as fi
import fastx_ref as fr
from conftest import MASK_PAT, ROOT
from pacbioassembly_amd import _lib
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_FX_FASTA, PBA_FX_FASTQ, PBA_FX_KEEP_CASE, PBA_FX_STRICT_ACGT, PbaError
from test_gpu_stream import export_bytes

pytestmark = pytest.mark.gpu
OK = [c for c in fi.cases() if c["ok"]]
BAD = [c for c in fi.cases() if not c["ok"]]


def flags_of(c):
    return PBA_FX_KEEP_CASE if c["keep"] else 0


@pytest.fixture(scope="module")
def want():
    """the restatement of every case, computed once"""
    return {c["name"]: fr.parse(c["data"], c["format"], c["keep"]) for c in fi.cases()}


def same_set(ctx, S, seqs):
    """S is byte for byte the set seqs_from_list makes of `seqs`"""
    W = ctx.seqs_from_list(seqs)
    assert S.count == len(seqs) and S.lengths().tolist() == [len(s) for s in seqs] and S.max_len == W.max_len
    got, want = export_bytes(S), export_bytes(W)
    assert got[1].tolist() == want[1].tolist() and np.array_equal(got[0], want[0])
    assert S.non_acgt == W.non_acgt == any(set(s) - set(b"ACGT") for s in seqs)
    W.close()


def same_index(ix, w):
    r = ix.recs()
    assert len(r) == len(w["records"])
    for f in fr.REC_FIELDS:
        assert r[f].tolist() == [x[f] for x in w["records"]], f


def check_parse(ctx, c, w, max_piece=0):
    S, ix = ctx.seqs_from_fastx(c["data"], c["format"], flags_of(c), max_piece)
    same_set(ctx, S, w["seqs"])
    same_index(ix, w)
    assert ix.names(c["data"]) == [x["name"].decode("latin-1") for x in w["records"]]
    st = ix.stats
    assert (st["format"], st["n_records"], st["n_bytes"], st["max_len"]) == (w["format"], len(w["seqs"]), len(c["data"]), S.max_len)
    assert (st["n_bases"], st["n_lines"], st["n_folded"]) == (sum(len(s) for s in w["seqs"]), w["n_lines"], w["n_folded"])
    assert st["n_pieces"] >= (1 if c["data"] else 0)
    return S, ix


# ----------------------------------------------------------------------------- 1. every parsing case
@pytest.mark.parametrize("c", OK, ids=lambda c: c["name"])
def test_parsing_case(ctx, want, c):
    S, ix = check_parse(ctx, c, want[c["name"]])
    assert ix.stats["n_pieces"] == (1 if c["data"] else 0)
    S.close()


def test_read_fastx_and_memmap(ctx, want, tmp_path):
    for name in ("fa_300rec", "empty"):
        (tmp_path / name).write_bytes(fi.by_name(name)["data"])
        S, ix = ctx.read_fastx(str(tmp_path / name))
        same_set(ctx, S, want[name]["seqs"])
        same_index(ix, want[name])


# ----------------------------------------------------------------------------- 2. every failing case
def refused(ctx, data, format=0, flags=0, max_piece=0):
    """status and error text of a refused parse; neither a set nor an index comes back"""
    buf = np.frombuffer(data, np.uint8)
    h, ih, st = C.c_void_p(0xDEAD), C.c_void_p(0xDEAD), _lib.PbaFastxStats()
    rc = ctx.lib.pba_seqs_from_fastx_budget(ctx.h, C.c_void_p(buf.ctypes.data), len(data), format, flags, C.byref(h), C.byref(ih), C.byref(st),
                                            max_piece)
    assert rc != 0 and not h.value and not ih.value and st.n_records == 0
    return rc, ctx.lib.pba_ctx_error(ctx.h).decode()


@pytest.mark.parametrize("c", BAD, ids=lambda c: c["name"])
def test_failing_case(ctx, want, c):
    rc, text = refused(ctx, c["data"], c["format"], flags_of(c))
    assert rc == _lib.PBA_E_INVALID
    assert [int(v) for v in re.findall(r"line (\d+)", text)] == [want[c["name"]][1]], text
    nxt = fi.by_name("fa_lengths_w60")                         # the ctx still parses the next case correctly
    check_parse(ctx, nxt, want[nxt["name"]])[0].close()


def test_strict_acgt_and_bad_arguments(ctx, want):
    c = fi.by_name("fa_N_and_space")
    rc, text = refused(ctx, c["data"], flags=PBA_FX_STRICT_ACGT)
    assert rc == _lib.PBA_E_ALPHABET and "ACGT" in text
    check_parse(ctx, c, want[c["name"]])[0].close()
    ok = fi.by_name("fa_2rec")
    S, _ = ctx.seqs_from_fastx(ok["data"], flags=PBA_FX_STRICT_ACGT)              # a clean file passes
    same_set(ctx, S, want["fa_2rec"]["seqs"])
    assert refused(ctx, ok["data"], format=3)[0] == _lib.PBA_E_INVALID and refused(ctx, ok["data"], flags=4)[0] == _lib.PBA_E_INVALID
    with pytest.raises(PbaError) as e:                          # the aligning entry points refuse what the file held
        N, _ = ctx.seqs_from_fastx(c["data"])
        ctx.seqs_revcomp(N)
    assert e.value.status == _lib.PBA_E_ALPHABET


# ----------------------------------------------------------------------------- 3. pieces
def largest_record(w, n):
    starts = [r["hdr_off"] for r in w["records"]] + [n]
    return max(b - a for a, b in zip(starts, starts[1:]))


@pytest.mark.parametrize("name", ["fa_300rec"] + [c["name"] for c in OK if c["name"].startswith("fq_")])
def test_pieces(ctx, want, name):
    c, w = fi.by_name(name), want[name]
    big = largest_record(w, len(c["data"]))
    for budget in (big, 2 * big):
        S, ix = check_parse(ctx, c, w, budget)
        assert (ix.stats["n_pieces"] > 1) == (len(c["data"]) > budget), (budget, ix.stats)      # a piece holds at most `budget` bytes
        if name in ("fa_300rec", "fq_300rec") or (budget == big and len(w["records"]) > 1):
            assert ix.stats["n_pieces"] > 1
        S.close()
    rc, text = refused(ctx, c["data"], c["format"], flags_of(c), big - 1)
    k = max(range(len(w["records"])), key=lambda i: ([r["hdr_off"] for r in w["records"]] + [len(c["data"])])[i + 1] - w["records"][i]["hdr_off"])
    assert rc == _lib.PBA_E_TOOLONG and [int(v) for v in re.findall(r"hdr_off (\d+)", text)] == [w["records"][k]["hdr_off"]], text


def test_pieces_do_not_hide_a_refusal(ctx, want):
    for name in ("bad_fq_late", "bad_fq_blank_between", "bad_fq_three_line_last"):
        c = fi.by_name(name)
        for budget in (100, 200, 1000):
            rc, text = refused(ctx, c["data"], c["format"], 0, budget)
            assert rc == _lib.PBA_E_INVALID and [int(v) for v in re.findall(r"line (\d+)", text)] == [want[name][1]], (name, budget, text)


# ----------------------------------------------------------------------------- 4. the writer
WRITER = ["fa_zero_inside", "fa_lengths_w60", "fa_300rec", "fq_empty_seq", "fa_wrap63", "fa_hdr_hdr"]


@pytest.mark.parametrize("name", WRITER)
def test_writer(ctx, want, name):
    c, w = fi.by_name(name), want[name]
    S, ix = ctx.seqs_from_fastx(c["data"], c["format"], flags_of(c))
    names = [x["name"] for x in w["records"]]
    n = len(names)
    zero = [i for i, s in enumerate(w["seqs"]) if not s]
    ranges = [(0, n), (n // 2, n // 2)] + ([(zero[0], zero[-1] + 1)] if len(zero) >= 2 else [])     # ... from and to a zero-length sequence
    assert name != "fa_zero_inside" or ranges[2] == (1, 5)
    for width in (0, 1, 16, 60, 61):
        for lo, hi in ranges:
            assert S.write_fasta(names[lo:hi], width, lo, hi) == fr.format_fasta(names[lo:hi], w["seqs"][lo:hi], width), (width, lo, hi)
            assert S.write_fasta(None, width, lo, hi) == fr.format_fasta([b"%d" % i for i in range(lo, hi)], w["seqs"][lo:hi], width)
    # the size-only call, a cap one byte short, and the image parsed again
    img = S.write_fasta(names, 60)
    size = C.c_uint64()
    assert ctx.lib.pba_seqs_write_fasta(ctx.h, S.h, 0, n, None, None, 60, None, 0, C.byref(size)) == 0
    assert size.value == len(fr.format_fasta([b"%d" % i for i in range(n)], w["seqs"], 60))
    out = np.full(size.value + 8, 0xA5, np.uint8)
    size2 = C.c_uint64()
    rc = ctx.lib.pba_seqs_write_fasta(ctx.h, S.h, 0, n, None, None, 60, C.c_void_p(out.ctypes.data), size.value - 1, C.byref(size2))
    assert rc == _lib.PBA_E_INVALID and size2.value == size.value and (out == 0xA5).all()
    assert ctx.lib.pba_seqs_write_fasta(ctx.h, S.h, 2, 1, None, None, 60, None, 0, C.byref(size2)) == _lib.PBA_E_INVALID
    assert ctx.lib.pba_seqs_write_fasta(ctx.h, S.h, 0, n + 1, None, None, 60, None, 0, C.byref(size2)) == _lib.PBA_E_INVALID
    back, bix = ctx.seqs_from_fastx(img, PBA_FX_FASTA)
    same_set(ctx, back, w["seqs"])
    assert bix.names(img) == [x.decode("latin-1") for x in names]
    ctx.trim()                                                  # the work buffers are the pool's: gone, and the next call still works
    assert S.write_fasta(names, 60) == img


# ----------------------------------------------------------------------------- 5. one end-to-end tie
def test_map_reads_on_parsed_files(ctx, tmp_path):
    contigs = [bytes(eng.synth_genome(70 + k, n)) for k, n in enumerate((9000, 6000, 4000))]
    reads, rnames = [], []
    for k, (g, n) in enumerate(zip(contigs, (16, 14, 10))):
        text, offs, _ = eng.synth_reads(700 + k, np.frombuffer(g, np.uint8), n, 900)      # synth_reads' own error mix
        reads += [bytes(text[int(offs[i]):int(offs[i + 1])]) for i in range(n)]
    rs = np.random.RandomState(5)
    for i in range(len(reads)):
        if i % 3 == 1:
            reads[i] = reads[i][::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))
        rnames.append(b"read_%d/%d" % (i, i * 7))
    cnames = [b"ctgA", b"ctgB", b"ctgC"]
    fa = fi.fasta([(nm + b" len=%d" % len(s), s) for nm, s in zip(cnames, contigs)], 70)
    fq = fi.fastq([(nm + b" some comment", s, b"+", fi.qual(rs, len(s))) for nm, s in zip(rnames, reads)])
    assert len(reads) == 40
    T, tix = ctx.seqs_from_fastx(fa)
    Rd, rix = ctx.seqs_from_fastx(fq)
    assert tix.stats["format"] == PBA_FX_FASTA and rix.stats["format"] == PBA_FX_FASTQ
    mask = eng.mask_from_pattern(MASK_PAT)
    rows, _ = ctx.map_reads(ctx.index_build_set(T, mask), T, Rd, 0.30, 50, 500, strands=3)
    T2, R2 = ctx.seqs_from_list(contigs, strict_acgt=True), ctx.seqs_from_list(reads, strict_acgt=True)
    rows2, _ = ctx.map_reads(ctx.index_build_set(T2, mask), T2, R2, 0.30, 50, 500, strands=3)
    assert rows.tobytes() == rows2.tobytes() and int(rows["found"].sum()) >= 20 and set(rows["strand"][rows["found"] == 1].tolist()) == {1, -1}
    Rc = ctx.seqs_revcomp(Rd)
    runs, counts, _, _, _ = ctx.map_cigar(T, Rd, rows, 0.30, reads_rc=Rc)
    lines = eng.paf_map_lines(rows, counts, runs, Rd.lengths(), T.lengths(), rix.names(fq), tix.names(fa))
    found = rows[rows["found"] == 1]
    assert [ln.split("\t")[0] for ln in lines] == [rnames[int(r["read"])].decode() for r in found]
    assert [ln.split("\t")[5] for ln in lines] == [cnames[int(r["contig"])].decode() for r in found]
    # examples/map_fastx_gpu.cpp: the same files from disk, the same lines on stdout
    libdir = os.path.join(ROOT, "pacbioassembly_amd", "lib")
    exe = str(tmp_path / "map_fastx_gpu")
    subprocess.run(["g++", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "examples", "map_fastx_gpu.cpp"), "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}"], check=True)
    (tmp_path / "c.fa").write_bytes(fa)
    (tmp_path / "r.fq").write_bytes(fq)
    r = subprocess.run([exe, str(tmp_path / "c.fa"), str(tmp_path / "r.fq"), MASK_PAT, "0.30", "3"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().splitlines() == lines and len(lines) >= 20
