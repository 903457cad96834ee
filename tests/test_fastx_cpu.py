"""FASTA / FASTQ input without a GPU: the restatement of the rules (fastx_ref.py) against expectations written by hand; the host
arithmetic of the C ABI -- pba_fastx_sniff, pba_fastx_cut -- against brute force at every `want` of every case (fastx_inputs.py);
the new symbols, structs and NULL checks; csrc/fastx_lines.h alone as a stand-alone host program (tests/cpp/fastx_main.cpp, under
ASan + UBSan where the compiler has the runtimes) equal to the restatement on every case; and examples/map_fastx_gpu.cpp over
include/pba.h.  Nothing is loaded into python but libpba.so."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import fastx_inputs as fi
import fastx_ref as fr
from conftest import HERE, ROOT

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"]
NEW_SYMBOLS = ["pba_seqs_from_fastx", "pba_seqs_from_fastx_budget", "pba_fastx_index_count", "pba_fastx_index_recs",
               "pba_fastx_index_destroy", "pba_fastx_sniff", "pba_fastx_cut", "pba_seqs_write_fasta"]


def rules_of(c):
    """the format whose record starts pba_fastx_cut looks for when it is handed the case's format"""
    f = c["format"] or fr.sniff(c["data"])[0]
    return f if f > 0 else (fr.FASTA if f == 0 else None)


# ----------------------------------------------------------------------------- the restatement and the cases
def test_restatement_against_hand_written_expectations():
    assert len(fi.HAND) >= 12
    for name, want in fi.HAND.items():
        c = fi.by_name(name)
        got = fr.parse(c["data"], c["format"], c["keep"])
        if want[0] == "error":
            assert got == want and not c["ok"], name
        else:
            assert c["ok"] and got["format"] == want[0], name
            assert [(r["name"], s) for r, s in zip(got["records"], got["seqs"])] == want[1], name
            assert len(got["records"]) == len(got["seqs"]) == len(want[1])
    r = fr.parse(fi.by_name("fa_blank_lines")["data"])["records"]
    assert [(x["hdr_off"], x["seq_off"], x["hdr_len"], x["seq_len"], x["n_seq_lines"]) for x in r] == [(3, 7, 1, 7, 2), (19, 25, 1, 2, 1)]
    r = fr.parse(fi.by_name("fa_hdr_at_eof")["data"])["records"]
    assert (r[1]["hdr_off"], r[1]["seq_off"], r[1]["seq_len"], r[1]["n_seq_lines"]) == (8, 10, 0, 0)   # the byte after the header line: the end
    q = fr.parse(b"@a b\nACG\n+x\n@+I\n")
    assert q["format"] == fr.FASTQ and q["seqs"] == [b"ACG"]
    assert {k: q["records"][0][k] for k in fr.REC_FIELDS} == dict(hdr_off=0, seq_off=5, qual_off=12, hdr_len=3, name_len=1, seq_len=3, n_seq_lines=1)
    assert fr.parse(b">a\nacgTn\n")["seqs"] == [b"ACGTN"] and fr.parse(b">a\nacgTn\n")["n_folded"] == 4
    assert fr.parse(b">a\nacgTn\n", keep_case=True)["seqs"] == [b"acgTn"]
    assert fr.parse(b">a\r\nAC\r\r\n")["seqs"] == [b"AC\r"]                   # one "\r" only
    assert fr.parse(b"@r\n\n\n", fr.FASTQ) == ("error", 2)                      # trailing blank lines go first: the sequence line is missing


def test_every_case_is_what_its_name_says():
    cs = fi.cases()
    for c in cs:
        got = fr.parse(c["data"], c["format"], c["keep"])
        assert (not isinstance(got, tuple)) == c["ok"], c["name"]
        assert c["ok"] == (not c["name"].startswith("bad_")), c["name"]
    p = {c["name"]: fr.parse(c["data"], c["format"], c["keep"]) for c in cs if c["ok"]}
    for w in fi.WIDTHS:
        r = p[f"fa_wrap{w}"]["records"]
        assert [x["seq_len"] for x in r] == [2 * w + 3, w, min(w, 7)] and r[0]["n_seq_lines"] == -(-(2 * w + 3) // w) and r[1]["n_seq_lines"] == 1
    assert set(fi.WIDTHS) >= {1, 15, 16, 17, 60, 63, 64, 65, 4095, 4096, 4097, 16383, 16384, 16385}
    assert [x["seq_len"] for x in p["fa_lengths_w60"]["records"]] == fi.LENGTHS == [x["seq_len"] for x in p["fa_lengths_oneline"]["records"]]
    assert [len(p[n]["records"]) for n in ("fa_1rec", "fa_2rec", "fa_300rec", "fq_300rec")] == [1, 2, 300, 300]
    assert p["fa_line70000"]["records"][0]["n_seq_lines"] == 1 and p["fa_line70000"]["records"][0]["seq_len"] == 70000
    for k in range(6, 15):
        d = fi.by_name(f"fa_cr_split{k}")["data"]
        assert d[2 ** k - 1:2 ** k + 1] == b"\r\n" and [len(s) for s in p[f"fa_cr_split{k}"]["seqs"]] == [70, 33]
    assert b"\r" not in b"".join(p["fa_crlf"]["seqs"] + p["fq_crlf"]["seqs"]) and fi.by_name("fa_crlf")["data"].count(b"\r\n") == fi.by_name("fa_crlf")["data"].count(b"\n")
    assert not fi.by_name("fa_no_final_newline")["data"].endswith(b"\n") and fi.by_name("fa_no_final_newline_after_cr")["data"].endswith(b"\r")
    assert [len(s) for s in p["fa_no_final_newline_after_cr"]["seqs"]] == [70, 45] == [len(s) for s in p["fa_no_final_newline"]["seqs"]]
    assert p["fa_hdr5000"]["records"][0]["hdr_len"] == 5000 and p["fa_hdr5000"]["records"][0]["name_len"] == 4
    assert p["fa_lower"]["n_folded"] > 100 and p["fa_lower_keep"]["n_folded"] == 0 and p["fa_lower_keep"]["seqs"][0].islower()
    assert p["fa_lower"]["seqs"] == [s.upper() for s in p["fa_lower_keep"]["seqs"]]
    q = fi.by_name("fq_qual_at_plus")["data"]
    quals = [q[r["qual_off"]:r["qual_off"] + 1] for r in p["fq_qual_at_plus"]["records"]]
    assert quals == [b"@", b"+", b"@", b"@", b"+"]
    assert [r["seq_len"] for r in p["fq_empty_seq"]["records"]] == [0, 16, 0] == [r["seq_len"] for r in p["fq_empty_seq"]["records"]]
    assert [r["seq_len"] for r in p["fq_empty_seq_trailing_blanks"]["records"]] == [16, 0]
    assert p["empty"]["records"] == [] and p["blank_only"]["records"] == [] and p["blank_only"]["n_lines"] == 4


# ----------------------------------------------------------------------------- the C ABI without a device
def test_symbols_declared_exported_and_bound(lib):
    from pacbioassembly_amd import _lib
    from test_abi_symbols import declared_functions
    raw = C.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared_functions() and n in _lib.SYMBOLS and hasattr(raw, n), n
    assert (_lib.PBA_FX_AUTO, _lib.PBA_FX_FASTA, _lib.PBA_FX_FASTQ, _lib.PBA_FX_KEEP_CASE, _lib.PBA_FX_STRICT_ACGT) == (0, 1, 2, 1, 2)


def test_structs_as_the_header_lays_them_out(lib, tmp_path):
    from pacbioassembly_amd import _lib, engine
    src = tmp_path / "layout.cpp"
    fields = {"pba_fastx_rec": [n for n, _ in _lib.PbaFastxRec._fields_], "pba_fastx_stats": [n for n, _ in _lib.PbaFastxStats._fields_]}
    body = "".join('printf("%s %%zu", sizeof(%s));%s printf("\\n");\n' % (
        t, t, "".join(' printf(" %%zu", offsetof(%s, %s));' % (t, f) for f in fs)) for t, fs in fields.items())
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "pba.h"\nint main() {\n' + body +
                   'printf("%d %d %d %u %u\\n", PBA_FX_AUTO, PBA_FX_FASTA, PBA_FX_FASTQ, PBA_FX_KEEP_CASE, PBA_FX_STRICT_ACGT);\nreturn 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["g++", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, check=True).stdout.decode().splitlines()
    for line, cls in zip(out, (_lib.PbaFastxRec, _lib.PbaFastxStats)):
        got = [int(v) for v in line.split()[1:]]
        assert got == [C.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_], line
    assert out[2].split() == ["0", "1", "2", "1", "2"]
    assert [engine.FASTX_REC_DTYPE.fields[n][1] for n, _ in _lib.PbaFastxRec._fields_] == [getattr(_lib.PbaFastxRec, n).offset for n, _ in _lib.PbaFastxRec._fields_]


def test_null_arguments_refused_without_a_device(lib):
    from pacbioassembly_amd._lib import PBA_E_INVALID
    h, ih, cut, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(77), C.c_uint64(77)
    buf = np.frombuffer(b">a\nAC\n", np.uint8)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.pba_seqs_from_fastx(None, p, 6, 0, 0, C.byref(h), C.byref(ih), None) == PBA_E_INVALID and not h.value and not ih.value
    assert lib.pba_seqs_from_fastx_budget(None, p, 6, 0, 0, C.byref(h), None, None, 0) == PBA_E_INVALID
    assert lib.pba_seqs_write_fasta(None, None, 0, 0, None, None, 60, None, 0, C.byref(nb)) == PBA_E_INVALID
    assert lib.pba_fastx_index_count(None) == 0 and lib.pba_fastx_index_recs(None, None, 0) == PBA_E_INVALID
    lib.pba_fastx_index_destroy(None)
    assert lib.pba_fastx_sniff(None, 5) == PBA_E_INVALID and lib.pba_fastx_sniff(None, 0) == 0
    assert lib.pba_fastx_cut(p, 6, 1, 3, None) == PBA_E_INVALID and lib.pba_fastx_cut(None, 6, 1, 3, C.byref(cut)) == PBA_E_INVALID
    assert lib.pba_fastx_cut(p, 6, 3, 3, C.byref(cut)) == PBA_E_INVALID and cut.value == 77
    assert lib.pba_fastx_cut(None, 0, 0, 0, C.byref(cut)) == 0 and cut.value == 0


def test_sniff_of_every_case(lib):
    from pacbioassembly_amd import engine
    for c in fi.cases():
        want = fr.sniff(c["data"])[0]
        if want < 0:
            with pytest.raises(engine.PbaError):
                engine.fastx_sniff(c["data"])
        else:
            assert engine.fastx_sniff(c["data"]) == want, c["name"]
    assert engine.fastx_sniff(np.frombuffer(b"\r\n\n@x", np.uint8)) == fr.FASTQ
    with pytest.raises(engine.PbaError):                          # one "\r" only: the line "\r\r\n" has content
        engine.fastx_sniff(b"\r\r\n>a")


def test_cut_against_brute_force_at_every_want_of_every_case(lib):
    """pba_fastx_cut(want) is the largest record start p with 0 < p <= want, the length for want >= length, 0 if there is none"""
    cut = C.c_uint64()
    ref = C.byref(cut)
    fn = lib.pba_fastx_cut
    n_cut_inside = 0
    for c in fi.cases():
        data = c["data"]
        buf = np.frombuffer(data, np.uint8)
        p = C.c_void_p(buf.ctypes.data) if len(data) else None
        if rules_of(c) is None:                                   # AUTO on a file that is neither
            assert fn(p, len(data), c["format"], 1, ref) == -1, c["name"]
            formats = [(fr.FASTA, fr.FASTA), (fr.FASTQ, fr.FASTQ)]
        else:
            formats = [(c["format"], rules_of(c))]
            if len(data) < 3000:                                  # ... and both forced formats on the short ones
                formats += [(fr.FASTA, fr.FASTA), (fr.FASTQ, fr.FASTQ)]
        for fmt, rules in formats:
            want_all = fr.cut_brute(data, rules)
            got = []
            for want in range(len(data) + 2):
                assert fn(p, len(data), fmt, want, ref) == 0
                got.append(cut.value)
            assert got == want_all, (c["name"], fmt, next(k for k in range(len(got)) if got[k] != want_all[k]))
            n_cut_inside += len(set(want_all)) > 2
    assert n_cut_inside >= 40
    # a quality line that starts with '@' is no record start, whatever follows two lines below it ... unless a sequence starts with '+'
    d = b"@a\nAC\n+\n@I\n@b\nGG\n+\nII\n"
    assert fr.record_starts(d, fr.FASTQ) == [0, 11] and fr.cut_brute(d, fr.FASTQ)[10:13] == [0, 11, 11]


# ----------------------------------------------------------------------------- fastx_lines.h as a host program
@pytest.fixture(scope="module")
def host_answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("fastx")
    exe = str(d / "fastx_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pacbioassembly_amd", "csrc"),
           os.path.join(HERE, "cpp", "fastx_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    cs = fi.cases()
    with open(d / "cases.bin", "wb") as f:
        for c in cs:
            f.write(struct.pack("<IIQ", c["format"], int(c["keep"]), len(c["data"])) + c["data"])
    p = subprocess.run([exe, str(d / "cases.bin")], capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode(errors="replace")[-4000:]
    lines, out, at = p.stdout.decode().splitlines(), [], 0
    for c in cs:
        head = lines[at].split()
        at += 1
        if head[0] == "error":
            out.append(("error", int(head[1])))
            continue
        n = int(head[2])
        out.append((tuple(int(v) for v in head[1:]), [ln.split() for ln in lines[at:at + n]]))
        at += n
    assert at == len(lines)
    return cs, out


def test_host_program_equals_the_restatement(host_answers):
    for c, got in zip(*host_answers):
        want = fr.parse(c["data"], c["format"], c["keep"])
        if isinstance(want, tuple):
            assert got == want, c["name"]
            continue
        assert got[0] == (want["format"], len(want["records"]), want["n_lines"], want["n_folded"]), c["name"]
        for r, s, ln in zip(want["records"], want["seqs"], got[1]):
            assert [int(v) for v in ln[:7]] == [r[k] for k in fr.REC_FIELDS], (c["name"], r)
            assert (b"" if ln[7] == "-" else bytes.fromhex(ln[7])) == s, (c["name"], r["name"])


# ----------------------------------------------------------------------------- the example
def test_example_builds_against_the_c_abi_and_stops_without_a_device(lib, tmp_path):
    import torch
    libdir = os.path.join(ROOT, "pacbioassembly_amd", "lib")
    exe = str(tmp_path / "map_fastx_gpu")
    subprocess.run(["g++", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "examples", "map_fastx_gpu.cpp"), "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}"], check=True)
    r = subprocess.run([exe], capture_output=True)
    assert r.returncode != 0 and b"usage" in r.stderr
    if torch.cuda.is_available():
        return
    (tmp_path / "c.fa").write_bytes(b">c0\n" + b"ACGT" * 100 + b"\n")
    (tmp_path / "r.fq").write_bytes(b"@r0\nACGT\n+\nIIII\n")
    r = subprocess.run([exe, str(tmp_path / "c.fa"), str(tmp_path / "r.fq"), "111*11*11*1*1111"], capture_output=True)
    assert r.returncode != 0 and r.stdout == b"" and b"device" in r.stderr.lower()
