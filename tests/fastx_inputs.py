"""The named FASTA / FASTQ inputs of test_fastx_cpu.py (the rules against hand-written expectations, the stand-alone host
program, pba_fastx_cut against brute force) and test_gpu_fastx.py (pba_seqs_from_fastx against the restatement).  Built once.

A case: {"name", "data", "format" (what the caller passes), "keep" (PBA_FX_KEEP_CASE), "ok"}.  The line kernels work in tiles
of 4 096 bytes and lanes of 16: the widths and the "\\r" | "\\n" splits sweep 2^6 .. 2^14 around both."""
import functools

import numpy as np

AUTO, FASTA, FASTQ = 0, 1, 2
WIDTHS = [1, 15, 16, 17, 60] + [w for k in range(6, 15) for w in (2 ** k - 1, 2 ** k, 2 ** k + 1)]
LENGTHS = [0, 1, 15, 16, 17, 2047, 2048, 2049]


def rnd(rs, n, alphabet=b"ACGT"):
    return bytes(np.frombuffer(alphabet, np.uint8)[rs.randint(0, len(alphabet), n)])


def fasta(recs, width=60, eol=b"\n", final=True):
    out = []
    for h, s in recs:
        out.append(b">" + h)
        out += [s[k:k + width] for k in range(0, len(s), width)] if width else ([s] if s else [])
    data = eol.join(out) + eol
    return data if final else data[:-len(eol)]


def fastq(recs, eol=b"\n", final=True):
    data = b"".join(b"@" + h + eol + s + eol + p + eol + q + eol for h, s, p, q in recs)
    return data if final else data[:-len(eol)]


def qual(rs, n, first=None):
    q = rnd(rs, n, b"!#+5:@FIJ~")
    return (first + q[1:]) if first and n else q


@functools.lru_cache(maxsize=None)
def cases():
    rs = np.random.RandomState(4011)
    out = []

    def add(name, data, format=AUTO, keep=False, ok=True):
        out.append({"name": name, "data": bytes(data), "format": format, "keep": keep, "ok": ok})

    # ---- FASTA that must parse
    for w in WIDTHS:
        add(f"fa_wrap{w}", fasta([(b"a x", rnd(rs, 2 * w + 3)), (b"b", rnd(rs, w)), (b"c", rnd(rs, min(w, 7)))], w))
    add("fa_line70000", fasta([(b"long one", rnd(rs, 70000))], 0))
    add("fa_lengths_w60", fasta([(b"L%d" % n, rnd(rs, n)) for n in LENGTHS], 60))
    add("fa_lengths_oneline", fasta([(b"L%d" % n, rnd(rs, n)) for n in LENGTHS], 0))
    add("fa_1rec", fasta([(b"only", rnd(rs, 100))]))
    add("fa_2rec", fasta([(b"one", rnd(rs, 61)), (b"two", rnd(rs, 59))]))
    add("fa_300rec", fasta([(b"r%d len=%d" % (i, 20 + 7 * (i % 41)), rnd(rs, 20 + 7 * (i % 41))) for i in range(300)], 50))
    add("fa_crlf", fasta([(b"a desc", rnd(rs, 130)), (b"b", b""), (b"c", rnd(rs, 60))], 60, b"\r\n"))
    for k in range(6, 15):                                        # the "\r" is byte 2^k - 1, its "\n" byte 2^k
        add(f"fa_cr_split{k}", fasta([(b"h" * (2 ** k - 24), rnd(rs, 70)), (b"t", rnd(rs, 33))], 20, b"\r\n"))
    add("fa_no_final_newline", fasta([(b"a", rnd(rs, 70)), (b"b", rnd(rs, 45))], 60, final=False))
    add("fa_no_final_newline_after_cr", fasta([(b"a", rnd(rs, 70)), (b"b", rnd(rs, 45))], 60, b"\r\n")[:-1])
    add("fa_blank_lines", b"\n\r\n>a\n\nACGT\n\n\nGGA\n\n>b\n\r\n\nTT\n\n\n")
    add("fa_hdr_hdr", b">a\n>b\nACGT\n>c\n>d\n")
    add("fa_hdr_at_eof", b">a\nACGT\n>b")
    add("fa_hdr_only", b">lonely header\n")
    add("fa_hdr_then_blank", b">a\n\n\n")
    add("empty", b"")
    add("blank_only", b"\n\n\r\n\n")
    add("fa_hdr5000", fasta([(b"name " + rnd(rs, 4995, b"abc >@+\t"), rnd(rs, 100)), (b"n2\tcomment", rnd(rs, 10))]))
    add("fa_gt_inside", b">a>b >c\nAC>GT\nA>\n>d\nAA\n")
    low = fasta([(b"a", rnd(rs, 100, b"acgt")), (b"b", rnd(rs, 77, b"ACGTacgtNn"))], 30)
    add("fa_lower", low)
    add("fa_lower_keep", low, keep=True)
    add("fa_N_and_space", b">a\nACGNNT A\nAC\tG\n>b\nNNNN\n")
    add("fa_forced", fasta([(b"a", rnd(rs, 100))]), format=FASTA)
    add("fa_zero_inside", fasta([(b"s0", rnd(rs, 5)), (b"z1", b""), (b"s2", rnd(rs, 61)), (b"s3", rnd(rs, 120)), (b"z4", b""), (b"s5", rnd(rs, 7))]))
    add("fa_at_header_forced", b">a\n@CGT\n+\n", format=FASTA)      # '@' and '+' lines are sequence lines of a FASTA record
    # ---- FASTQ that must parse
    s = [rnd(rs, n) for n in (40, 1, 16, 17, 300)]
    add("fq_plain", fastq([(b"r%d" % i, x, b"+", qual(rs, len(x))) for i, x in enumerate(s)]))
    add("fq_qual_at_plus", fastq([(b"r0", s[0], b"+", qual(rs, 40, b"@")), (b"r1", s[4], b"+", qual(rs, 300, b"+")),
                                  (b"r2 x", s[2], b"+r2 x", qual(rs, 16, b"@")), (b"r3", s[1], b"+", b"@"), (b"r4", s[3], b"+", qual(rs, 17, b"+"))]))
    add("fq_plus_name", fastq([(b"r0 d", s[0], b"+r0 d", qual(rs, 40)), (b"r1", s[3], b"+anything at all", qual(rs, 17))]))
    add("fq_empty_seq", fastq([(b"e0", b"", b"+", b""), (b"r1", s[2], b"+", qual(rs, 16)), (b"e2", b"", b"+", b"")]))
    add("fq_empty_seq_trailing_blanks", fastq([(b"r1", s[2], b"+", qual(rs, 16)), (b"e2", b"", b"+", b"")]) + b"\n\r\n\n")
    add("fq_crlf", fastq([(b"r%d" % i, x, b"+", qual(rs, len(x))) for i, x in enumerate(s)], b"\r\n"))
    add("fq_no_final_newline", fastq([(b"r0", s[0], b"+", qual(rs, 40))], final=False))
    add("fq_no_final_newline_after_cr", fastq([(b"r0", s[0], b"+", qual(rs, 40))], b"\r\n")[:-1])
    add("fq_trailing_blanks", fastq([(b"r0", s[0], b"+", qual(rs, 40))]) + b"\n\n")
    low = fastq([(b"r0", rnd(rs, 50, b"acgtN"), b"+", qual(rs, 50))])
    add("fq_lower", low)
    add("fq_lower_keep", low, keep=True)
    add("fq_300rec", fastq([(b"q%d" % i, x, b"+", qual(rs, len(x), b"@" if i % 3 == 0 else b"+" if i % 3 == 1 else None))
                            for i in range(300) for x in [rnd(rs, 10 + 13 * (i % 29))]]))
    add("fq_line70000", fastq([(b"long", x, b"+", qual(rs, 70000)) for x in [rnd(rs, 70000)]]))
    add("fq_forced", fastq([(b"r0", s[0], b"+", qual(rs, 40))]), format=FASTQ)
    add("blank_only_forced_fastq", b"\n\r\n", format=FASTQ)
    # ---- must fail
    add("bad_fa_text_before_header", b"\nACGT\n>a\nAC\n", format=FASTA, ok=False)
    add("bad_auto_first_byte", b"\n\nACGT\n>a\nAC\n", ok=False)
    add("bad_fq_missing_plus", b"@a\nACGT\nIIII\n@b\nAC\n+\nII\n", ok=False)
    add("bad_fq_qual_short", b"@a\nACGT\n+\nIIII\n@b\nACG\n+\nII\n", ok=False)
    add("bad_fq_qual_long", b"@a\nACGT\n+\nIIIII\n@b\nACG\n+\nIII\n", ok=False)
    add("bad_fq_three_line_last", b"@a\nACGT\n+\nIIII\n@b\nACG\n+\n", ok=False)
    add("bad_fq_three_line_last_no_newline", b"@a\nACGT\n+\nIIII\n@b\nACG\n+", ok=False)
    add("bad_fq_header_only_last", b"@a\nACGT\n+\nIIII\n@b\n\n\n", ok=False)
    add("bad_fq_blank_inside", b"@a\nACGT\n\n+\nIIII\n", ok=False)
    add("bad_fq_blank_between", b"@a\nACGT\n+\nIIII\n\n@b\nAC\n+\nII\n", ok=False)
    add("bad_fq_two_line_seq", b"@a\nACGT\nACGT\n+\nIIIIIIII\n", ok=False)
    add("bad_fq_leading_blank", b"\n@a\nACGT\n+\nIIII\n", ok=False)
    add("bad_forced_fasta_on_fastq", fastq([(b"r0", s[0], b"+", qual(rs, 40))]), format=FASTA, ok=False)
    add("bad_forced_fastq_on_fasta", fasta([(b"a", rnd(rs, 100))]), format=FASTQ, ok=False)
    add("bad_fq_late", fastq([(b"q%d" % i, s[0], b"+", qual(rs, 40)) for i in range(150)]) + b"@z\nACGT\n+\nIII\n", ok=False)
    # ---- one record wrapped at width 1: 8 192 and 8 193 lines, either side of the one-workgroup scan of the per-line counts
    # (PBA_SCAN_SMALL_MAX); a generator of their own, so that the cases above keep their bytes
    rs2 = np.random.RandomState(4012)
    for n_lines in (8192, 8193):
        add(f"fa_lines{n_lines}", fasta([(b"one per line", rnd(rs2, n_lines - 1))], 1))
    assert len({c["name"] for c in out}) == len(out)
    return out


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


# what the lines say, written down by hand: name -> (format, [(name, sequence)]) or ("error", line)
HAND = {
    "fa_blank_lines": (FASTA, [(b"a", b"ACGTGGA"), (b"b", b"TT")]),
    "fa_hdr_hdr": (FASTA, [(b"a", b""), (b"b", b"ACGT"), (b"c", b""), (b"d", b"")]),
    "fa_hdr_at_eof": (FASTA, [(b"a", b"ACGT"), (b"b", b"")]),
    "fa_hdr_only": (FASTA, [(b"lonely", b"")]),
    "empty": (0, []),
    "blank_only": (0, []),
    "fa_gt_inside": (FASTA, [(b"a>b", b"AC>GTA>"), (b"d", b"AA")]),
    "fa_N_and_space": (FASTA, [(b"a", b"ACGNNT AAC\tG"), (b"b", b"NNNN")]),
    "fa_at_header_forced": (FASTA, [(b"a", b"@CGT+")]),
    "bad_fa_text_before_header": ("error", 2),
    "bad_auto_first_byte": ("error", 3),
    "bad_fq_missing_plus": ("error", 3),
    "bad_fq_qual_short": ("error", 8),
    "bad_fq_qual_long": ("error", 4),
    "bad_fq_three_line_last": ("error", 8),
    "bad_fq_three_line_last_no_newline": ("error", 8),
    "bad_fq_header_only_last": ("error", 6),
    "bad_fq_blank_inside": ("error", 3),
    "bad_fq_blank_between": ("error", 5),
    "bad_fq_two_line_seq": ("error", 3),
    "bad_fq_leading_blank": ("error", 1),
    "bad_forced_fasta_on_fastq": ("error", 1),
    "bad_forced_fastq_on_fasta": ("error", 1),
    "bad_fq_late": ("error", 604),
}
