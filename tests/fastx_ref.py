"""The rules of FASTA / FASTQ input restated in plain Python, line by line, for the tests of pba_seqs_from_fastx.

Lines end at "\\n"; one "\\r" directly in front of it -- or at the very end of a file without a final "\\n" -- is not content; a
line without content is blank.  A last line without "\\n" is a line; a file that ends in "\\n" has no line behind it.

parse(data, format, keep_case) returns
    {"format", "records": [dict per record], "seqs": [bytes], "n_lines", "n_folded"}     or     ("error", 1-based line)
FASTQ: the lines that count are those up to the last non-blank one, and the blank line straight behind it when that last
non-blank line is a record's third ("+") line: the empty quality of an empty sequence.  Their number must be a multiple of
four, else the first line that is missing offends.
"""
AUTO, FASTA, FASTQ = 0, 1, 2
REC_FIELDS = ("hdr_off", "seq_off", "qual_off", "hdr_len", "name_len", "seq_len", "n_seq_lines")


def lines_of(data: bytes):
    """[(start, content)] of every line"""
    out, pos = [], 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl
        content = data[pos:end]
        if content.endswith(b"\r"):
            content = content[:-1]
        out.append((pos, content))
        pos = end + 1
    return out


def sniff(data: bytes):
    """(format, 0-based line of the first non-blank line): FASTA / FASTQ, 0 for no such line, -1 for another first byte"""
    for k, (_, c) in enumerate(lines_of(data)):
        if c:
            return {b">": FASTA, b"@": FASTQ}.get(c[:1], -1), k
    return 0, None


def fold(seq: bytes, keep_case: bool):
    if keep_case:
        return seq, 0
    return seq.upper(), sum(1 for ch in seq if 97 <= ch <= 122)


def _name_len(hdr: bytes) -> int:
    k = 0
    while k < len(hdr) and hdr[k:k + 1] not in (b" ", b"\t"):
        k += 1
    return k


def parse(data: bytes, format: int = AUTO, keep_case: bool = False):
    lines = lines_of(data)
    fmt = format
    if fmt == AUTO:
        fmt, at = sniff(data)
        if fmt < 0:
            return ("error", at + 1)
    recs, seqs, n_folded = [], [], 0
    if fmt == FASTQ:
        last = max([k for k, (_, c) in enumerate(lines) if c], default=-1)
        n_eff = last + 1
        if last % 4 == 2 and last + 1 < len(lines):
            n_eff = last + 2
        for k in range(n_eff):
            s, c = lines[k]
            if k % 4 == 0 and c[:1] != b"@":
                return ("error", k + 1)
            if k % 4 == 2 and c[:1] != b"+":
                return ("error", k + 1)
            if k % 4 == 3:
                if len(c) != len(lines[k - 2][1]):
                    return ("error", k + 1)
                hs, hc = lines[k - 3]
                seq, nf = fold(lines[k - 2][1], keep_case)
                n_folded += nf
                seqs.append(seq)
                recs.append(dict(hdr_off=hs, seq_off=lines[k - 2][0], qual_off=s, hdr_len=len(hc) - 1, name_len=_name_len(hc[1:]),
                                 seq_len=len(seq), n_seq_lines=1, name=hc[1:1 + _name_len(hc[1:])]))
        if n_eff % 4:
            return ("error", n_eff + 1)
    else:                                                         # FASTA, and the file without a non-blank line
        cur = None
        for k, (s, c) in enumerate(lines):
            if not c:
                continue
            if c[:1] == b">":
                end = data.find(b"\n", s)
                cur = dict(hdr_off=s, seq_off=len(data) if end < 0 else end + 1, qual_off=0, hdr_len=len(c) - 1, name_len=_name_len(c[1:]),
                           seq_len=0, n_seq_lines=0, name=c[1:1 + _name_len(c[1:])])
                recs.append(cur)
                seqs.append(b"")
            elif cur is None:
                return ("error", k + 1)
            else:
                if cur["n_seq_lines"] == 0:
                    cur["seq_off"] = s
                seq, nf = fold(c, keep_case)
                n_folded += nf
                seqs[-1] += seq
                cur["seq_len"] += len(seq)
                cur["n_seq_lines"] += 1
    return {"format": fmt, "records": recs, "seqs": seqs, "n_lines": len(lines), "n_folded": n_folded}


def record_starts(data: bytes, fmt: int):
    """where pba_fastx_cut may cut: FASTA a line start holding '>'; FASTQ a line start holding '@' whose line after next exists
    and starts with '+'"""
    starts = [0] + [k + 1 for k in range(len(data)) if data[k:k + 1] == b"\n" and k + 1 < len(data)]
    out = []
    for i, p in enumerate(starts):
        if fmt == FASTQ:
            ok = data[p:p + 1] == b"@" and i + 2 < len(starts) and data[starts[i + 2]:starts[i + 2] + 1] == b"+"
        else:
            ok = data[p:p + 1] == b">"
        if ok:
            out.append(p)
    return out


def cut_brute(data: bytes, fmt: int):
    """pba_fastx_cut at every want in 0 .. len(data) + 1"""
    n, out, best, it = len(data), [], 0, 0
    rs = [p for p in record_starts(data, fmt) if p > 0]
    for want in range(n + 2):
        while it < len(rs) and rs[it] <= want:
            best = rs[it]
            it += 1
        out.append(n if want >= n else best)
    return out


def format_fasta(names, seqs, width: int) -> bytes:
    out = []
    for nm, s in zip(names, seqs):
        out.append(b">" + nm + b"\n")
        if width == 0:
            if s:
                out.append(s + b"\n")
        else:
            out += [s[k:k + width] + b"\n" for k in range(0, len(s), width)]
    return b"".join(out)
