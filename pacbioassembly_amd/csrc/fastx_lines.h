// fastx_lines.h -- the rules of FASTA / FASTQ as arithmetic over a table of line starts: what a line's content
// is, what kind of line it is, which line offends, what a record's fields are, where a file may be cut (pba_fastx_cut) and
// what format it is (pba_fastx_sniff).  The kernels of pba_fastx.hip run these per line and per record; a host program can
// compile the file alone (tests/cpp/fastx_main.cpp does, serially, against tests/fastx_ref.py).
//   line L of an image of n bytes is bytes [start[L], start[L + 1]): its '\n' included where it has one, start[n_lines] = n.
//   A last line without '\n' is a line; an image that ends in '\n' has no line behind it.
//   content: the line without its '\n' and without ONE '\r' directly in front of it (or at the very end of the image).
//   blank: content of length 0.
#ifndef PBA_FASTX_LINES_H
#define PBA_FASTX_LINES_H

#include <stdint.h>

#if defined(__HIPCC__)
#define FX_HD __host__ __device__ static inline
#else
#define FX_HD static inline
#endif

enum { FX_AUTO = 0, FX_FASTA = 1, FX_FASTQ = 2 };            // = PBA_FX_* (include/pba.h)
enum { FX_BLANK = 0, FX_HEADER = 1, FX_SEQ = 2 };              // what a line of a FASTA file is
#define FX_NO_LINE 0xFFFFFFFFu                                 // "no offending line" of the atomicMin word

// content length of the line [s, e)
FX_HD uint32_t fx_content_len(const uint8_t *f, uint64_t s, uint64_t e) {
    if (e > s && f[e - 1] == '\n') --e;
    if (e > s && f[e - 1] == '\r') --e;
    return (uint32_t)(e - s);
}

// FASTA: a '>' at the first byte is a header, every other non-blank line a sequence line
FX_HD int fx_fasta_kind(const uint8_t *f, uint64_t s, uint32_t clen) { return clen == 0 ? FX_BLANK : f[s] == '>' ? FX_HEADER : FX_SEQ; }
// ... and a sequence line in front of the first header (hdr_before = headers on earlier lines) offends
FX_HD bool fx_fasta_bad(int kind, uint32_t hdr_before) { return kind == FX_SEQ && hdr_before == 0; }

// FASTQ: the lines that belong to records, given the line behind the last non-blank one (last_nb1 = its index + 1, 0 = none)
// and whether blank lines may trail (the last piece of a file): blank lines behind the last record do not count -- but the
// blank line straight behind a '+' line is that record's empty quality.
FX_HD uint32_t fx_fastq_neff(uint32_t last_nb1, uint32_t n_lines, bool trailing_ok) {
    if (!trailing_ok) return n_lines;
    if ((last_nb1 & 3u) == 3u && last_nb1 < n_lines) return last_nb1 + 1;
    return last_nb1;
}
// the verdict on line L < n_eff (phase = L & 3): first = the first content byte (unread where clen == 0), seq_clen = the
// content length of line L - 2 (phase 3 only)
FX_HD bool fx_fastq_bad(uint32_t phase, uint32_t clen, uint8_t first, uint32_t seq_clen) {
    if (phase == 0) return clen == 0 || first != '@';
    if (phase == 2) return clen == 0 || first != '+';
    if (phase == 3) return clen != seq_clen;
    return false;
}
// n_eff lines make n_eff / 4 records; a remainder is a truncated record, and the line that is missing offends
FX_HD uint32_t fx_fastq_truncated(uint32_t n_eff) { return (n_eff & 3u) ? n_eff : FX_NO_LINE; }

// a header's first token: content after the marker up to the first space or tab
FX_HD uint32_t fx_name_len(const uint8_t *f, uint64_t s, uint32_t hdr_len) {
    uint32_t k = 0;
    while (k < hdr_len && f[s + 1 + k] != ' ' && f[s + 1 + k] != '\t') ++k;
    return k;
}

// One record's fields, offsets relative to the image (the driver adds the piece's base).  start: the line table.
struct FxRec { uint64_t hdr_off, seq_off, qual_off; uint32_t hdr_len, name_len, seq_len, n_seq_lines; };
// FASTA: the record whose header is line h, the next header (or n_lines) line hn; seq_len / n_seq_lines come from the scans
FX_HD FxRec fx_fasta_rec(const uint8_t *f, const uint32_t *start, uint32_t h, uint32_t hn, uint32_t seq_len, uint32_t n_seq_lines) {
    FxRec r;
    r.hdr_off = start[h];
    r.hdr_len = fx_content_len(f, start[h], start[h + 1]) - 1;
    r.name_len = fx_name_len(f, start[h], r.hdr_len);
    uint32_t l = h + 1;
    while (l < hn && fx_content_len(f, start[l], start[l + 1]) == 0) ++l;
    r.seq_off = l < hn ? start[l] : start[h + 1];
    r.qual_off = 0;
    r.seq_len = seq_len; r.n_seq_lines = n_seq_lines;
    return r;
}
// FASTQ: record k is lines 4k .. 4k + 3
FX_HD FxRec fx_fastq_rec(const uint8_t *f, const uint32_t *start, uint32_t k) {
    FxRec r;
    const uint32_t h = 4 * k;
    r.hdr_off = start[h];
    const uint32_t c = fx_content_len(f, start[h], start[h + 1]);
    r.hdr_len = c ? c - 1 : 0;
    r.name_len = fx_name_len(f, start[h], r.hdr_len);
    r.seq_off = start[h + 1];
    r.qual_off = start[h + 3];
    r.seq_len = fx_content_len(f, start[h + 1], start[h + 2]);
    r.n_seq_lines = 1;
    return r;
}

// upper case of a sequence byte
FX_HD uint8_t fx_fold(uint8_t c, bool keep, uint32_t *n_folded) {
    if (!keep && c >= 'a' && c <= 'z') { ++*n_folded; return (uint8_t)(c - 32); }
    return c;
}

// pba_fastx_sniff: the first byte of the first non-blank line -- FX_FASTA, FX_FASTQ, 0 for no such line, -1 for another byte
// (at, line: nullable -- where that line starts and its 0-based number; n and the line count where there is none)
FX_HD int fx_sniff(const uint8_t *f, uint64_t n, uint64_t *at = nullptr, uint64_t *line = nullptr) {
    uint64_t s = 0, l = 0;
    int got = 0;
    while (s < n) {
        uint64_t e = s;
        while (e < n && f[e] != '\n') ++e;
        if (e < n) ++e;
        if (fx_content_len(f, s, e)) { got = f[s] == '>' ? FX_FASTA : f[s] == '@' ? FX_FASTQ : -1; break; }
        s = e; ++l;
    }
    if (at) *at = s;
    if (line) *line = l;
    return got;
}

// is p (0 < p < n, a line start) a record start?
FX_HD bool fx_record_start(const uint8_t *f, uint64_t n, int format, uint64_t p) {
    if (format == FX_FASTA) return f[p] == '>';
    if (f[p] != '@') return false;
    uint64_t q = p;
    for (int k = 0; k < 2; ++k) {                              // the start of the line after next
        while (q < n && f[q] != '\n') ++q;
        if (q == n) return false;
        ++q;
    }
    return q < n && f[q] == '+';
}
// pba_fastx_cut: the largest record start p with 0 < p <= want; n if want >= n; 0 if there is none.  FASTQ: a line start
// holding '@' whose line after next exists and starts with '+' -- exact for files whose sequence lines do not begin with '+'
// (a quality line may begin with '@' or '+': the line two below it is the next record's sequence line).
FX_HD uint64_t fx_cut(const uint8_t *f, uint64_t n, int format, uint64_t want) {
    if (want >= n) return n;
    for (uint64_t p = want; p > 0; --p)
        if (f[p - 1] == '\n' && fx_record_start(f, n, format, p)) return p;
    return 0;
}

#endif
