// fastx_main.cpp -- csrc/fastx_lines.h alone, as a host program: the line and record rules that the kernels of pba_fastx.hip run
// per line and per record, run serially here over a line table built byte by byte (tests/test_fastx_cpu.py, under ASan + UBSan
// where the compiler has the runtimes).
//   fastx_main cases.bin      cases.bin: per case [u32 format][u32 keep][u64 n][n bytes]
// prints per case   "error <line>"   or   "ok <format> <n_records> <n_lines> <n_folded>" followed by one line per record:
//   hdr_off seq_off qual_off hdr_len name_len seq_len n_seq_lines <sequence as hex, "-" if empty>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fastx_lines.h"

static void run(const uint8_t *f, uint64_t n, int format, bool keep) {
    int fmt = format;
    if (fmt == FX_AUTO) {
        uint64_t line = 0;
        fmt = fx_sniff(f, n, nullptr, &line);
        if (fmt < 0) { printf("error %llu\n", (unsigned long long)(line + 1)); return; }
    }
    const int rules = fmt ? fmt : FX_FASTA;
    std::vector<uint32_t> start(1, 0);
    for (uint64_t k = 0; k < n; ++k)
        if (f[k] == '\n') start.push_back((uint32_t)(k + 1));
    if (n && f[n - 1] != '\n') start.push_back((uint32_t)n);
    const uint32_t n_lines = (uint32_t)start.size() - 1;
    // per line, then the scans (x1[L]: what lies in front of line L)
    std::vector<uint32_t> hdr1(n_lines + 1, 0), sq1(n_lines + 1, 0), by1(n_lines + 1, 0);
    uint32_t last_nb1 = 0;
    for (uint32_t L = 0; L < n_lines; ++L) {
        const uint32_t clen = fx_content_len(f, start[L], start[L + 1]);
        uint32_t h = 0, s = 0, b = 0;
        if (rules == FX_FASTA) {
            const int kind = fx_fasta_kind(f, start[L], clen);
            h = kind == FX_HEADER; s = kind == FX_SEQ; b = kind == FX_SEQ ? clen : 0;
        } else
            b = (L & 3u) == 1u ? clen : 0;
        hdr1[L + 1] = hdr1[L] + h; sq1[L + 1] = sq1[L] + s; by1[L + 1] = by1[L] + b;
        if (clen) last_nb1 = L + 1;
    }
    const uint32_t n_eff = rules == FX_FASTQ ? fx_fastq_neff(last_nb1, n_lines, true) : n_lines;
    const uint32_t n_rec = rules == FX_FASTQ ? n_eff / 4 : hdr1[n_lines];
    uint32_t bad = rules == FX_FASTQ ? fx_fastq_truncated(n_eff) : FX_NO_LINE;
    std::vector<uint32_t> rec_line(n_rec + 1, n_lines);
    for (uint32_t L = 0; L < n_lines; ++L) {
        const uint32_t s = start[L], clen = fx_content_len(f, s, start[L + 1]);
        bool is_bad = false;
        if (rules == FX_FASTA) {
            const int kind = fx_fasta_kind(f, s, clen);
            is_bad = fx_fasta_bad(kind, hdr1[L]);
            if (kind == FX_HEADER) rec_line[hdr1[L]] = L;
        } else if (L < n_eff) {
            const uint32_t seq_clen = (L & 3u) == 3u ? fx_content_len(f, start[L - 2], start[L - 1]) : 0u;
            is_bad = fx_fastq_bad(L & 3u, clen, clen ? f[s] : (uint8_t)0, seq_clen);
        }
        if (is_bad && L < bad) bad = L;
    }
    if (bad != FX_NO_LINE) { printf("error %u\n", bad + 1); return; }
    // the bases, line by line
    std::vector<uint8_t> text(by1[n_lines]);
    uint32_t n_folded = 0;
    for (uint32_t L = 0; L < n_lines; ++L)
        for (uint32_t k = 0; k < by1[L + 1] - by1[L]; ++k) text[by1[L] + k] = fx_fold(f[start[L] + k], keep, &n_folded);
    printf("ok %d %u %u %u\n", fmt, n_rec, n_lines, n_folded);
    for (uint32_t r = 0; r < n_rec; ++r) {
        FxRec x;
        uint32_t h;
        if (rules == FX_FASTA) {
            h = rec_line[r];
            const uint32_t hn = rec_line[r + 1];
            x = fx_fasta_rec(f, start.data(), h, hn, by1[hn] - by1[h], sq1[hn] - sq1[h]);
        } else {
            h = 4 * r;
            x = fx_fastq_rec(f, start.data(), r);
        }
        printf("%llu %llu %llu %u %u %u %u ", (unsigned long long)x.hdr_off, (unsigned long long)x.seq_off, (unsigned long long)x.qual_off,
               x.hdr_len, x.name_len, x.seq_len, x.n_seq_lines);
        if (!x.seq_len) printf("-");
        for (uint32_t k = 0; k < x.seq_len; ++k) printf("%02x", text[by1[h] + k]);
        printf("\n");
    }
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: fastx_main cases.bin\n"); return 2; }
    FILE *fp = fopen(argv[1], "rb");
    if (!fp) { perror(argv[1]); return 2; }
    for (;;) {
        uint32_t head[2];
        uint64_t n;
        if (fread(head, 4, 2, fp) != 2) break;
        if (fread(&n, 8, 1, fp) != 1) return 3;
        std::vector<uint8_t> buf(n);                              // exactly n bytes: a read past the image is the sanitizer's to find
        if (n && fread(buf.data(), 1, n, fp) != n) return 3;
        run(buf.data(), n, (int)head[0], head[1] != 0);
    }
    fclose(fp);
    return 0;
}
