// map_paf_gpu.cpp -- map reads onto a set of contigs on both strands and print how each one aligns, as PAF with a cg:Z: tag:
//   map_paf_gpu contig_file seed [R] [strands] < seq_file
// contig_file holds one contig per line (an empty line is an empty contig); every whitespace-separated token of stdin is a
// read.  The reads are mapped (pba_map_reads), the found rows are re-run on the device with their paths run-length encoded
// on the way out (pba_map_rows_cigar), and one PAF line per found read goes to stdout: the twelve columns (the read is the
// query, named read<i>; the contig the target, named contig<c>; matching bases; alignment block length; mapping quality
// 255), NM:i:<edit distance> and cg:Z:<CIGAR over = X I D>.
//
//   g++ -O2 -I include -o map_paf_gpu examples/map_paf_gpu.cpp -L pacbioassembly_amd/lib -lpba -Wl,-rpath,$PWD/pacbioassembly_amd/lib
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pba.h"

static void die(pba_ctx *ctx, const char *what, int st) {
    fprintf(stderr, "%s: %s (%s)\n", what, pba_strerror(st), ctx ? pba_ctx_error(ctx) : "");
    exit(EXIT_FAILURE);
}

int main(int argc, char *argv[]) {
    if (argc <= 2) {
        fprintf(stderr, "usage: map_paf_gpu contig_file seed [R] [strands] < seq_file\n");
        return EXIT_FAILURE;
    }
    const double R = argc > 3 ? atof(argv[3]) : 0.15;
    const int strands = argc > 4 ? atoi(argv[4]) : 3;
    FILE *fp = fopen(argv[1], "r");
    if (!fp) { perror(argv[1]); return EXIT_FAILURE; }
    std::string text;                                                 // the contigs back to back
    std::vector<uint64_t> toff(1, 0);
    bool open_line = false;
    for (int ch; (ch = fgetc(fp)) != EOF;) {
        if (ch == '\r') continue;
        if (ch == '\n') { toff.push_back(text.size()); open_line = false; }
        else { text.push_back((char)ch); open_line = true; }
    }
    if (open_line) toff.push_back(text.size());
    fclose(fp);
    std::string reads, tok;                                           // the reads back to back
    std::vector<uint64_t> roff(1, 0);
    for (int ch; (ch = getchar()) != EOF;) {
        if (ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r') {
            if (!tok.empty()) { reads += tok; roff.push_back(reads.size()); tok.clear(); }
        } else tok.push_back((char)ch);
    }
    if (!tok.empty()) { reads += tok; roff.push_back(reads.size()); }
    const uint32_t n = (uint32_t)(roff.size() - 1);

    pba_ctx *ctx = NULL;
    int st = pba_ctx_create(0, &ctx);
    if (st != PBA_OK) die(NULL, "pba_ctx_create", st);
    pba_seqs *T = NULL, *Rd = NULL, *Rc = NULL;
    pba_index *ix = NULL;
    if ((st = pba_seqs_from_text(ctx, text.data(), toff.data(), (uint32_t)(toff.size() - 1), 0, &T)) != PBA_OK) die(ctx, "contigs", st);
    if ((st = pba_seqs_from_text(ctx, reads.data(), roff.data(), n, 0, &Rd)) != PBA_OK) die(ctx, "reads", st);
    if ((st = pba_seqs_revcomp(ctx, Rd, NULL, &Rc)) != PBA_OK) die(ctx, "revcomp", st);
    if ((st = pba_index_build_set(ctx, T, pba_mask_from_pattern(argv[2]), &ix)) != PBA_OK) die(ctx, "index", st);
    std::vector<pba_map_row> rows(n ? n : 1);
    pba_map_stats stats;
    // locator.cpp:68-92: 50 probe offsets, reads of >= 500 bases
    if ((st = pba_map_reads(ctx, ix, T, Rd, Rc, R, 50, 500, 0, 0, PBA_KERNEL_AUTO, strands, rows.data(), &stats)) != PBA_OK) die(ctx, "map", st);

    // the runs: one call for the total, one with room for it
    std::vector<uint64_t> off((size_t)n + 1);
    std::vector<pba_aln_counts> counts(n ? n : 1);
    uint64_t total = 0;
    if ((st = pba_map_rows_cigar(ctx, T, Rd, Rc, rows.data(), n, R, NULL, 0, off.data(), &total, NULL, NULL)) != PBA_OK) die(ctx, "cigar", st);
    std::vector<uint32_t> cigar(total ? total : 1);
    if ((st = pba_map_rows_cigar(ctx, T, Rd, Rc, rows.data(), n, R, cigar.data(), total, off.data(), &total, counts.data(), NULL)) != PBA_OK)
        die(ctx, "cigar", st);

    std::vector<char> cg;
    long long found = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const pba_map_row &r = rows[k];
        if (!r.found) continue;
        const pba_aln_counts &c = counts[k];
        const int32_t nr = (int32_t)(off[k + 1] - off[k]);
        cg.resize((size_t)nr * 11 + 1);
        pba_cigar_string(cigar.data() + off[k], nr, cg.data(), (int32_t)cg.size());
        printf("read%d\t%llu\t%d\t%d\t%c\tcontig%d\t%llu\t%d\t%d\t%d\t%d\t255\tNM:i:%d\tcg:Z:%s\n", r.read,
               (unsigned long long)(roff[r.read + 1] - roff[r.read]), r.r_beg, r.r_end, r.strand == 1 ? '+' : '-', r.contig,
               (unsigned long long)(toff[r.contig + 1] - toff[r.contig]), r.c_beg, r.c_end, c.n_eq, c.n_eq + c.n_x + c.n_ins + c.n_del,
               r.cost, cg.data());
        ++found;
    }
    fprintf(stderr, "totally %u sequences processed, %lld mapped\n", n, found);
    pba_index_destroy(ix);
    pba_seqs_destroy(Rc);
    pba_seqs_destroy(Rd);
    pba_seqs_destroy(T);
    pba_ctx_destroy(ctx);
    return EXIT_SUCCESS;
}
