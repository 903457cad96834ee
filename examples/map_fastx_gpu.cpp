// map_fastx_gpu.cpp -- map the reads of a FASTA / FASTQ file onto the contigs of another, on both strands, as PAF with cg:Z::
//   map_fastx_gpu contigs.fa reads.fq seed [R] [strands]
// map_paf_gpu's pipeline with files as its users have them: each input is read by one fread and parsed on the device
// (pba_seqs_from_fastx, format by the first byte), the reads are mapped (pba_map_reads), the found rows are re-run with their
// paths run-length encoded (pba_map_rows_cigar), and one PAF line per found read goes to stdout -- under the files' own names,
// taken from the index of each parse.
//
//   g++ -O2 -I include -o map_fastx_gpu examples/map_fastx_gpu.cpp -L pacbioassembly_amd/lib -lpba -Wl,-rpath,$PWD/pacbioassembly_amd/lib
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

static std::vector<char> slurp(const char *path) {
    FILE *fp = fopen(path, "rb");
    if (!fp) { perror(path); exit(EXIT_FAILURE); }
    fseek(fp, 0, SEEK_END);
    const long n = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    std::vector<char> buf(n > 0 ? (size_t)n : 0);
    if (n > 0 && fread(buf.data(), 1, (size_t)n, fp) != (size_t)n) { perror(path); exit(EXIT_FAILURE); }
    fclose(fp);
    return buf;
}

struct Parsed {
    std::vector<char> file;
    pba_seqs *set = NULL;
    std::vector<pba_fastx_rec> recs;
    std::string name(uint32_t i) const { return std::string(file.data() + recs[i].hdr_off + 1, recs[i].name_len); }
};

static void parse(pba_ctx *ctx, const char *path, Parsed *p) {
    p->file = slurp(path);
    pba_fastx_index *ix = NULL;
    pba_fastx_stats st;
    const int rc = pba_seqs_from_fastx(ctx, p->file.data(), p->file.size(), PBA_FX_AUTO, 0, &p->set, &ix, &st);
    if (rc != PBA_OK) die(ctx, path, rc);
    p->recs.resize(pba_fastx_index_count(ix) ? pba_fastx_index_count(ix) : 1);
    pba_fastx_index_recs(ix, p->recs.data(), (uint32_t)p->recs.size());
    pba_fastx_index_destroy(ix);
    fprintf(stderr, "%s: %u %s records, %llu bases, parsed in %.2f ms (copy %.2f, pack %.2f)\n", path, st.n_records,
            st.format == PBA_FX_FASTQ ? "FASTQ" : "FASTA", (unsigned long long)st.n_bases, st.parse_ms, st.h2d_ms, st.pack_ms);
}

int main(int argc, char *argv[]) {
    if (argc <= 3) {
        fprintf(stderr, "usage: map_fastx_gpu contigs.fa reads.fq seed [R] [strands]\n");
        return EXIT_FAILURE;
    }
    const double R = argc > 4 ? atof(argv[4]) : 0.15;
    const int strands = argc > 5 ? atoi(argv[5]) : 3;
    pba_ctx *ctx = NULL;
    int st = pba_ctx_create(0, &ctx);
    if (st != PBA_OK) die(NULL, "pba_ctx_create", st);
    Parsed T, Rd;
    parse(ctx, argv[1], &T);
    parse(ctx, argv[2], &Rd);
    const uint32_t n = pba_seqs_count(Rd.set);
    pba_seqs *Rc = NULL;
    pba_index *ix = NULL;
    if ((st = pba_seqs_revcomp(ctx, Rd.set, NULL, &Rc)) != PBA_OK) die(ctx, "revcomp", st);
    if ((st = pba_index_build_set(ctx, T.set, pba_mask_from_pattern(argv[3]), &ix)) != PBA_OK) die(ctx, "index", st);
    std::vector<pba_map_row> rows(n ? n : 1);
    pba_map_stats stats;
    // locator.cpp:68-92: 50 probe offsets, reads of >= 500 bases
    if ((st = pba_map_reads(ctx, ix, T.set, Rd.set, Rc, R, 50, 500, 0, 0, PBA_KERNEL_AUTO, strands, rows.data(), &stats)) != PBA_OK) die(ctx, "map", st);

    // the runs: one call for the total, one with room for it
    std::vector<uint64_t> off((size_t)n + 1);
    std::vector<pba_aln_counts> counts(n ? n : 1);
    uint64_t total = 0;
    if ((st = pba_map_rows_cigar(ctx, T.set, Rd.set, Rc, rows.data(), n, R, NULL, 0, off.data(), &total, NULL, NULL)) != PBA_OK) die(ctx, "cigar", st);
    std::vector<uint32_t> cigar(total ? total : 1);
    if ((st = pba_map_rows_cigar(ctx, T.set, Rd.set, Rc, rows.data(), n, R, cigar.data(), total, off.data(), &total, counts.data(), NULL)) != PBA_OK)
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
        printf("%s\t%u\t%d\t%d\t%c\t%s\t%u\t%d\t%d\t%d\t%d\t255\tNM:i:%d\tcg:Z:%s\n", Rd.name((uint32_t)r.read).c_str(),
               Rd.recs[r.read].seq_len, r.r_beg, r.r_end, r.strand == 1 ? '+' : '-', T.name((uint32_t)r.contig).c_str(),
               T.recs[r.contig].seq_len, r.c_beg, r.c_end, c.n_eq, c.n_eq + c.n_x + c.n_ins + c.n_del, r.cost, cg.data());
        ++found;
    }
    fprintf(stderr, "totally %u sequences processed, %lld mapped\n", n, found);
    pba_index_destroy(ix);
    pba_seqs_destroy(Rc);
    pba_seqs_destroy(Rd.set);
    pba_seqs_destroy(T.set);
    pba_ctx_destroy(ctx);
    return EXIT_SUCCESS;
}
