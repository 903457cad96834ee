// map_stream_gpu.cpp -- map reads that arrive as a stream onto a set of contigs, on both strands:
//   map_stream_gpu contig_file seed [R] [reads_per_batch] [strands] < seq_file
// contig_file holds one contig per line (an empty line is an empty contig); every whitespace-separated token of stdin is a
// read.  stdin is consumed in batches through a pba_map_stream: every batch is written straight into the pinned buffer of a
// free slot, batch k+1 is submitted before batch k is collected (its upload and the packs of both strands run behind the
// walks of batch k), and the rows of a batch are printed as soon as it completes -- one TSV line per read, the columns of
// pba_map_row in their order.  Nothing is allocated per batch.
//
//   g++ -O2 -I include -o map_stream_gpu examples/map_stream_gpu.cpp -L pacbioassembly_amd/lib -lpba -Wl,-rpath,$PWD/pacbioassembly_amd/lib
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
        fprintf(stderr, "usage: map_stream_gpu contig_file seed [R] [reads_per_batch] [strands] < seq_file\n");
        return EXIT_FAILURE;
    }
    const double R = argc > 3 ? atof(argv[3]) : 0.15;
    const long per_batch = argc > 4 ? atol(argv[4]) : 4096;
    const int strands = argc > 5 ? atoi(argv[5]) : 3;
    if (per_batch < 1 || per_batch > (1 << 24)) { fprintf(stderr, "reads_per_batch must be in [1, 2^24]\n"); return EXIT_FAILURE; }
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

    pba_ctx *ctx = NULL;
    int st = pba_ctx_create(0, &ctx);
    if (st != PBA_OK) die(NULL, "pba_ctx_create", st);
    pba_seqs *T = NULL;
    pba_index *ix = NULL;
    pba_map_stream *ms = NULL;
    if ((st = pba_seqs_from_text(ctx, text.data(), toff.data(), (uint32_t)(toff.size() - 1), 0, &T)) != PBA_OK) die(ctx, "contigs", st);
    if ((st = pba_index_build_set(ctx, T, pba_mask_from_pattern(argv[2]), &ix)) != PBA_OK) die(ctx, "index", st);
    // a slot holds reads_per_batch reads of up to 16 kb on average, 64 MB at the most (and always one read of the engine's limit)
    uint64_t slot_bytes = (uint64_t)per_batch * 16384;
    if (slot_bytes > (64u << 20)) slot_bytes = 64u << 20;
    if (slot_bytes < 65536) slot_bytes = 65536;
    // locator.cpp:68-92: 50 probe offsets, reads of >= 500 bases
    if ((st = pba_map_stream_create(ctx, ix, T, R, 50, 500, 0, 0, PBA_KERNEL_AUTO, strands, slot_bytes, (uint32_t)per_batch,
                                    PBA_STREAM_TEXT, &ms)) != PBA_OK) die(ctx, "stream", st);

    std::vector<pba_map_row> rows((size_t)per_batch);
    long long kept = 0, found = 0;
    int pending = 0;
    auto collect = [&]() {                                            // the oldest batch: its rows
        uint32_t n = 0;
        if ((st = pba_map_stream_collect(ms, rows.data(), (uint32_t)rows.size(), &n, NULL)) != PBA_OK) die(ctx, "map", st);
        for (uint32_t i = 0; i < n; ++i) {
            const pba_map_row &r = rows[i];
            printf("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n", r.read, r.nseq, r.found, r.strand, r.contig, r.j,
                   r.pos, r.cost, r.seglen, r.matlen_a, r.matlen_b, r.diag_cost, r.n_pairs, r.r_beg, r.r_end, r.c_beg, r.c_end);
            kept += r.nseq >= 0;
            found += r.found;
        }
        --pending;
    };
    char *bytes = NULL;
    uint64_t *offs = NULL;
    uint32_t n = 0;
    auto next_slot = [&]() {                                          // both slots in flight: the older one has to complete first
        if (pending == 2) collect();
        void *b = NULL;
        if ((st = pba_map_stream_buffer(ms, &b, &offs)) != PBA_OK) die(ctx, "buffer", st);
        bytes = (char *)b; offs[0] = 0; n = 0;
    };
    auto submit = [&]() {
        if ((st = pba_map_stream_submit(ms, n)) != PBA_OK) die(ctx, "reads", st);
        ++pending; bytes = NULL;
    };
    auto add = [&](const std::string &tok) {
        if (tok.size() > slot_bytes) die(ctx, "reads", PBA_E_TOOLONG);
        if (bytes && (n == (uint32_t)per_batch || offs[n] + tok.size() > slot_bytes)) submit();
        if (!bytes) next_slot();
        memcpy(bytes + offs[n], tok.data(), tok.size());
        offs[n + 1] = offs[n] + tok.size();
        ++n;
    };
    std::string tok;
    for (int ch; (ch = getchar()) != EOF;) {
        if (ch == ' ' || ch == '\n' || ch == '\t' || ch == '\r') {
            if (!tok.empty()) { add(tok); tok.clear(); }
        } else tok.push_back((char)ch);
    }
    if (!tok.empty()) add(tok);
    if (bytes) submit();
    while (pending) collect();
    fprintf(stderr, "totally %lld sequences processed, %lld mapped\n", kept, found);
    pba_map_stream_destroy(ms);
    pba_index_destroy(ix);
    pba_seqs_destroy(T);
    pba_ctx_destroy(ctx);
    return EXIT_SUCCESS;
}
