/*
 * pba.h -- C ABI of the MI355X seed-and-extend overlap engine (libpba.so).
 *
 * This is the drop-in boundary.  The reference (vmingchen/PacBioAssembly) has no
 * FFI layer: its mains and tests compile against the header-level C++ API in
 * src/dna_seq.h, src/seq_aligner.h and src/ref_seq.h.  include/compat/ re-creates
 * that API (same class, method and field names) on top of the entry points below;
 * each entry point names the reference interface it replaces (file:line into
 * /root/reference/).  Plain pointers and sizes only; no exceptions cross the
 * boundary; every function that can fail returns a pba_status.
 *
 * Threading: a pba_ctx is bound to one GPU and one HIP stream and must be used by
 * one host thread at a time (the reference is single-threaded with global
 * singletons, spaced_seed.cpp:71-96).  One process per GPU, one ctx per process.
 *
 * There is no CPU fallback: with no usable GPU pba_ctx_create fails with
 * PBA_E_NODEVICE and nothing else in the device API can be called.
 */
#ifndef PBA_H
#define PBA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PBA_VERSION 1

typedef enum {
    PBA_OK = 0,
    PBA_E_INVALID = -1,     /* bad argument */
    PBA_E_NOMEM = -2,       /* host or device allocation failed */
    PBA_E_HIP = -3,         /* a HIP call or kernel failed; see pba_ctx_error */
    PBA_E_TOOLONG = -4,     /* sequence longer than the engine supports */
    PBA_E_NODEVICE = -5,    /* no usable gfx950 device */
    PBA_E_ALPHABET = -6     /* byte outside ACGT where the packed path needs ACGT */
} pba_status;

/* ------------------------------------------------------------------------ */
/* Host-side codec.  Pure functions, no ctx, bit-compatible with dna_seq.   */
/* ------------------------------------------------------------------------ */

/* dna_seq::encode (dna_seq.h:86): 16 chars -> u32, byte k = bases 4k..4k+3 */
uint32_t pba_encode16(const char *text16);
/* dna_seq::decode (dna_seq.h:101) */
void pba_decode16(uint32_t code, char *text16);
/* dna_seq::text2bin (dna_seq.h:113) with an explicit length: writes the record
 * [u32 len][ceil(len/4) packed bytes]; returns bytes written, 0 if cap is too small */
size_t pba_text2bin(const char *text, size_t tlen, uint8_t *record, size_t cap);
/* dna_seq::bin2text (dna_seq.h:133): returns the length, writes the NUL; 0 if cap <= len */
size_t pba_bin2text(const uint8_t *record, char *text, size_t cap);
/* dna_seq::seed_at (dna_seq.h:62), BUG-COMPATIBLE: for pos%4==0 it returns the word at
 * byte offset pos, exactly like the reference */
uint32_t pba_seed_at(const uint8_t *record, int pos);
/* the window seed_at was meant to return: == pba_encode16(text + pos) */
uint32_t pba_seed_at_fixed(const uint8_t *record, int pos);
/* parse_pattern (spaced_seed.cpp:167) / locator.cpp:51-54: '1' -> care, else don't care */
uint32_t pba_mask_from_pattern(const char *pattern);
/* dna_seq::value_at (dna_seq.h:78) */
char pba_value_at(uint8_t packed_byte, int idx);
/* record walk of open_binary (spaced_seed.cpp:330-342): byte offsets of the records with
 * min_excl < len < max_excl; returns how many were kept (writes at most cap offsets) */
size_t pba_open_binary(const uint8_t *file, size_t file_len, uint32_t min_excl, uint32_t max_excl,
                       uint64_t *offsets, size_t cap, size_t *n_records_total);

/* ------------------------------------------------------------------------ */
/* Synthetic workload generator (bench/test infrastructure, host code).     */
/* Integer-only counter RNG: the same bytes on every machine.               */
/* ------------------------------------------------------------------------ */
void pba_synth_genome(uint64_t seed, char *out, size_t n);
/* n_reads reads of read_len bases, forward strand, start uniform in [0, L - 1.5*read_len),
 * per-step error p_ins / p_del / p_sub.  out holds n_reads*read_len chars
 * (no separators); starts (nullable) receives each read's genome start. */
int pba_synth_reads(uint64_t seed, const char *genome, size_t L, uint32_t n_reads, uint32_t read_len,
                    double p_ins, double p_del, double p_sub, char *out, uint32_t *starts, int nthreads);
/* reads [r_lo, r_hi) of the same set (read r is a function of (seed, r) only): what one rank of a multi-GPU run generates.
 * out holds (r_hi - r_lo) * read_len chars, starts (nullable) r_hi - r_lo slots. */
int pba_synth_reads_range(uint64_t seed, const char *genome, size_t L, uint32_t r_lo, uint32_t r_hi, uint32_t read_len,
                          double p_ins, double p_del, double p_sub, char *out, uint32_t *starts, int nthreads);

/* ------------------------------------------------------------------------ */
/* Context                                                                  */
/* ------------------------------------------------------------------------ */
typedef struct pba_ctx pba_ctx;
int pba_ctx_create(int device_id, pba_ctx **ctx);
void pba_ctx_destroy(pba_ctx *ctx);
/* text of the last failure on this ctx (never NULL) */
const char *pba_ctx_error(const pba_ctx *ctx);
/* Streams.  Run on a caller-owned hipStream_t (e.g. torch's current stream); NULL = the ctx's own.  The contract:
 *  - Every call enqueues its device work on the ctx's stream -- the one set when the call is made -- and returns with that work
 *    complete (it ends in a synchronise of that stream).  The one exception is pba_*_stream_submit, which enqueues on the
 *    object's copy stream and returns at once; the matching collect orders the walk behind it with an event.
 *  - Device buffers, d_* parameters: a buffer the caller hands in (read, written or both) must have been written ON THE CTX'S
 *    STREAM -- then the call is ordered behind the write, pending or not, and no synchronise is owed -- or be complete before
 *    the call.  What a call writes into a d_* buffer is complete when it returns.  The ten entry points that take one are
 *    pba_seqs_from_device_text, pba_seqs_export, pba_seqs_from_device_packed, pba_index_scan, pba_index_from_entries,
 *    pba_overlap_probes, pba_overlap_all_probes, pba_probe_table_create, pba_census_mask_probes and (pba_dist.h)
 *    pba_dist_all_gather; tests/test_gpu_caller_stream.py holds the first nine to it with the producer still pending.
 *  - The ctx's own stream is created hipStreamNonBlocking: it is NOT ordered against the legacy default stream.  Work a
 *    host queued on the default stream (torch's default stream is that one) is not waited for by a ctx on its own stream:
 *    synchronise, or put both on a created stream.
 *  - NULL selects the own stream, and the legacy default stream's handle IS NULL (torch: handle 0): it cannot be selected.
 *    A host that works on the default stream synchronises before a call, or works on a created stream and sets that.
 *  - The stream must outlive its use: set another (or NULL) before destroying it.  pba_loc_stream / pba_map_stream objects
 *    record the ctx's stream at create and are tied to it (see there). */
int pba_ctx_set_stream(pba_ctx *ctx, void *hip_stream);
int pba_ctx_sync(pba_ctx *ctx);
/* The ctx keeps the work buffers of its drivers between calls (candidate arrays, per-read rows, traceback scratch: mapping
 * gigabytes anew costs more than the kernels that use them).  pba_ctx_trim gives them back to the device. */
int pba_ctx_trim(pba_ctx *ctx);
/* Test support: what a call finds in a buffer the ctx kept from an earlier call is undefined, and these two make that
 * testable.  pba_ctx_kept_bytes: the capacity in bytes of everything the ctx keeps between calls -- its pool slots in the
 * order of the internal enum (n_pool of them), the three idle arrays of the index cache (entries, offsets, the entry buffer
 * a build did not keep), the trace / vote scratch, the pinned staging buffer and the work-queue counters; 0 = not allocated.
 * pba_ctx_scribble: every one of them, over its whole capacity, set to `byte` (its low 8 bits); allocates nothing and frees
 * nothing.  No call may be in flight on the ctx, and open pba_loc_stream / pba_map_stream objects must be idle (nothing
 * submitted and not collected): the stream is synchronised before and after, but a batch in flight reads these buffers. */
typedef struct { uint32_t n_pool; uint64_t pool[32]; uint64_t ix_cache[3]; uint64_t scratch, stage, queue; } pba_kept_bytes;
int pba_ctx_kept_bytes(pba_ctx *ctx, pba_kept_bytes *out);
int pba_ctx_scribble(pba_ctx *ctx, int byte);
/* HIP-event timings (on the ctx's stream) of the most recent pba_index_build / pba_locate /
 * pba_align_batch / pba_spaced_round on this ctx: measurement support for bench.py.
 * The all-vs-all entry points (pba_overlap_all*, pba_overlap_strands*: the profile of the last pass) fill the four ring
 * fields for their walk and leave the timings alone: nb_first / n_first = ring and work items of the call's first walk
 * launch (0 = row sweep, or no launch at all), nb_redo / n_redo = ring and runs of the last launch that resumed parked
 * (target, query) runs (0 = none). */
typedef struct {
    float index_ms;        /* pba_index_build: first kernel to last kernel */
    float align_ms;        /* first launch of the aligning kernel (all pairs / reads) */
    float align_redo_ms;   /* second launch (pairs / reads the narrow band could not certify); 0 if none */
    uint32_t nb_first;     /* blocks per lane of the bit-vector array in the first launch; 0 = row sweep */
    uint32_t nb_redo;
    uint32_t n_first;      /* pairs or reads in the first launch */
    uint32_t n_redo;       /* pairs or reads re-run at the reference band */
} pba_profile;
int pba_ctx_last_profile(const pba_ctx *ctx, pba_profile *out);
/* device facts for the bench report */
int pba_ctx_device_info(const pba_ctx *ctx, char *name, size_t name_cap, int *n_cu, int *clock_mhz,
                        uint64_t *hbm_bytes);

/* ------------------------------------------------------------------------ */
/* Sequence sets resident in HBM, 2-bit packed in the reference byte layout */
/* (dna_seq.h:147-159: first base in bits 7:6), each sequence 16-B aligned. */
/* Replaces: the mmap'd read buffer (spaced_seed.cpp:310-345), contig[] and */
/* sequence[] (locator.cpp:26-27), ref_seq::txt_buf (ref_seq.h:370).        */
/* ------------------------------------------------------------------------ */
typedef struct pba_seqs pba_seqs;
/* text: concatenated ASCII; sequence i = text[offsets[i] .. offsets[i+1]).  Bytes are packed
 * with C2I (dna_seq.h:21).  If strict_acgt != 0 a byte outside "ACGT" fails with
 * PBA_E_ALPHABET (the packed DP compares codes, the reference compares bytes: they agree
 * exactly on ACGT input).  Packing runs on the GPU.  With strict_acgt == 0 such bytes are packed
 * as code 3 (that is what the seed index of locator.cpp:62-66 sees), the set remembers it, and the
 * aligning entry points (pba_align_batch, pba_locate, pba_spaced_round) refuse it with
 * PBA_E_ALPHABET rather than return scores the reference would not: use pba_align_text there. */
int pba_seqs_from_text(pba_ctx *ctx, const char *text, const uint64_t *offsets, uint32_t n,
                       int strict_acgt, pba_seqs **out);
/* same, but text/offsets are DEVICE pointers (inputs already resident in HBM) */
int pba_seqs_from_device_text(pba_ctx *ctx, const void *d_text, const void *d_offsets_u64, uint32_t n,
                              uint64_t total_bytes, uint32_t max_len, pba_seqs **out);
/* reference binary read file ([u32 len][packed])*, kept records min_excl < len < max_excl
 * (spaced_seed.cpp:330-342); payloads are uploaded as they are, no re-packing */
int pba_seqs_from_records(pba_ctx *ctx, const uint8_t *file, size_t file_len, uint32_t min_excl,
                          uint32_t max_excl, pba_seqs **out);
/* Multi-GPU exchange of packed reads (every rank packs its own shard, the shards are all-gathered over RCCL):
 * pba_seqs_export copies the set's packed arena (pba_seqs_packed_bytes bytes) into the DEVICE buffer d_dst and returns the
 * byte offset of every sequence's first packed byte in it (offsets: n host slots); pba_seqs_from_device_packed builds a
 * set from such bytes resident on the device -- the gathered buffer, offsets[i] = where sequence i starts in it (rank
 * base + exported offset), lengths in bases -- without re-packing (one device copy; the bit planes are rebuilt).
 * non_acgt: whether any contributing set was built with strict_acgt == 0 and met a byte outside ACGT. */
int pba_seqs_export(pba_ctx *ctx, const pba_seqs *s, void *d_dst, uint64_t cap, uint64_t *offsets);
int pba_seqs_from_device_packed(pba_ctx *ctx, const void *d_packed, uint64_t n_bytes, const uint64_t *offsets,
                                const uint32_t *lengths, uint32_t n, int non_acgt, pba_seqs **out);
int pba_seqs_non_acgt(const pba_seqs *s);
void pba_seqs_destroy(pba_seqs *s);
uint32_t pba_seqs_count(const pba_seqs *s);
uint32_t pba_seqs_max_len(const pba_seqs *s);
uint64_t pba_seqs_packed_bytes(const pba_seqs *s);
int pba_seqs_lengths(const pba_seqs *s, uint32_t *lengths, uint32_t cap);
/* unpack sequence i back to text (bin2text), for round-trip checks */
int pba_seqs_get_text(pba_ctx *ctx, const pba_seqs *s, uint32_t i, char *text, size_t cap);
/* A new set whose sequence i is rc(src i) -- reversed, then A<->T and C<->G (on the 2-bit codes: code ^ 3) -- where
 * flip == NULL or flip[i] != 0 (flip: n host bytes), and src i unchanged otherwise.  The layout is pba_seqs_from_text's
 * (16-byte aligned starts, zero pad bits), whatever layout src had (a binary read file's records included): byte for byte
 * what pba_seqs_from_text makes of the same texts.  Packed bytes and bit planes are built on the device; no base goes
 * through the host.  PBA_E_ALPHABET if src holds bytes outside ACGT (code 3 stands for N as well as T: no complement).
 * The reference never reverse-complements a read; this feeds pba_overlap_strands and pba_map_reads (the locate on both
 * strands). */
int pba_seqs_revcomp(pba_ctx *ctx, const pba_seqs *src, const uint8_t *flip, pba_seqs **out);

/* ------------------------------------------------------------------------ */
/* FASTA / FASTQ in, FASTA out.  The file image goes up as it is; line ends, */
/* headers and sequence lines are found on the device, the    */
/* bases are gathered into one device text and packed by the path of         */
/* pba_seqs_from_device_text.  The reference reads its own binary record     */
/* file only (spaced_seed.cpp:310-345); this is what its users' files are.   */
/* ------------------------------------------------------------------------ */
/* Lines end at '\n'; one '\r' directly before it (or at the very end of a file without a final '\n') is not content; a line
 * with no content is blank.  FASTA: a line whose first byte is '>' starts a record, every other non-blank line up to the next
 * header is one of its sequence lines (concatenated; none: a sequence of length 0), blank lines are ignored anywhere, a
 * non-blank line before the first header is an error.  FASTQ, strictly four lines per record counted from the start of the
 * file: '@' header, sequence (may be empty), '+' line (the rest of it ignored), quality of the sequence's length (not kept:
 * qual_off says where it is); blank lines only after the last record.  An empty or all-blank file is a set of 0 sequences.
 * PBA_FX_AUTO: the first byte of the first non-blank line decides ('>' / '@', else PBA_E_INVALID).  Sequence bytes a-z are
 * folded to upper case unless PBA_FX_KEEP_CASE; every other byte -- a space or tab too -- goes through and is a base outside
 * ACGT.  A structural error is PBA_E_INVALID with "line <1-based number of the first offending line>" in pba_ctx_error (a
 * truncated last FASTQ record: the line that is missing); nothing is returned.  Name = header content after the marker up
 * to the first space or tab. */
enum { PBA_FX_AUTO = 0, PBA_FX_FASTA = 1, PBA_FX_FASTQ = 2 };
#define PBA_FX_KEEP_CASE   1u
#define PBA_FX_STRICT_ACGT 2u   /* any base outside ACGT after folding: PBA_E_ALPHABET, nothing is returned */
typedef struct {                /* all offsets into the caller's file image */
    uint64_t hdr_off;           /* the '>' / '@' */
    uint64_t seq_off;           /* first byte of the first sequence line (FASTA without one: the byte after the header line) */
    uint64_t qual_off;          /* FASTQ: first byte of the quality line; FASTA: 0 */
    uint32_t hdr_len, name_len; /* header content without the marker and without line end; its first token */
    uint32_t seq_len, n_seq_lines;
} pba_fastx_rec;
typedef struct {
    int32_t format; uint32_t n_records, n_pieces, max_len;   /* format: as resolved; 0 = no non-blank line */
    uint64_t n_bytes, n_lines, n_bases, n_folded /* lower-case bytes folded */;
    float h2d_ms, parse_ms, pack_ms;   /* HIP events on the ctx's stream, summed over the pieces */
} pba_fastx_stats;
typedef struct pba_fastx_index pba_fastx_index;   /* host object: the records of one parse */

/* The set is a plain pba_seqs in pba_seqs_from_text's layout, byte for byte what pba_seqs_from_text makes of the same
 * sequences; sequence i is record i in file order; pba_seqs_non_acgt reports what the file held.  The file is cut with
 * pba_fastx_cut into pieces of at most max_piece_bytes (_budget; 0 or the plain call: 1 GiB; more is clamped to it, so that
 * line and byte counters inside a piece are 32-bit); the answer does not depend on the cut.  A record longer than a piece:
 * PBA_E_TOOLONG, its hdr_off in pba_ctx_error.  More than 0x7FFFFFFF records, or a record of 0x7FFFFFF0 bases or more:
 * PBA_E_TOOLONG.  Work buffers come from the ctx's pool (pba_ctx_trim). */
int pba_seqs_from_fastx(pba_ctx *ctx, const void *file, uint64_t file_len, int format, uint32_t flags,
                        pba_seqs **out, pba_fastx_index **index /* nullable */, pba_fastx_stats *stats /* nullable */);
int pba_seqs_from_fastx_budget(pba_ctx *ctx, const void *file, uint64_t file_len, int format, uint32_t flags,
                               pba_seqs **out, pba_fastx_index **index /* nullable */, pba_fastx_stats *stats /* nullable */,
                               uint64_t max_piece_bytes /* 0 = the default */);
uint32_t pba_fastx_index_count(const pba_fastx_index *index);
int pba_fastx_index_recs(const pba_fastx_index *index, pba_fastx_rec *out, uint32_t cap);   /* cap below count: PBA_E_INVALID */
void pba_fastx_index_destroy(pba_fastx_index *index);
/* host arithmetic, no ctx */
/* PBA_FX_FASTA / PBA_FX_FASTQ, 0 for no non-blank line, PBA_E_INVALID for another first byte (or file == NULL with bytes) */
int pba_fastx_sniff(const void *file, uint64_t file_len);
/* *cut = the largest record start p with 0 < p <= want; file_len if want >= file_len; 0 if there is no such p.  FASTA: a line
 * start holding '>'.  FASTQ: a line start holding '@' whose line after next exists and starts with '+' -- exact for files
 * whose sequence lines do not begin with '+' (a quality line may begin with '@' or '+': the line two below such a quality
 * line is the next record's sequence).  A file that breaks the assumption is cut inside a record, and the parse of that
 * piece refuses it (PBA_E_INVALID).  format PBA_FX_AUTO: as pba_fastx_sniff finds (PBA_E_INVALID where that does; a file
 * without a non-blank line has no record start). */
int pba_fastx_cut(const void *file, uint64_t file_len, int format, uint64_t want, uint64_t *cut);
/* The bases of sequences [lo, hi) as one FASTA image: record i is '>' + name + '\n', then its bases in lines of `width`
 * (0: one line) with a '\n' after each; a sequence of length 0 contributes the header line only.  names / name_off: the
 * name of sequence lo + k is names[name_off[k] .. name_off[k + 1]); both NULL: the decimal index lo + k.  Code 3 prints as
 * 'T', as pba_seqs_get_text does: a set with bytes outside ACGT does not come back as it went in.  The size is host
 * arithmetic from the lengths: *n_bytes is always set.  out == NULL: size only.  cap below the size: PBA_E_INVALID, nothing is
 * written.  One kernel writes bases and line ends into a device image, one copy brings it out, the host fills in the
 * headers: one synchronise, whatever hi - lo is. */
int pba_seqs_write_fasta(pba_ctx *ctx, const pba_seqs *s, uint32_t lo, uint32_t hi, const char *names,
                         const uint64_t *name_off /* hi-lo+1 entries; both NULL: decimal ids */, uint32_t width /* 0: one line */,
                         char *out /* NULL: size only */, uint64_t cap, uint64_t *n_bytes);

/* ------------------------------------------------------------------------ */
/* Seed-hit index.  Replaces hash_table = hash_map<unsigned, list<int>>     */
/* (common.h:54) and its two builders.                                      */
/* ------------------------------------------------------------------------ */
typedef struct pba_index pba_index;
typedef enum {
    PBA_INDEX_ALL = 0,        /* locator.cpp:62-66: every position [0,len), tail windows padded with code 3 */
    PBA_INDEX_HEAD_TAIL = 1   /* ref_seq::get_seedmap, ref_seq.h:291-311: head ascending, then tail descending */
} pba_index_mode;
/* index sequence `seq` of `target` under `mask`; entries whose masked key is 0 are dropped
 * (ref_seq.h:300,307; locator.cpp:64); per-key hit order = the reference's insertion order */
int pba_index_build(pba_ctx *ctx, const pba_seqs *target, uint32_t seq, uint32_t mask, int mode,
                    pba_index **out);
/* Multi-GPU form of the build (one process per GPU; the exchange itself is the caller's RCCL
 * all-gather on device buffers): rank `part` of `nparts` scans its contiguous slice of the
 * reference's visiting order and writes the raw entries (key << 32 | ordinal, any order) to the
 * DEVICE buffer d_entries (cap u64 slots) ... */
int pba_index_scan(pba_ctx *ctx, const pba_seqs *target, uint32_t seq, uint32_t mask, int mode, uint32_t part,
                   uint32_t nparts, void *d_entries, uint64_t cap, uint64_t *n_out);
/* ... and every rank builds the same index from the gathered DEVICE list (n slots; slots holding
 * all-ones are padding).  seq_len / mode / mask must be those of the scan. */
int pba_index_from_entries(pba_ctx *ctx, const void *d_entries, uint64_t n, uint32_t mask, int mode,
                           uint32_t seq_len, pba_index **out);
/* PBA_INDEX_ALL applied to EVERY sequence of `target`, each on its own: every position [0, len_c) of contig c is indexed, tail
 * windows are padded with code 3 from that contig's own length (no window sees a neighbour's bases), masked key 0 is dropped.
 * The ordinal of an entry is its GLOBAL position g = cum[c] + pos, cum = the exclusive prefix sum of the lengths; per-key hit
 * order is ascending g: the per-contig lists of locator.cpp:62-66 concatenated in contig order.  pba_index_find /
 * pba_index_dump on such an index return global positions; pba_index_visited the total bases.  Empty contigs and contigs
 * shorter than 16 bases are legal; a set with bytes outside ACGT is legal here (pba_map_reads refuses it); the total must
 * stay below 0x7FFFFFF0 bases (PBA_E_TOOLONG, decided from the lengths before anything is allocated).  One segmented scan
 * launch whatever the number of contigs.  For pba_map_reads. */
int pba_index_build_set(pba_ctx *ctx, const pba_seqs *target, uint32_t mask, pba_index **out);
/* sequences the index covers: 1 for pba_index_build / pba_index_from_entries */
uint32_t pba_index_seqs(const pba_index *ix);
void pba_index_destroy(pba_index *ix);
uint64_t pba_index_entries(const pba_index *ix);
/* what get_seedmap returns (ref_seq.h:310): positions visited, not entries kept */
uint32_t pba_index_visited(const pba_index *ix);
/* all entries sorted by key, reference hit order within a key; returns PBA_OK and *n.  The partitions are merged on the
 * host, so a dump does not witness the order the device left the entries in; pba_index_find does. */
int pba_index_dump(pba_ctx *ctx, const pba_index *ix, uint32_t *keys, int32_t *pos, uint64_t cap, uint64_t *n);
/* hash_table::find (locator.cpp:76, spaced_seed.cpp:265) for a batch of keys: for key q the hits are
 * hit_pos[hit_off[q] .. hit_off[q+1]) in reference list order.  hit_off has n_keys+1 slots. */
int pba_index_find(pba_ctx *ctx, const pba_index *ix, const uint32_t *keys, uint32_t n_keys,
                   uint64_t *hit_off, int32_t *hit_pos, uint64_t hit_cap);

/* ------------------------------------------------------------------------ */
/* Banded edit-distance extension.  Replaces seq_aligner<MAXN,MAXM>::align  */
/* (seq_aligner.h:92-125) and its result fields (seq_aligner.h:73-81).      */
/* ------------------------------------------------------------------------ */
typedef struct {
    uint32_t a_seq;      /* sequence id in set A */
    int32_t  a_pos;      /* accessor origin: base index inside the sequence (dna_seq.h:191) */
    int32_t  a_len;      /* accessor length */
    uint32_t b_seq;
    int32_t  b_pos;
    int32_t  b_len;
    uint32_t flags;      /* PBA_A_BACKWARD / PBA_B_BACKWARD: element k is seq[pos-k] (dna_seq.h:211,221) */
} pba_pair;
#define PBA_A_BACKWARD 1u
#define PBA_B_BACKWARD 2u

typedef struct {
    int32_t rc;          /* align()'s return: -1 or matlen_b (seq_aligner.h:106,111,114,124) */
    int32_t cost;        /* final_cost() (seq_aligner.h:130); 0 when rc < 0 */
    int32_t matlen_a;    /* 0 when rc < 0 unless only the acceptance test failed */
    int32_t matlen_b;
    int32_t len_a;       /* parameter block, seq_aligner.h:94-102 */
    int32_t len_b;
    int32_t max_dst;
    int32_t diag_cost;   /* get_cost(m, m), m = min(len_a, len_b): the end of the diagonal -- what locator.cpp:86 prints as
                          * get_cost(len - j, len - j) when len_b >= len_a; -1 when the sweep stopped before that row */
} pba_result;

typedef enum {
    PBA_KERNEL_AUTO = 0,
    PBA_KERNEL_ROWSWEEP = 1,   /* full-band row sweep, band row in LDS */
    PBA_KERNEL_BITVEC = 2      /* bit-parallel delta encoding, exact */
} pba_kernel;

/* maxn/maxm: the template limits of the seq_aligner instantiation being replaced (size guard,
 * seq_aligner.h:104: len_a >= maxn+maxm || max_dst >= maxm -> -1); maxn <= 0 disables the guard */
int pba_align_batch(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n,
                    double R, int maxn, int maxm, int kernel, pba_result *out);
/* one pair given as host text, RAW BYTE comparison exactly like seq_aligner.h:136 (any bytes,
 * case-sensitive).  a/b are accessor origins: element k is p[k] when fwd, p[-k] otherwise. */
int pba_align_text(pba_ctx *ctx, const char *a, int a_fwd, int a_len, const char *b, int b_fwd, int b_len,
                   double R, int maxn, int maxm, pba_result *out);

/* Traceback (seq_aligner.h:115-116, 214-233): the same alignment plus its edit script, ops[k] = 1 MATCH,
 * 2 INSERT, 3 DELETE in the order seq_aligner::edits[] holds them (the `val` of a MATCH / INSERT is the b
 * element it consumes, which the caller can read off b while replaying the ops).
 * Text form: raw bytes, full-band row sweep with one parent code per band cell in HBM
 * ((len_a+1) * (2*max_dst+1) bytes): for single pairs (display, the compat seq_aligner).
 * *nedit is always the full length of the script (0 when rc < 0); ops receives its first min(*nedit, ops_cap) ops in
 * edits[] order (the origin's end of the path), whichever kernel answers, and no byte of ops behind them is written.
 * ops_cap = a_len + b_len always holds the whole script. */
int pba_align_text_trace(pba_ctx *ctx, const char *a, int a_fwd, int a_len, const char *b, int b_fwd, int b_len,
                         double R, int maxn, int maxm, pba_result *out, uint8_t *ops, int32_t ops_cap, int32_t *nedit);
/* The DP matrix itself, for callers that read it (seq_aligner<>::mat, get_cost / get_parent, seq_aligner.h:81,131-134;
 * locator.cpp:86): cost[i * W + c] and parent[i * W + c] for cell (i, j) with W = 2*max_dst + 1 and c = j - i + max_dst, the
 * reference's own diagonal-stripe layout; (len_a + 1) * W cells (cap_cells must hold them: len_a and max_dst follow from the
 * lengths and R as in seq_aligner.h:94-102).  Cells the call writes -- init_cell's borders and the band of rows
 * 1 .. *rows_swept (all rows, or up to the row of the early failure) -- hold their values; every other cell holds cost
 * 0xFFFF and parent 0 (the reference would hand back whatever an earlier call left there).  One pair, raw bytes. */
int pba_align_text_matrix(pba_ctx *ctx, const char *a, int a_fwd, int a_len, const char *b, int b_fwd, int b_len, double R,
                          int maxn, int maxm, pba_result *out, uint16_t *cost, uint8_t *parent, uint64_t cap_cells,
                          int32_t *rows_swept);
/* Batch form on packed sets: pair q's script goes to ops[ops_off[q] .. ops_off[q+1]) (needs a_len + b_len
 * slots), its length to nedit[q] (0 when rc < 0).  kernel: PBA_KERNEL_AUTO / _BITVEC run the bit-vector array
 * and stream 2 parent bits per processed cell into a per-wavefront scratch area that the same wavefront walks
 * back (HBM-bound: ~16 MB written per 15 kb pair, any batch size); PBA_KERNEL_ROWSWEEP keeps one parent byte
 * per band cell for every pair of the batch at once (135 MB per 15 kb pair; the cross-check). */
int pba_align_batch_trace(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n,
                          double R, int maxn, int maxm, int kernel, pba_result *out, uint8_t *ops,
                          const uint64_t *ops_off, int32_t *nedit);

/* Run-length alignments (CIGAR over = X I D).  A run is one 32-bit word, len << 4 | op, op in BAM's numbering; the four
 * counts are the bases of each kind.  By default a is the CIGAR's query and b its reference: I consumes a only (the
 * reference's DELETE, seq_aligner.h:170), D consumes b only (its INSERT, seq_aligner.h:167); a MATCH (seq_aligner.h:164) is
 * `=` where the two elements are equal and X where they are not. */
#define PBA_CIG_INS 1
#define PBA_CIG_DEL 2
#define PBA_CIG_EQ  7
#define PBA_CIG_X   8
typedef struct { int32_t n_eq, n_x, n_ins, n_del; } pba_aln_counts;
#define PBA_CIG_REVERSED   1u   /* runs goal-first (text order of two backward accessors) */
#define PBA_CIG_B_IS_QUERY 2u   /* I consumes b only, D consumes a only */
/* Host arithmetic, no ctx: an upper bound on the runs of a successful pair.  After the clip of seq_aligner.h:94-102, with
 * m = min(len_a, len_b): m > 10 gives 2 * max_dst - 1 (every edit adds at most two runs to the single run of an exact copy,
 * and a pair that passed the early-failure test at row m, seq_aligner.h:185, costs at most floor(m * R) = max_dst - 1);
 * m <= 10, where no such test ran, gives len_a + len_b.  0 for a negative length or an R outside (0, 1). */
uint32_t pba_cigar_bound(int a_len, int b_len, double R);
/* The alignments of pba_align_batch_trace as runs, made on the device from the traceback walk (no script exists): pair q's
 * runs go to cigar[cig_off[q] .. ), their number to ncig[q], the bases of each kind to counts[q].  cig_off (n + 1 entries)
 * must leave at least pba_cigar_bound(a_len, b_len, R) slots per pair, else PBA_E_INVALID.  A pair with rc < 0 has
 * ncig = 0 and zero counts.  For every other pair n_eq + n_x + n_ins = matlen_a, n_eq + n_x + n_del = matlen_b (I and D
 * exchanged under PBA_CIG_B_IS_QUERY) and n_x + n_ins + n_del = cost.  Runs are origin-first, the order of edits[], or
 * goal-first under PBA_CIG_REVERSED.  Bit-vector kernel only: a band too wide for it is PBA_E_TOOLONG.  Sets with bytes
 * outside ACGT: PBA_E_ALPHABET.  A pair whose runs outgrow its slot (the bound would be wrong) is PBA_E_HIP, text in
 * pba_ctx_error; nothing is written beyond a slot. */
int pba_align_batch_cigar(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R,
                          int maxn, int maxm, uint32_t flags, pba_result *out, uint32_t *cigar, const uint64_t *cig_off,
                          int32_t *ncig, pba_aln_counts *counts);
/* Host helpers, no ctx.  The same encoding from a script (pba_align_text_trace, pba_align_batch_trace: origin-first ops) and
 * the elements of its two accessors in element order (a_elems[k] = element k of a; any bytes; each array holds at least the
 * elements the script consumes, matlen_a and matlen_b): at most cap runs are written, the number of runs is returned (-1
 * for a NULL or an op outside 1 .. 3); counts is nullable. */
int pba_cigar_from_script(const uint8_t *ops, int32_t nedit, const char *a_elems, const char *b_elems, uint32_t flags,
                          uint32_t *cigar, int32_t cap, pba_aln_counts *counts);
/* "12=1X3I..." with a terminating NUL; returns the length, 0 if cap is too small (or n == 0: the empty string) */
int pba_cigar_string(const uint32_t *cigar, int32_t n, char *out, int32_t cap);

/* ------------------------------------------------------------------------ */
/* Consensus voting and reference growth: the unlocked half of ref_seq      */
/* (ref_seq.h:25-188 base_vote / vote_box, :207-242 ctor / append / prepend, */
/* :317-362 evolve / elect).  One vote box per reference position, resident */
/* in HBM; max_len plays MAX_SEQ_LEN (common.h:31): the object spans        */
/* 3*max_len positions with its origin (`beg`) at max_len.                  */
/* ------------------------------------------------------------------------ */
typedef struct pba_cons pba_cons;
/* ref_seq(const char*, int len, bool, int w) (ref_seq.h:218-225): every box starts as vote_box(text[i], weight) */
int pba_cons_create(pba_ctx *ctx, const char *text, int len, int weight, int max_len, pba_cons **out);
void pba_cons_destroy(pba_cons *c);
/* extent[0..2] = pre - beg, post - beg, end - beg (ref_seq.h:364-367) */
int pba_cons_extent(const pba_cons *c, int32_t *extent);
/* ref_seq::append / prepend (ref_seq.h:227-242): seg holds the new characters in text order */
int pba_cons_append(pba_ctx *ctx, pba_cons *c, const char *seg, int len);
int pba_cons_prepend(pba_ctx *ctx, pba_cons *c, const char *seg, int len);
/* ref_seq::elect + apply_edits (ref_seq.h:352-362, 25-41) for n edit scripts at once (votes commute): script q
 * starts at reference position pos[q] (relative to beg, must be contained), runs forward (fwd[q] != 0) or
 * backward, and is ops/vals[ops_off[q] .. +nedit[q]) with ops as pba_align_*_trace returns them and vals[k] =
 * edits[k].val (the b element of a MATCH / INSERT, seq_aligner.h:218,224). */
int pba_cons_elect(pba_ctx *ctx, pba_cons *c, uint32_t n, const int32_t *pos, const uint8_t *fwd, const uint8_t *ops,
                   const char *vals, const uint64_t *ops_off, const int32_t *nedit);
/* The batch form of try_align's align + OVERLAP_MIN gate + elect (ref_seq.h:264-267), everything on the device: pair q
 * aligns a = A[ref_seq] from pairs[q].a_pos (the reference text of these boxes, as the caller uploaded it) against its
 * b, and if it succeeds with matlen_a >= overlap_min the path is voted straight from the traceback walk -- no edit
 * script leaves the GPU.  Both accessors of a pair run in the same direction.  No growth: append / prepend stay the
 * caller's (a round of interior reads).  out[q] as pba_align_batch returns it. */
int pba_cons_vote_pairs(pba_ctx *ctx, pba_cons *c, const pba_seqs *A, uint32_t ref_seq, const pba_seqs *B,
                        const pba_pair *pairs, size_t n, double R, int maxn, int maxm, int overlap_min, pba_result *out);
/* ref_seq::evolve (ref_seq.h:317-349): votes -> next reference; the boxes keep their counts, the new text
 * (new_len characters, up to cap copied) starts at beg and pre = beg, post = end = beg + new_len. */
int pba_cons_evolve(pba_ctx *ctx, pba_cons *c, char *text_out, int cap, int32_t *new_len);
/* the boxes of [pre, post) in order: sel/sup 4 u16 each (A,C,G,T), tot; *n = their number (up to cap copied) */
int pba_cons_dump(pba_ctx *ctx, const pba_cons *c, uint16_t *sel, uint16_t *sup, int32_t *tot, int cap, int32_t *n);
/* the text of [pre, post) as ref_seq::get_accessor sees it */
int pba_cons_text(pba_ctx *ctx, const pba_cons *c, char *out, int cap, int32_t *n);

/* ------------------------------------------------------------------------ */
/* Drivers: the reference's ordered first-success loops, run on the GPU.    */
/* ------------------------------------------------------------------------ */
typedef struct {
    int32_t read;        /* index into the read set */
    int32_t nseq;        /* locator's id: index among reads with len >= min_len, else -1 (locator.cpp:72,91) */
    int32_t found;
    int32_t j;           /* probe offset of the successful candidate, -1 if none */
    int32_t pos;         /* TSV column 2 (locator.cpp:84) */
    int32_t cost;        /* TSV column 3 */
    int32_t seglen;      /* TSV column 4: len - j */
    int32_t matlen_a, matlen_b;
    int32_t n_pairs;     /* candidate pairs the reference loop hands to align for this read */
    int32_t diag_cost;   /* TSV column 5 (locator.cpp:86): get_cost(len - j, len - j), a written cell when the contig remainder is
                          * at least as long as the read remainder; -1 if none */
} pba_loc_row;

typedef struct {
    int64_t n_reads_kept, n_probe_hits, n_pairs, n_located;
    int64_t n_cells;     /* band cells the reference loop would evaluate for those pairs */
} pba_loc_stats;

/* locator.cpp:70-92 with R / trials / min_len as parameters (stock: 0.15 / 50 / 500).
 * ix must be a PBA_INDEX_ALL index of sequence target_seq of `target`. */
int pba_locate(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, uint32_t target_seq,
               const pba_seqs *reads, double R, int trials, int min_len, int maxn, int maxm, int kernel,
               pba_loc_row *rows, pba_loc_stats *stats);

/* locator.cpp:70-92 against a target of MANY sequences and on BOTH strands of the reads.  ix: the pba_index_build_set index of
 * `target` (same count, same lengths; else PBA_E_INVALID).  A read's order of trial on one strand: for j ascending, the hits
 * of its key in ascending (contig, pos); first success, as pba_locate.  strands: 1 = the reads as given, 2 = rc(read) only,
 * 3 = every read on +, then the reads with len >= min_len that found nothing again as rc(read) (an id list over reads_rc, no
 * new set); the first success in that order is the row.  reads_rc: pba_seqs_revcomp(reads, NULL), or NULL to have it built
 * inside (a set of another count or other lengths: PBA_E_INVALID).  Sets with bytes outside ACGT: PBA_E_ALPHABET.
 * j, pos, cost, seglen, matlen_a, matlen_b, diag_cost are pba_loc_row's, in the coordinates of the text that was walked (for
 * strand -1: of rc(read)), pos local to the contig; not found: pba_loc_row's values, strand 0, contig -1, intervals 0.
 * Intervals (a = the read from j, b = the contig from pos): walked read [j, j + matlen_a), contig [pos, pos + matlen_b);
 * for strand -1 the read interval is given on the read's forward strand, [len - j - matlen_a, len - j).
 * stats->strand[0] / [1]: the + / - walk (n_reads_kept: the reads of that walk with len >= min_len); n_second_walk: reads
 * walked on - after failing on + (strands == 3).  pba_ctx_last_profile afterwards: the two walks summed. */
typedef struct {
    int32_t read, nseq, found;
    int32_t strand;                 /* +1 / -1; 0 when not found */
    int32_t contig;                 /* -1 when not found */
    int32_t j, pos, cost, seglen, matlen_a, matlen_b, diag_cost;   /* as pba_loc_row, in the coordinates of the text walked */
    int32_t n_pairs;                /* pairs of the + walk plus pairs of the - walk */
    int32_t r_beg, r_end, c_beg, c_end;   /* half-open, forward strand of the read / of the contig */
} pba_map_row;
typedef struct { pba_loc_stats strand[2]; uint32_t n_second_walk; } pba_map_stats;
int pba_map_reads(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, const pba_seqs *reads,
                  const pba_seqs *reads_rc /* nullable: built inside */, double R, int trials, int min_len,
                  int maxn, int maxm, int kernel, int strands /* 1, 2, 3 as pba_overlap_strands */,
                  pba_map_row *rows, pba_map_stats *stats);

typedef struct {
    int32_t read, found, j, dir;   /* dir +1 forward / -1 backward (spaced_seed.cpp:426) */
    int32_t ref_pos;               /* hit position (list value) */
    int32_t cost, matlen_a, matlen_b;
    int32_t n_trials;              /* probes that hit the map (DBG _ntrials, spaced_seed.cpp:268-270) */
    int32_t n_pairs;
} pba_ss_row;

/* one locked round of spaced_seed.cpp:420-437 against a PBA_INDEX_HEAD_TAIL index.
 * buggy_seed_at != 0 reproduces dna_seq::seed_at's pos%4==0 behaviour (needs reads built with
 * pba_seqs_from_records so the bytes after each record are the file's). */
int pba_spaced_round(pba_ctx *ctx, const pba_index *ix, const pba_seqs *ref, uint32_t ref_seq,
                     const pba_seqs *reads, double R, int max_trial, int overlap_min, int buggy_seed_at,
                     int kernel, pba_ss_row *rows);

/* spaced_seed's main loop (spaced_seed.cpp:409-452) for a LOCKED reference (-l; the reference never changes, so a
 * round is pba_spaced_round over the reads not found yet): the seed of a round is masks[picks[k] % n_masks] for the
 * k-th draw (picks[] stands in for rand(), spaced_seed.cpp:412) after a round that found something, else the seeds in
 * order; found reads leave the pool; the loop ends after max_round rounds or when every seed failed in a row.
 * rows[r] = the row of the round that found read r (found = 0: its last failed round), found_round[r] = that round
 * (1-based) or 0; log[k] describes round k+1 (up to log_cap), *n_rounds = rounds run. */
typedef struct {
    int32_t round;
    uint32_t mask;
    int32_t n_tried, n_found;
} pba_ss_round_log;
int pba_spaced_multi(pba_ctx *ctx, const pba_seqs *ref, uint32_t ref_seq, const pba_seqs *reads, double ratio, int max_trial,
                     int overlap_min, int buggy_seed_at, int kernel, const uint32_t *masks, int n_masks,
                     const uint32_t *picks, int n_picks, int max_round, pba_ss_row *rows, int32_t *found_round,
                     pba_ss_round_log *log, int log_cap, int *n_rounds);

/* One round of spaced_seed.cpp:420-446 against the UNLOCKED reference c: the reads pool[0..n_pool) in that order, each
 * walked like spaced_seed.cpp:424-437 (first success over j, forward then backward) with ref_seq::try_align voting and
 * growing the reference as it goes (ref_seq.h:259-276) -- so a read sees the text as the reads before it left it.  The
 * seed index is get_seedmap's (ref_seq.h:291-311) over [beg, end) as the round finds it.  maxn / maxm: the size guard of
 * the caller's aligner (t_aligner: 26000, 6000; 0, 0 = none).  rows[read id] is filled for the reads of the pool.  The
 * caller calls pba_cons_evolve afterwards (spaced_seed.cpp:451).  Replaces: the loop body of spaced_seed.cpp:410-446
 * for a reference that is not locked.  Runs as batches on the device (see pba_device.hip); results are those of the
 * serial loop. */
typedef struct {
    int32_t n_found;               /* nmatches, spaced_seed.cpp:434 */
    int32_t n_batches;             /* launches of the round kernel (1 + one per growth that mattered to a later read) */
    int32_t n_grown_fwd, n_grown_bwd;   /* append / prepend calls, ref_seq.h:270-273 */
    uint32_t n_deferred;           /* reads put back behind a growth, summed over the batches */
    uint32_t n_index;              /* entries of the round's seed index */
} pba_cons_round_stats;
int pba_cons_round(pba_ctx *ctx, pba_cons *c, const pba_seqs *reads, const uint32_t *pool, uint32_t n_pool, uint32_t mask,
                   double R, int max_trial, int overlap_min, int buggy_seed_at, int kernel, int maxn, int maxm,
                   pba_ss_row *rows, pba_cons_round_stats *stats);
/* spaced_seed's main loop (spaced_seed.cpp:409-452) WITHOUT -l: pba_cons_round over the reads not found yet, the seed of
 * a round chosen as in pba_spaced_multi, pba_cons_evolve after every round except one that ends the loop (every seed
 * failed in a row, spaced_seed.cpp:450).  rows / found_round / log as in pba_spaced_multi; ref_len_log[k] = length of the
 * reference after round k+1. */
int pba_cons_assemble(pba_ctx *ctx, pba_cons *c, const pba_seqs *reads, double R, int max_trial, int overlap_min,
                      int buggy_seed_at, int kernel, int maxn, int maxm, const uint32_t *masks, int n_masks,
                      const uint32_t *picks, int n_picks, int max_round, pba_ss_row *rows, int32_t *found_round,
                      pba_ss_round_log *log, int32_t *ref_len_log, int log_cap, int *n_rounds);

/* ------------------------------------------------------------------------ */
/* Streamed locate: read batches that arrive step by step.  pba_locate works  */
/* on a resident set; a caller with fresh reads every step (locator.cpp:70    */
/* consumes them as they come) would pay pba_seqs_from_text -- allocations,   */
/* a pageable copy, two packing kernels, several synchronisations -- in front */
/* of every step.  A stream owns two SLOTS and a copy stream of its own:      */
/* while the locate of batch k runs on the ctx's stream, batch k+1 is copied  */
/* from pinned memory and packed on the copy stream.  Nothing is allocated or */
/* freed between create and destroy.                                          */
/*   for every batch:  pba_loc_stream_buffer  -> fill the pinned buffer       */
/*                     pba_loc_stream_submit  -> returns at once              */
/*                     pba_loc_stream_collect -> rows of the OLDEST batch     */
/* Submit batch k+1 before collecting batch k to hide the upload.             */
/* The pinned buffer of a slot must not be written between its submit and the */
/* collect of that batch (nothing can check this).  One host thread, no graph */
/* capture.  The object records the ctx's stream at create and is tied to it: */
/* submit, pending and collect with the ctx on another stream return          */
/* PBA_E_INVALID (text in pba_ctx_error), enqueue nothing and leave the       */
/* object as it was -- usable once the ctx is back on that stream.  Destroy   */
/* is legal whatever stream the ctx is on: it synchronises the copy stream    */
/* and the recorded stream, which must still exist.                           */
/* ------------------------------------------------------------------------ */
typedef struct pba_loc_stream pba_loc_stream;
enum { PBA_STREAM_TEXT = 0, PBA_STREAM_RECORDS = 1 };
/* The locate parameters are pba_locate's, checked the same way with the same codes (ix a PBA_INDEX_ALL index of
 * target_seq of target, target without bytes outside ACGT, R, kernel); ix and target must outlive the stream.  Each slot
 * takes slot_bytes input bytes and slot_reads reads per batch: a pinned host buffer of slot_bytes and slot_reads + 1 u64
 * offsets (at least 3), the device staging of the bytes, the packed arena and the bit planes with their slack, the
 * offset / length arrays, and a pba_seqs that borrows them.  All or nothing: PBA_E_NOMEM leaves nothing behind. */
int pba_loc_stream_create(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, uint32_t target_seq, double R, int trials,
                          int min_len, int maxn, int maxm, int kernel, uint64_t slot_bytes, uint32_t slot_reads, int form,
                          pba_loc_stream **out);
/* The pinned buffers of the next free slot, to be filled in place.  PBA_STREAM_TEXT: the ASCII of the reads back to back
 * and offsets[0..n] as for pba_seqs_from_text (offsets[0] = 0).  PBA_STREAM_RECORDS: the bytes of a binary read file as
 * pba_seqs_from_records takes them, offsets[0] = the byte count, offsets[1] / offsets[2] = min_excl / max_excl.
 * PBA_E_INVALID when both slots are pending. */
int pba_loc_stream_buffer(pba_loc_stream *s, void **bytes, uint64_t **offsets);
/* Hand the filled slot over as a batch of n reads (n == 0 is a batch; PBA_STREAM_RECORDS: n is not looked at, the batch
 * holds the records the walk of pba_open_binary keeps).  Checked on the host: offsets not non-decreasing PBA_E_INVALID;
 * more bytes than slot_bytes, more reads than slot_reads, or a read beyond the engine limit PBA_E_TOOLONG; a truncated
 * record PBA_E_INVALID.  A refused batch enqueues nothing and leaves the slot free.  Otherwise the copy of the bytes and
 * of the small arrays, the pack and an event are enqueued on the copy stream; nothing is synchronised. */
int pba_loc_stream_submit(pba_loc_stream *s, uint32_t n);
/* The locate of the oldest pending batch (the driver of pba_locate, on the ctx's stream, behind that batch's pack event);
 * *n = its reads, rows[0 .. *n) and stats (nullable) as pba_locate fills them, except that rows[i].read counts from the
 * first read ever submitted to the stream and rows[i].nseq continues the running id of locator.cpp:72,91 across batches:
 * the rows of all batches, concatenated, are the rows of one pba_locate over the concatenated reads.  stats is per batch.
 * A batch with a byte outside ACGT returns PBA_E_ALPHABET (as pba_locate does for such a set) before anything is launched:
 * the batch is dropped, the slot is free, the stream stays usable, and the running `read` and `nseq` counters DO advance
 * by what its reads would have contributed (re-submitted clean, they get new ids).  PBA_E_INVALID with nothing pending or
 * cap below the batch size (the batch stays pending).  After any other failure the stream is spent: every later call
 * returns PBA_E_INVALID; destroy still works. */
int pba_loc_stream_collect(pba_loc_stream *s, pba_loc_row *rows, uint32_t cap, uint32_t *n, pba_loc_stats *stats);
/* The set of the batch collect would run next, borrowed from its slot (valid until that collect; pba_seqs_destroy leaves
 * it alone).  Blocks until the batch's pack has finished.  For pba_align_batch / pba_seqs_export on streamed reads. */
int pba_loc_stream_pending(pba_loc_stream *s, const pba_seqs **set);
/* HIP-event times of the batch collected last: the copy of its bytes, its pack, its locate, and how long the ctx's stream
 * stood at the pack event before the locate could start (near 0 when the upload was hidden behind the batch before) */
typedef struct {
    float h2d_ms, pack_ms, locate_ms, stall_ms;
    uint32_t n_reads;
    uint64_t n_bytes;              /* input bytes copied */
} pba_stream_profile;
int pba_loc_stream_last_profile(const pba_loc_stream *s, pba_stream_profile *out);
/* waits for the copy stream and for the ctx's stream as recorded at create, then frees; legal with batches pending and with
 * the ctx on any stream */
void pba_loc_stream_destroy(pba_loc_stream *s);

/* ------------------------------------------------------------------------ */
/* Streamed mapping: pba_map_reads (many contigs, both strands) on read       */
/* batches that arrive step by step.  The slots, the copy stream and the      */
/* buffer / submit / collect protocol are pba_loc_stream's; with strands & 2  */
/* a slot also holds rc(batch) -- a second packed arena, a second set of bit  */
/* planes and a second borrowed pba_seqs -- written on the copy stream behind */
/* the forward pack: from the same staged ASCII (PBA_STREAM_TEXT) or from the */
/* uploaded file (PBA_STREAM_RECORDS).  No pba_seqs_revcomp, no allocation    */
/* between create and destroy.                                                */
/* ------------------------------------------------------------------------ */
typedef struct pba_map_stream pba_map_stream;
/* The mapping parameters are pba_map_reads', checked the same way with the same codes at the door: ix the
 * pba_index_build_set index of target (same count, same lengths), strands in 1..3, R, kernel; a target with bytes outside
 * ACGT: PBA_E_ALPHABET.  ix and target must outlive the stream.  slot_bytes, slot_reads, form and what a slot holds are
 * pba_loc_stream_create's; with strands == 1 nothing is allocated for the reverse complement.  All or nothing:
 * PBA_E_NOMEM leaves nothing behind. */
int pba_map_stream_create(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, double R, int trials, int min_len,
                          int maxn, int maxm, int kernel, int strands, uint64_t slot_bytes, uint32_t slot_reads, int form,
                          pba_map_stream **out);
/* as pba_loc_stream_buffer */
int pba_map_stream_buffer(pba_map_stream *s, void **bytes, uint64_t **offsets);
/* as pba_loc_stream_submit: the same host checks with the same codes, a refused batch enqueues nothing; behind the forward
 * pack the pack of rc(batch) is enqueued (strands & 2), and one event behind both */
int pba_map_stream_submit(pba_map_stream *s, uint32_t n);
/* pba_map_reads of the oldest pending batch (both walks on the ctx's stream, behind that batch's pack event); *n = its
 * reads, rows[0 .. *n) and stats (nullable, per batch) as pba_map_reads fills them, except that rows[i].read counts from the
 * first read ever submitted and rows[i].nseq continues the running id across batches: the rows of all batches,
 * concatenated, are the rows of one pba_map_reads over the concatenated reads, and every field of stats, summed over the
 * batches, is that call's (strands == 3: the second walk is over the reads this batch's + walk left).  A batch with a byte
 * outside ACGT, the cap, nothing pending and a spent stream: as pba_loc_stream_collect. */
int pba_map_stream_collect(pba_map_stream *s, pba_map_row *rows, uint32_t cap, uint32_t *n, pba_map_stats *stats);
/* Both sets of the batch collect would run next, borrowed from its slot (valid until that collect): *fwd the reads, *rc their
 * reverse complement in pba_seqs_revcomp's layout, NULL with strands == 1.  Blocks until both packs have finished. */
int pba_map_stream_pending(pba_map_stream *s, const pba_seqs **fwd, const pba_seqs **rc);
/* as pba_loc_stream_last_profile: pack_ms covers the packs of both strands, locate_ms both walks */
int pba_map_stream_last_profile(const pba_map_stream *s, pba_stream_profile *out);
/* waits for the copy stream and for the ctx's stream as recorded at create, then frees; legal with batches pending and with
 * the ctx on any stream */
void pba_map_stream_destroy(pba_map_stream *s);

/* ------------------------------------------------------------------------ */
/* All-vs-all overlap.  Not a loop the reference  */
/* has, but built only from its pieces: every read t in [t_lo, t_hi) takes the */
/* reference role (ref_seq::get_seedmap index of t, ref_seq.h:291-311) and     */
/* every other read q is walked like one read of a locked spaced_seed round    */
/* (spaced_seed.cpp:420-437 with the intended seed_at): first       */
/* success per (t, q); every successful pair is reported.                      */
/* ------------------------------------------------------------------------ */
typedef struct {
    int32_t target, query;         /* read ids; target = the `a` side (ref_seq.h:264) */
    int32_t j, dir, ref_pos;       /* probe offset, +1 forward / -1 backward, hit position in the target */
    int32_t cost, matlen_a, matlen_b;
} pba_overlap;

typedef struct {
    uint64_t n_probe_entries;      /* probe keys indexed (2*max_trial per read, zero keys dropped) */
    uint64_t n_candidates;         /* (target position, probe) matches */
    uint64_t n_pairs;              /* candidate pairs handed to the banded DP (stops at the first success per pair of reads) */
    uint64_t n_overlaps;           /* successful (target, query) pairs */
    uint64_t n_redo;               /* (target, query) runs resumed at the reference band (narrow window not certified) */
    float scan_ms, sort_ms, walk_ms;
    uint32_t wide_first;           /* 1: a sample showed the narrow window rarely certifies, the rest went straight to the reference band */
    float table_ms;                /* build of the probe table this call scanned against (once per table, not per call) */
    uint32_t n_big_targets;        /* targets whose candidates outgrew one LDS sort and were cut into pieces of consecutive queries */
    uint64_t n_prefiltered;        /* bit-vector kernels: candidates that failed the reference's diagonal check within their first 32
                                      rows where the scan found them -- pairs the reference aligned and dropped there: counted in
                                      n_pairs, never written (row-sweep kernel: 0, every candidate is written, sorted and walked) */
    uint32_t cap_fill;             /* 1: the survivors' slices were not sized by a census launch first but given equal room, sized by an earlier range of the table */
    uint32_t cap_overflow;         /* 1: a slice outgrew that room and the range was scanned again with exact slices */
    uint64_t n_listed;             /* candidates written, sorted and walked: the survivors of the scan's 32 rows (row-sweep kernel: all) */
} pba_overlap_stats;

/* Limits of the all-vs-all entry points (explicit PBA_E_TOOLONG beyond them, never a wrapped count):
 *   reads                      < PBA_OVL_MAX_READS       (a candidate packs the query id next to 23 bits of probe and ordinal)
 *   reads * 2 * max_trial      < PBA_OVL_MAX_PROBES      (a probe id is 32 bits)
 *   LISTED candidates of ONE call < PBA_OVL_MAX_CANDIDATES (n_listed; offsets into the candidate array are 32 bits: go through the targets
 *                                                         in ranges [t_lo, t_hi) against one probe table -- BASELINE config 5,
 *                                                         10 M reads, takes ~4 000 targets per call)
 *   max_trial                  in [1, 63], read length <= 65 000 */
#define PBA_OVL_MAX_READS (1u << 24)
#define PBA_OVL_MAX_PROBES (1ull << 32)
#define PBA_OVL_MAX_CANDIDATES 0xFFFFFFF0ull

/* out: caller-allocated, cap entries; *n_out = overlaps found (may exceed cap: then only cap are written).
 * Results are sorted by (target, query).  Targets shard across GPUs through [t_lo, t_hi). */
int pba_overlap_all(pba_ctx *ctx, const pba_seqs *reads, uint32_t t_lo, uint32_t t_hi, uint32_t mask, double R,
                    int max_trial, int overlap_min, int kernel, pba_overlap *out, uint64_t cap, uint64_t *n_out,
                    pba_overlap_stats *stats);
/* Multi-GPU form (the one exchange of SURVEY 8e): a rank emits the probe entries of ITS queries [q_lo, q_hi)
 * into a DEVICE buffer (2*max_trial slots per query are enough), the ranks all-gather those buffers over RCCL
 * (slots holding all-ones are padding), and every rank hands the gathered list to pba_overlap_all_probes,
 * which is pba_overlap_all with the probe table given instead of built. */
int pba_overlap_probes(pba_ctx *ctx, const pba_seqs *reads, uint32_t q_lo, uint32_t q_hi, uint32_t mask, int max_trial,
                       void *d_entries, uint64_t cap, uint64_t *n_out);
int pba_overlap_all_probes(pba_ctx *ctx, const pba_seqs *reads, uint32_t t_lo, uint32_t t_hi, const void *d_probe_entries,
                           uint64_t n_probe_slots, uint32_t mask, double R, int max_trial, int overlap_min, int kernel,
                           pba_overlap *out, uint64_t cap, uint64_t *n_out, pba_overlap_stats *stats);
/* The same in two steps, for read sets that go through the targets in many ranges (or many ranks' worth of them): the
 * probe table -- what hash_table is to one reference (common.h:54), for the probes of every read: bucket offsets by key,
 * the probe ids bucket by bucket, one presence bit per key -- is built ONCE from the (gathered) DEVICE entry list and
 * every pba_overlap_all_table call scans its target range against it. */
typedef struct pba_probe_table pba_probe_table;
int pba_probe_table_create(pba_ctx *ctx, const void *d_probe_entries, uint64_t n_probe_slots, uint32_t mask, int max_trial,
                           pba_probe_table **out);
void pba_probe_table_destroy(pba_probe_table *t);
uint64_t pba_probe_table_entries(const pba_probe_table *t);
int pba_overlap_all_table(pba_ctx *ctx, const pba_seqs *reads, uint32_t t_lo, uint32_t t_hi, const pba_probe_table *tab, double R,
                          int overlap_min, int kernel, pba_overlap *out, uint64_t cap, uint64_t *n_out, pba_overlap_stats *stats);

/* Both strands.  A strand +1 overlap of target t and query q is exactly a pba_overlap_all row.  A strand -1 overlap is the
 * same computation with the query's text replaced by rc(q) (pba_seqs_revcomp): its j, dir, ref_pos, cost and match lengths
 * are those of target t against the set of reverse-complemented reads, so j and dir are in rc(q)'s own coordinates.  A read
 * is never paired with itself on either strand.  Each row also carries half-open intervals on the FORWARD strand of each
 * read (spaced_seed.cpp:274-276, ref_seq.h:282-286; slen = the query's length):
 *   dir +1: target [ref_pos, ref_pos + matlen_a),            query [j, j + matlen_b)
 *   dir -1: target [ref_pos + 16 - matlen_a, ref_pos + 16),  query [slen - j - matlen_b, slen - j)
 *   strand -1: the query interval [b0, b1) above is that of rc(q), and is given as [slen - b1, slen - b0). */
typedef struct {
    int32_t target, query, strand;        /* strand +1 / -1 */
    int32_t j, dir, ref_pos;              /* as pba_overlap, in the coordinates of the query text that was walked */
    int32_t cost, matlen_a, matlen_b;
    int32_t t_beg, t_end, q_beg, q_end;   /* half-open, forward strand of each read */
} pba_strand_overlap;

/* strands: 1 = +1 only, 2 = -1 only, 3 = both.  reads_rc: rc of every read of `reads` (pba_seqs_revcomp with flip == NULL),
 * or NULL to have it built inside.  A reads_rc of another count or other lengths is refused (PBA_E_INVALID); one with the
 * same lengths but other bases cannot be told apart cheaply and gives the -1 rows of whatever it holds.  Rows sorted by
 * (target, query, strand), +1 before -1.  stats[0] / stats[1]: the +1 / -1 pass.  Same limits as pba_overlap_all; cap
 * bounds the rows of each pass and of the merged list: *n_out = rows found on both strands (may exceed cap: then only cap
 * are written).  PBA_E_ALPHABET for sets with bytes outside ACGT. */
int pba_overlap_strands(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                        uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands,
                        pba_strand_overlap *out, uint64_t cap, uint64_t *n_out, pba_overlap_stats stats[2]);
/* The range / multi-GPU form: tab_fwd built from pba_overlap_probes(reads, ...) entries, tab_rc from
 * pba_overlap_probes(reads_rc, ...) entries (either may be NULL to skip that strand; tab_rc needs reads_rc).  A rank
 * reverse-complements its gathered read set locally and emits the probes of its rc queries: no new exchange.  A table
 * belongs to the set whose probes filled it. */
int pba_overlap_strands_table(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                              const pba_probe_table *tab_fwd, const pba_probe_table *tab_rc, double R, int overlap_min,
                              int kernel, pba_strand_overlap *out, uint64_t cap, uint64_t *n_out,
                              pba_overlap_stats stats[2]);

/* ------------------------------------------------------------------------ */
/* Read correction from overlap pile-ups.  Not a loop the reference has, but  */
/* built only from its pieces: every read t takes the reference role          */
/* (ref_seq(T, len, false, weight), ref_seq.h:218-225: one vote box per base), */
/* every overlap row of t is re-aligned with traceback and its path voted      */
/* (elect / apply_edits, ref_seq.h:25-41, 352-362), and evolve()              */
/* (ref_seq.h:317-349) gives the corrected read.  NO GROWTH: append / prepend  */
/* (ref_seq.h:268-275) are not applied, the text the votes address is T        */
/* throughout, so votes commute and the order of the rows does not matter.     */
/* ------------------------------------------------------------------------ */
/* Host arithmetic, no ctx: the pair of accessors a row stands for, as a locked spaced_seed round forms them
 * (spaced_seed.cpp:274-285, ref_seq.h:282-286; slen = query_len):
 *   dir +1: a forward from ref_pos, a_len = target_len - ref_pos;       b forward from j, b_len = slen - j
 *   dir -1: a backward from ref_pos + 15, a_len = ref_pos + 16;         b backward from slen - j - 1, b_len = slen - j
 * a_seq = row->target, b_seq = row->query: for a strand -1 row b indexes the set of reverse-complemented reads (the row's
 * j and dir are in rc(q)'s coordinates already).  PBA_E_INVALID for a NULL, a strand or dir other than +1 / -1, or
 * lengths that put an accessor outside its read. */
int pba_overlap_row_pair(const pba_strand_overlap *row, uint32_t target_len, uint32_t query_len, pba_pair *out);

/* The vote boxes of reads [t_lo, t_hi) in one device arena, one segment per target (no margins: there is no growth), filled
 * on the device from the packed set.  20 bytes per base.  The counters are u16 halves bumped with 32-bit atomics on their
 * dword: a selection counter holds weight + votes <= 65 535 (a vote beyond that would carry into the neighbouring counter
 * instead of wrapping like the reference's unsigned short), so keep weight small next to 65 535 - coverage.  Box indices are 32-bit inside the kernels: a range of 2^31 bases or more is refused with PBA_E_TOOLONG
 * (pba_correct_reads goes through such a range in chunks).  weight: the selection count of the read's own base, in
 * [1, 0xFFFF] (with 0 a read without rows would evolve to nothing).  `reads` may be any set, a set of contigs included: a
 * pile-up with a segment of more than 65 536 boxes is filled and evolved tile by tile (4 096 boxes per workgroup), byte for
 * byte what the per-target kernels give. */
typedef struct pba_pileup pba_pileup;
int pba_pileup_create(pba_ctx *ctx, const pba_seqs *reads, uint32_t t_lo, uint32_t t_hi, int weight, pba_pileup **out);
void pba_pileup_destroy(pba_pileup *p);
/* Vote n rows (any order, any mix of strands, any number of calls; every row's target in [t_lo, t_hi)).  reads is the set
 * the pile-up was made from, reads_rc its reverse complement (pba_seqs_revcomp; may be NULL if no row has strand -1).
 * res[k] (nullable) as pba_align_batch returns it.  Everything that can be checked on the host -- targets, strands,
 * accessors inside their reads, the sets -- is checked before any vote: PBA_E_INVALID / PBA_E_ALPHABET leave the boxes as
 * they were.  A row whose re-run disagrees with its cost / matlen_a / matlen_b (the rows are not overlaps of these sets
 * under this R) is PBA_E_INVALID too, text in pba_ctx_error, but is found after the batch has voted: the pile-up is spent.
 * The +1 rows and the -1 rows of a call are two batches.  A batch can still be refused where the host checks end --
 * PBA_E_TOOLONG (band too wide for the voting kernel), PBA_E_NOMEM, PBA_E_HIP: if that happens after a batch of the call
 * has voted, or with any status other than PBA_E_TOOLONG / PBA_E_INVALID, the boxes may hold part of the call's votes and the
 * pile-up is spent as well (do not retry on it: make a new one). */
int pba_pileup_vote(pba_ctx *ctx, pba_pileup *p, const pba_seqs *reads, const pba_seqs *reads_rc,
                    const pba_strand_overlap *rows, uint64_t n, double R, pba_result *res);
/* the boxes of one target as they stand (before evolve), layout of pba_cons_dump */
int pba_pileup_dump(pba_ctx *ctx, const pba_pileup *p, uint32_t target, uint16_t *sel, uint16_t *sup, int32_t *tot, int cap,
                    int32_t *n);
typedef struct {
    int32_t target, n_rows;        /* rows voted into this target */
    int32_t len_in, len_out;
} pba_correct_row;
/* evolve every segment: the corrected reads as a NEW set (sequence k = target t_lo + k, pba_seqs_from_text's layout; a
 * zero-length result is legal), written and packed on the device; rows_out (nullable): t_hi - t_lo entries.  Afterwards the
 * pile-up is spent: its boxes are released, further vote / dump / evolve calls return PBA_E_INVALID. */
int pba_pileup_evolve(pba_ctx *ctx, pba_pileup *p, pba_seqs **corrected, pba_correct_row *rows_out);
/* The whole thing for targets [t_lo, t_hi): overlaps on the strands asked for (pba_overlap_strands, same arguments, limits
 * and stats, summed over the chunks), vote, evolve.  The range is cut into chunks of consecutive targets so that the boxes
 * (20 bytes per base, at most a quarter of the free device memory and fewer than 2^31 boxes) sit next to what the overlap
 * call needs; a chunk the overlap call finds too large is halved.  The answer does not depend on the cut.
 * The rows voted are the engine's own: should one not re-run to itself, that is an inconsistency inside the engine, not a bad
 * argument, and is reported as PBA_E_HIP (text in pba_ctx_error), never as PBA_E_INVALID. */
int pba_correct_reads(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                      uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                      pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2]);
/* The same with a ceiling on the boxes of one chunk (max_boxes bases; 0 = none): for a caller that shares the device with
 * other allocations and wants the pile-up smaller than a quarter of what is free.  A chunk always holds at least one read. */
int pba_correct_reads_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                             uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                             uint64_t max_boxes, pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2]);
/* HIP-event timings (on the ctx's stream) of the most recent pba_correct_reads on this ctx, summed over its chunks */
typedef struct {
    float overlap_ms, vote_ms, evolve_ms;
    uint32_t n_chunks;
    uint64_t n_rows;               /* rows voted */
    uint64_t n_bases_in, n_bases_out;
} pba_correct_profile;
int pba_ctx_last_correct_profile(const pba_ctx *ctx, pba_correct_profile *out);

/* ------------------------------------------------------------------------ */
/* Polishing a contig set from its mapped reads: the reads pba_map_reads      */
/* places on a contig vote on that contig, evolve gives the next contig, and  */
/* the loop repeats -- what ref_seq::try_align + evolve do for one growing    */
/* reference (ref_seq.h:259-276, 317-349), for a whole set at once.           */
/* ------------------------------------------------------------------------ */
/* Host arithmetic, no ctx: the pair a found pba_map_row votes with, in try_align's roles (ref_seq.h:264: the boxes belong to
 * a, the voted characters are b's) -- the mapper found the row with the read as a and the contig as b (locator.cpp:78-82):
 *   a_seq = row->contig, forward from row->pos;  b_seq = row->read, forward from row->j, b_len = read_len - j
 *   a_len = min(contig_len - pos, b_len + max_dst), max_dst = 1 + (int)(b_len * R)
 * For a strand -1 row b indexes the set of reverse-complemented reads (j is in rc(read)'s coordinates already).  The clip of
 * a loses nothing: align itself cuts len_a to len_b + max_dst whenever a is the longer side (seq_aligner.h:94-102), and the
 * clipped length stays above b_len, so the same branch is taken; it is made here because an accessor is limited to 65 000
 * elements and a contig remainder is megabases long.  PBA_E_INVALID: a NULL, found == 0, a strand other than +1 / -1, j or
 * pos outside its sequence, R outside (0, 1).  PBA_E_TOOLONG: an accessor (the clipped a, or b) beyond the engine's limit. */
int pba_map_row_pair(const pba_map_row *row, uint32_t contig_len, uint32_t read_len, double R, pba_pair *out);
/* Vote n pba_map_reads rows into p = pba_pileup_create(ctx, target, c_lo, c_hi, weight): `target` is the contig set the
 * pile-up was made from (count and lengths are checked), reads / reads_rc the sets the rows were mapped from (reads_rc may
 * be NULL if no row has strand -1).  Rows with found == 0 are skipped (res[k] zeroed, rc = -1); every other row's contig
 * must lie in [c_lo, c_hi).  The +1 rows and the -1 rows are two batches.  The gate is try_align's (ref_seq.h:264-265): a
 * pair votes if and only if it aligns (rc >= 0) with matlen_a >= overlap_min.  The alignment has its roles swapped against
 * the one the mapper ran, so it is NOT held to the row's cost or match lengths: a found row may legitimately not vote.
 * res[k] (nullable) as pba_align_batch returns it; *n_voted (nullable) = rows that voted; the per-target n_rows that
 * pba_pileup_evolve reports count voted rows only.  No growth (append / prepend are not applied), so votes commute.
 * Everything the host can check -- range, sets, accessors, PBA_E_ALPHABET, PBA_E_TOOLONG -- is checked before any vote and
 * leaves the boxes as they were; after a later failure the pile-up is spent under the rules of pba_pileup_vote. */
int pba_pileup_vote_mapped(pba_ctx *ctx, pba_pileup *p, const pba_seqs *target, const pba_seqs *reads,
                           const pba_seqs *reads_rc /* nullable if no row has strand -1 */, const pba_map_row *rows, uint64_t n,
                           double R, int overlap_min, pba_result *res /* nullable */, uint64_t *n_voted /* nullable */);
/* ------------------------------------------------------------------------ */
/* How a mapped read or an overlap aligns: run-length alignments per row,     */
/* for PAF with a cg:Z: tag (what the reference's visual_align.cpp shows).    */
/* ------------------------------------------------------------------------ */
/* Host arithmetic, no ctx: the pair the mapper itself aligned for a found row (locator.cpp:78-82), roles as it had them:
 *   a_seq = row->read, forward from row->j, rest of the read;  b_seq = row->contig, forward from row->pos, rest of the contig
 *   each side clipped to the other side's length + ITS max_dst, exactly as align clips it (seq_aligner.h:94-102)
 * For a strand -1 row a indexes the set of reverse-complemented reads.  The clip never changes which branch of
 * seq_aligner.h:94 is taken: with b the longer side (len_b >= len_a) it is cut to len_a + max_dst >= len_a, with a the
 * longer one to len_b + max_dst > len_b, so align on the clipped pair takes the same branch, derives the same max_dst and
 * clips to the same lengths again.  It is made here because an accessor holds at most 65 000 elements and a contig remainder
 * is megabases long.  Refusals as pba_map_row_pair's. */
int pba_map_row_aln_pair(const pba_map_row *row, uint32_t contig_len, uint32_t read_len, double R, pba_pair *out);
/* The alignments of n pba_map_reads rows as runs: SAM's CIGAR, the read (rc(read) for strand -1) is the query, the contig
 * forward the reference, runs origin-first.  Rows with found == 0 get no runs (counts and res zeroed, res rc = -1).  Every
 * other row is re-run in the mapper's own roles (pba_map_row_aln_pair) and IS held to the row's cost, matlen_a and matlen_b:
 * a disagreement is PBA_E_INVALID with text in pba_ctx_error.  cig_off (n + 1 entries) is always complete and *n_slots the
 * total; the runs of row k go to cigar[cig_off[k] ..) for the rows, in order, up to the first whose end exceeds cap.  counts
 * and res (n entries each) are nullable.  The rows go through the device in chunks whose bounded slots
 * (pba_cigar_bound) stay under a fixed budget (2^28 slots) or, in the _budget form, under max_slots (0 = the default; a
 * chunk holds at least one row); each chunk's runs are compacted on the device before they are copied.  The answer does not
 * depend on the cut.  reads_rc may be NULL if no row has strand -1. */
int pba_map_rows_cigar(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                       const pba_map_row *rows, uint64_t n, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off,
                       uint64_t *n_slots, pba_aln_counts *counts, pba_result *res);
int pba_map_rows_cigar_budget(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                              const pba_map_row *rows, uint64_t n, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off,
                              uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots);
/* The same for pba_strand_overlap rows: the pair is pba_overlap_row_pair's (a = the target), the query read is the CIGAR's
 * query (PBA_CIG_B_IS_QUERY; for strand -1 its text is rc(q), as the row defines it) and the runs are in the target's
 * forward order: origin-first for dir +1, goal-first (PBA_CIG_REVERSED) for dir -1.  Held to the row's cost and match
 * lengths. */
int pba_overlap_rows_cigar(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                           uint64_t n, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off, uint64_t *n_slots,
                           pba_aln_counts *counts, pba_result *res);
int pba_overlap_rows_cigar_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                  uint64_t n, double R, uint32_t *cigar, uint64_t cap, uint64_t *cig_off, uint64_t *n_slots,
                                  pba_aln_counts *counts, pba_result *res, uint64_t max_slots);

/* ------------------------------------------------------------------------ */
/* Per-window alignment counts, and rows trimmed where they break (DESIGN    */
/* 5.11; tests/windows_ref.py restates all of this in plain Python).  The a  */
/* sequence of a pair carries a grid of W-base windows fixed on ITS OWN      */
/* coordinates: a-element e lies at x(e) = a_pos + e (forward accessor) or   */
/* a_pos - e (backward), g(e) = x(e) div W, and the pair's local window      */
/* index is w(e) = |g(e) - g(0)|.  Windows of different pairs on one         */
/* sequence coincide.  Of a successful pair's script (origin-first):         */
/*   MATCH / DELETE consuming a-element e      -> window w(e)                 */
/*   INSERT met after i a-elements were consumed -> window w(max(i - 1, 0))   */
/* A window is one pba_aln_counts: = / X per element, I / D named as         */
/* pba_align_batch_cigar names them (PBA_CIG_B_IS_QUERY exchanges them).     */
/* n_win = w(max(matlen_a - 1, 0)) + 1; a pair with rc < 0 has none.  The    */
/* windows sum to the pair's counts, every window consumes at least one      */
/* a-element (matlen_a >= 1) and interior windows consume exactly W.         */
/* Origin-first, or goal-first under PBA_CIG_REVERSED.                       */
/* ------------------------------------------------------------------------ */
/* Host arithmetic: the windows the clipped len_a (seq_aligner.h:94-102) of a pair touches, which bounds n_win.  0 for W < 1,
 * a negative length or position, R outside (0,1) or a backward accessor that would start before position 0. */
uint32_t pba_windows_bound(int a_pos, int a_len, int b_len, double R, int W, int a_backward);
/* The host twin of the device sink, shaped like pba_cigar_from_script: the windows of a script and the elements of its two
 * accessors in element order.  Returns n_win (the first min(n_win, cap) written), -1 for an op outside 1..3, W < 1 or
 * unknown flag bits.  An empty script has one empty window. */
int pba_windows_from_script(const uint8_t *ops, int32_t nedit, const char *a_elems, const char *b_elems, int a_pos, int a_backward,
                            int W, uint32_t flags, pba_aln_counts *win, int32_t cap);
/* The windows of a batch, made on the device by the traceback walk (no script, no CIGAR in memory).  Pair q's windows go to
 * win[win_off[q] ..), nwin[q] of them; win_off (n + 1 entries) must leave pba_windows_bound(...) slots per pair, else
 * PBA_E_INVALID.  A pair with rc < 0: nwin = 0, its slot untouched, counts zero.  counts[q]: the pair's totals, as
 * pba_align_batch_cigar gives them.  Refusals and the alphabet rule as pba_align_batch_cigar; W < 1: PBA_E_INVALID. */
int pba_align_batch_windows(pba_ctx *ctx, const pba_seqs *A, const pba_seqs *B, const pba_pair *pairs, size_t n, double R, int maxn,
                            int maxm, int W, uint32_t flags, pba_result *out, pba_aln_counts *win, const uint64_t *win_off,
                            int32_t *nwin, pba_aln_counts *counts);
/* The windows of rows: the same re-run pairs, roles and order as pba_map_rows_cigar / pba_overlap_rows_cigar (the grid lies on
 * the read for mapped rows -- a is the read --, on the TARGET for overlap rows, whose windows come in the target's forward order,
 * I / D named with the query read as the query), held to the row's cost and match lengths.  Dense and in row order: row k's
 * windows at win[win_off[k] .. win_off[k + 1]) for the rows, in order, up to the first whose end exceeds cap; win_off (n + 1)
 * is always complete and *n_slots the total.  The rows go through the device in chunks whose bounded slots
 * (pba_windows_bound) stay under max_slots windows (0: 2^26; a chunk holds at least one row); the answer does not depend on
 * the cut.  counts / res nullable. */
int pba_map_rows_windows(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_map_row *rows,
                         uint64_t n, double R, int W, pba_aln_counts *win, uint64_t cap, uint64_t *win_off, uint64_t *n_slots,
                         pba_aln_counts *counts, pba_result *res);
int pba_map_rows_windows_budget(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                                const pba_map_row *rows, uint64_t n, double R, int W, pba_aln_counts *win, uint64_t cap,
                                uint64_t *win_off, uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots);
int pba_overlap_rows_windows(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                             double R, int W, pba_aln_counts *win, uint64_t cap, uint64_t *win_off, uint64_t *n_slots,
                             pba_aln_counts *counts, pba_result *res);
int pba_overlap_rows_windows_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                    uint64_t n, double R, int W, pba_aln_counts *win, uint64_t cap, uint64_t *win_off,
                                    uint64_t *n_slots, pba_aln_counts *counts, pba_result *res, uint64_t max_slots);

/* The trim rule, per item, over its windows in the order given, I / D named AS UNDER THE DEFAULT FLAGS (I consumes a):
 *   na_k = n_eq + n_x + n_ins, nb_k = n_eq + n_x + n_del, err_k = n_x + n_ins + n_del
 *   good     window k is good when err_k <= thr[na_k], thr[m] = (int32_t)(max_err * (double)m), computed on the host in FP64
 *   runs     the maximal runs of consecutive good windows (n_runs; n_good windows in them); the winner has the largest sum
 *            of na, a tie goes to the first run in the order given
 *   state    DROPPED without a run, with a winner whose na sum is below min_span, or whose nb sum is 0 (every other field but
 *            n_win, n_good, n_runs is 0 then); WHOLE when the winner is all windows; else CUT
 *   reported the winner [w_beg, w_end), the a- and b-elements before it (a0, b0) and inside it (na, nb), cost = its err sum */
enum { PBA_TRIM_DROPPED = 0, PBA_TRIM_WHOLE = 1, PBA_TRIM_CUT = 2 };
typedef struct { int32_t state, n_win, n_good, n_runs, w_beg, w_end, a0, b0, na, nb, cost; } pba_trim_span;
/* The trim kernel on windows the caller supplies (item q: win[win_off[q] .. win_off[q + 1])), so that the rule can be pinned
 * apart from the aligner.  PBA_E_INVALID for W < 1, max_err outside [0, 1], min_span < 0, offsets that decrease, a negative
 * count or a window with na_k > W.  No items are legal. */
int pba_windows_trim(pba_ctx *ctx, const pba_aln_counts *win, const uint64_t *win_off, uint64_t n, int W, double max_err, int min_span,
                     pba_trim_span *spans);
/* Overlap rows trimmed to the longest run of good target windows.  The windows are made as pba_overlap_rows_windows makes
 * them (target forward) and judged by the trim kernel on the device: no window crosses the host.  With a0, b0, na, nb
 * counted in ELEMENT order (the reverse of the target's order for dir -1), j, dir, slen as pba_strand_overlap defines them:
 *   target            dir +1: [t_beg + a0, t_beg + a0 + na)            dir -1: [t_end - a0 - na, t_end - a0)
 *   walked query text dir +1: [j + b0, j + b0 + nb)                    dir -1: [slen - j - b0 - nb, slen - j - b0)
 *   strand -1: a walked query interval [w0, w1) is given as [slen - w1, slen - w0)
 * They lie inside the row's own intervals.  A DROPPED row's four ends are 0. */
typedef struct { int32_t state, n_win, n_good, n_runs, w_beg, w_end, t_beg, t_end, q_beg, q_end, cost; } pba_trim_row;
typedef struct {
    uint64_t n_rows, n_windows;
    uint32_t n_whole, n_cut, n_dropped, n_chunks;
    float windows_ms, trim_ms;          /* HIP events on the ctx's stream: the traced passes, the trim kernels */
} pba_trim_stats;
int pba_overlap_rows_trim(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                          double R, int W, double max_err, int min_span, pba_trim_row *out, pba_trim_stats *stats /* nullable */);
int pba_overlap_rows_trim_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                 uint64_t n, double R, int W, double max_err, int min_span, pba_trim_row *out,
                                 pba_trim_stats *stats /* nullable */, uint64_t max_slots);
/* Host: the rows that are not DROPPED, in order, with their four interval ends replaced by the trimmed ones; returns their
 * number (out_rows holds up to n; may alias rows), -1 for a NULL.  These are INTERVAL ROWS: valid for pba_clip_create, which
 * reads only target, query, strand and the four ends; NOT valid for anything that re-runs the alignment from j / ref_pos
 * (pba_*_rows_cigar, pba_*_rows_windows, votes, layout): j, dir, ref_pos, cost and the match lengths are the untrimmed row's. */
int64_t pba_trim_rows_apply(const pba_strand_overlap *rows, const pba_trim_row *trims, uint64_t n, pba_strand_overlap *out_rows);

typedef struct { int32_t contig, n_rows, len_in, len_out; } pba_polish_row;     /* per contig, last round */
typedef struct {
    int32_t round;                 /* 1-based */
    uint32_t n_mapped, n_voted, n_chunks;   /* found rows, rows that voted, pile-ups of the round */
    uint64_t n_bases_in, n_bases_out;
    float index_ms, map_ms, vote_ms, evolve_ms;   /* HIP events on the ctx's stream */
} pba_polish_round_log;
/* `rounds` (>= 1) times: pba_index_build_set of the current contigs, pba_map_reads of the reads on them (R, trials, min_len,
 * maxn, maxm, kernel, strands as there), pile-ups over consecutive contig ranges (the budget of pba_correct_reads: 20 bytes
 * per base, a quarter of the free device memory, fewer than 2^31 boxes; a range always holds at least one contig, and a
 * single contig whose boxes do not fit is PBA_E_NOMEM), pba_pileup_vote_mapped of each range's rows, evolve, and the texts
 * stitched into the next set on the device.  *polished: the contigs after the last round as a NEW set, contig ids
 * unchanged: a contig that evolves to nothing stays as an empty contig, one without voted rows comes back as it was.  The
 * caller's target is never modified.  reads_rc: pba_seqs_revcomp(reads, NULL), or NULL to have it built once inside when
 * strands include -1.  rows_out (nullable): one entry per contig, of the last round.  log (nullable with log_cap 0): entry
 * k describes round k + 1, up to log_cap.  The answer does not depend on how the contigs are cut into ranges. */
int pba_polish_contigs(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc /* nullable */,
                       uint32_t mask, double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands,
                       int overlap_min, int weight, int rounds, pba_seqs **polished, pba_polish_row *rows_out,
                       pba_polish_round_log *log, int log_cap);
/* The same with a ceiling on the boxes of one range (max_boxes bases; 0 = none), as pba_correct_reads_budget */
int pba_polish_contigs_budget(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc /* nullable */,
                              uint32_t mask, double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands,
                              int overlap_min, int weight, int rounds, uint64_t max_boxes, pba_seqs **polished,
                              pba_polish_row *rows_out, pba_polish_round_log *log, int log_cap);

/* ------------------------------------------------------------------------ */
/* Layout: reads into contigs from their overlap rows (overlap -> LAYOUT ->   */
/* consensus).  Not a step the reference has -- it grows one reference, read  */
/* by read (spaced_seed.cpp:409-452) -- but built on the rows its walk gives: */
/* every pba_strand_overlap row is a semi-global alignment from a probe near  */
/* one end of the query to the end of one of the two reads                    */
/* (spaced_seed.cpp:420-437, seq_aligner.h:94-102), so it is a containment or */
/* a dovetail.  A best-overlap graph: one winning dovetail per read end,      */
/* mutual winners are mates, chains of mates are contigs.  DESIGN §5.6 has    */
/* the semantics in full; tests/layout_ref.py restates them.                  */
/* ------------------------------------------------------------------------ */
typedef struct pba_layout pba_layout;
enum { PBA_LAY_UNPLACED = 0, PBA_LAY_PLACED = 1, PBA_LAY_CONTAINED = 2 };
typedef struct {
    int32_t read, state;
    int32_t contig, rank, orient;   /* PLACED: contig id, position in its chain, 0 = as given / 1 = reverse-complemented */
    int32_t offset, skip, adv;      /* PLACED: first contig base it supplies, bases of the walked read skipped, bases supplied */
    int32_t container;              /* CONTAINED: the read that contains it; else -1 */
} pba_layout_row;                   /* not PLACED: contig -1, rank / orient / offset / skip / adv 0 */
typedef struct {
    /* n_rows = n_internal + n_contain (accepted) + n_contain_refused + n_dovetail; n_dovetail_dropped of the dovetails touch a contained read */
    uint64_t n_rows, n_internal, n_contain, n_contain_refused, n_dovetail, n_dovetail_dropped;
    /* n_mated_ends: read ends with a mate before the cycles are cut; n_cycles: cycles cut (each once, not once per direction) */
    uint32_t n_contained, n_mated_ends, n_cycles, n_contigs, n_placed, n_unplaced;
    uint64_t n_bases;               /* bases of all contigs */
    float classify_ms, chain_ms, stitch_ms;   /* HIP events on the ctx's stream; stitch_ms is filled by pba_layout_stitch */
} pba_layout_stats;
/* The layout of `reads` from n_rows overlap rows (host array, any order; only target, query, strand, cost and the four
 * interval ends are read).  hang: the largest overhang a row may leave on the shorter side of either end and still count
 * (beyond it the row is internal and ignored); min_reads: chains of fewer reads stay PBA_LAY_UNPLACED.  The rows go to the
 * device once; classification, the best edge of every read end (u64 atomicMax of length, cost, row index: the longest
 * interval, then the lowest cost -- taken within [0, 65535] --, then the lowest row index), mates, chains (pointer jumping
 * over the 2 * n states (read, orientation)), cycle cuts and the per-read table all run there; the host scans the head flags
 * into contig ids (ascending head read).  Checked on the host before anything is uploaded: PBA_E_INVALID for target == query, an id
 * outside the set, an interval empty or outside its read, a strand other than +1 / -1, hang < 0, min_reads < 1;
 * PBA_E_TOOLONG for 2^32 rows or more (a key holds 32 bits of row index), 2^28 reads or more, a read of more than 65 535
 * bases (16 bits of length), or a contig of 0x7FFFFFF0 bases or more.  No reads and no rows are legal: no contigs. */
int pba_layout_create(pba_ctx *ctx, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows, int hang,
                      int min_reads, pba_layout **out, pba_layout_stats *stats /* nullable */);
/* the per-read table, out[r] for read r; cap below the number of reads: PBA_E_INVALID */
int pba_layout_rows(pba_ctx *ctx, const pba_layout *lay, pba_layout_row *out /* one per read */, uint32_t cap);
uint32_t pba_layout_contigs(const pba_layout *lay);
/* per contig (any array nullable): the read its canonical traversal starts at, its reads, its bases; cap below the number
 * of contigs: PBA_E_INVALID */
int pba_layout_contig_info(const pba_layout *lay, int32_t *head_read, int32_t *n_reads, int32_t *length, uint32_t cap);
/* The contigs as a NEW set: contig base offset + p of a PLACED read is base skip + p of the read, or of its reverse
 * complement where orient == 1 (reversed, code ^ 3), for p in [0, adv).  ASCII is written on the device from the packed
 * arena and packed by pba_seqs_from_device_text: byte for byte what pba_seqs_from_text makes of the same texts.  `reads` must
 * be the set the layout was made from (another count or other lengths: PBA_E_INVALID); PBA_E_ALPHABET for a set with bytes
 * outside ACGT (no complement, as pba_seqs_revcomp). */
int pba_layout_stitch(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, pba_seqs **contigs);
int pba_layout_last_stats(const pba_layout *lay, pba_layout_stats *out);
void pba_layout_destroy(pba_layout *lay);

/* ------------------------------------------------------------------------ */
/* Placement and consensus of a layout (overlap -> layout -> PLACE -> VOTE   */
/* -> evolve; DESIGN §5.7, tests/place_ref.py restates the rule).  An overlap */
/* row ties its query to its target at an exact base: the first pair of      */
/* elements its alignment compared (pba_overlap_row_pair).  Where the target */
/* is PLACED and SUPPLIES that base to its contig, the base has a contig     */
/* coordinate, and the query -- contained reads included -- can vote on the  */
/* contig from there with try_align's gate, with no index and no mapper.     */
/* ------------------------------------------------------------------------ */
typedef struct {
    int32_t read, found;          /* found 0: no eligible row; every other field 0, contig -1 */
    uint32_t row;                 /* index of the winning row */
    int32_t contig, pos, dir;     /* anchor base on the contig; +1 forward / -1 backward (both accessors) */
    int32_t strand, j;            /* b = the read (+1) or its reverse complement (-1), anchor index in that text */
} pba_place_row;
typedef struct {
    /* n_rows = n_target_not_placed + n_outside (the anchor is not a base the target supplies) + n_eligible */
    uint64_t n_rows, n_target_not_placed, n_outside, n_eligible;
    /* reads with a placement, and of those the PLACED / CONTAINED / UNPLACED reads of the layout */
    uint32_t n_found, n_found_placed, n_found_contained, n_found_unplaced;
    float place_ms;               /* HIP events on the ctx's stream */
} pba_place_stats;
/* One placement per read from n_rows overlap rows (host array, any order, not necessarily the rows the layout was made
 * from; target, query, strand, dir, cost and the four interval ends are read).  With lt / lq the lengths of target t and
 * query q and T the layout's row of t:
 *   walked query interval  strand +1: [qb, qe) = [q_beg, q_end);  strand -1: [lq - q_end, lq - q_beg)
 *   anchor                 dir +1: xa = t_beg, yb = qb;           dir -1: xa = t_end - 1, yb = qe - 1
 *   eligible               T.state == PBA_LAY_PLACED and T.skip <= at < T.skip + T.adv, at = xa (T.orient 0) / lt - 1 - xa (1)
 *   on the contig          contig = T.contig, pos = T.offset + at - T.skip;
 *                          orient 0: dir, strand, j = yb;  orient 1 (the contig holds rc(t)): -dir, -strand, j = lq - 1 - yb
 * Among the eligible rows of a query the largest (q_end - q_beg, -cost within [0, 65535], -row index) wins: the key of the
 * layout's best edges.  The query may be in any state.  The rows go to the device once (the ctx's pooled row buffer); a lane
 * per row decides eligibility and does a u64 atomicMax into its query's slot, a lane per read writes its row; the work
 * arrays are pooled, nothing is allocated in a repeated call.  `reads` must be the set the layout was made from.  Checked on
 * the host before anything is uploaded, as pba_layout_create checks its rows; also PBA_E_INVALID: a dir other than +1 / -1,
 * a set of another count or other lengths, cap below the number of reads.  No rows and no reads are legal. */
int pba_layout_place(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows,
                     pba_place_row *out /* one per read */, uint32_t cap, pba_place_stats *stats /* nullable */);
/* Host arithmetic, no ctx: the pair a found placement votes with, in try_align's roles (a = the contig, b = the read):
 *   dir +1: a forward from pos,  remainder contig_len - pos;  b forward from j,  b_len = read_len - j
 *   dir -1: a backward from pos, remainder pos + 1;           b backward from j, b_len = j + 1 (PBA_A_BACKWARD | PBA_B_BACKWARD)
 *   a_len = min(remainder, b_len + max_dst), max_dst = 1 + (int)(b_len * R): the clip of pba_map_row_pair
 * For strand -1 b indexes the set of reverse-complemented reads.  PBA_E_INVALID: a NULL, found == 0, a dir or strand other
 * than +1 / -1, pos or j outside its sequence, R outside (0, 1).  PBA_E_TOOLONG: an accessor beyond the engine's limit. */
int pba_place_row_pair(const pba_place_row *row, uint32_t contig_len, uint32_t read_len, double R, pba_pair *out);
/* The twin of pba_pileup_vote_mapped for placement rows: p = pba_pileup_create(ctx, contigs, c_lo, c_hi, weight), any contig
 * set and any placement rows (not only a layout's).  Rows with found == 0 are skipped (res[k] zeroed, rc = -1); every other
 * row's contig must lie in [c_lo, c_hi).  The +1 rows and the -1 rows are two batches; a pair votes if and only if it aligns
 * (rc >= 0) with matlen_a >= overlap_min.  Checks, *n_voted, res and the rules of a spent pile-up as there. */
int pba_pileup_vote_placed(pba_ctx *ctx, pba_pileup *p, const pba_seqs *contigs, const pba_seqs *reads,
                           const pba_seqs *reads_rc /* nullable if no row has strand -1 */, const pba_place_row *rows, uint64_t n,
                           double R, int overlap_min, pba_result *res /* nullable */, uint64_t *n_voted /* nullable */);
typedef struct {
    pba_place_stats place;         /* of the one pba_layout_place (place.place_ms: its time) */
    uint64_t n_voted;              /* placements that voted */
    uint64_t n_bases_in, n_bases_out;
    uint32_t n_chunks, n_contigs;
    float stitch_ms, vote_ms, evolve_ms;   /* HIP events on the ctx's stream */
} pba_layout_cons_stats;
/* The consensus of a layout's contigs: pba_layout_stitch, pba_layout_place of `rows`, then pile-ups over consecutive contig
 * ranges (the budget of pba_polish_contigs: 20 bytes per base, a quarter of the free device memory, fewer than 2^31 boxes,
 * max_boxes where it is not 0; a range always holds at least one contig, and a single contig whose boxes do not fit is
 * PBA_E_NOMEM), pba_pileup_vote_placed of each range's placements, evolve, and the texts stitched into *consensus on the
 * device.  ONE round: a placement addresses the stitched text and evolve moves the coordinates; further rounds are
 * pba_polish_contigs'.  Contig ids are unchanged, a contig without votes comes back as it was, and the answer does not
 * depend on the cut.  reads_rc: pba_seqs_revcomp(reads, NULL), or NULL to have it built inside when a placement needs it.
 * rows_out (nullable): one entry per contig. */
int pba_layout_consensus(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, const pba_seqs *reads_rc /* nullable */,
                         const pba_strand_overlap *rows, uint64_t n_rows, double R, int overlap_min, int weight, uint64_t max_boxes,
                         pba_seqs **consensus, pba_polish_row *rows_out /* nullable */, pba_layout_cons_stats *stats /* nullable */);

/* ------------------------------------------------------------------------ */
/* Per-base evidence and Phred qualities of an evolved set; FASTQ out        */
/* (tests/qual_ref.py restates the rule).  Evolve decides      */
/* every output character from a vote box (sel, sup, tot).  The *_qual calls */
/* below keep, for every character, what the box said.  A pile-up is fresh:  */
/* sel = weight on the target's own base, sup = 0, tot = 1.  For box i       */
/* (input position i) of a target, w the pile-up's weight:                   */
/*   N = tot - 1 + w: the rows that consumed the box by MATCH or DELETE      */
/*   plus the weight of the target's own base (the weight counts as w        */
/*   observations);                                                           */
/*   the selection's character, if max4(sel) > tot / 2:                      */
/*     agree = max4(sel), src = i;                                            */
/*   then the suppliment's, if max4(sup) > tot / 2:                          */
/*     agree = max4(sup), src = i | PBA_QUAL_SUP;                            */
/*   both: depth = min(tot - 1, 65535), qv = phred(agree, N, qmax).          */
/* phred, in integers alone (host, device and numpy agree bit for bit):      */
/*   against = max(N - agree, 0)  (a suppliment counter can exceed N);       */
/*   S[q] = d[q mod 10] * 10^(q div 10), d = {1000, 1258, 1584, 1995, 2511,  */
/*   3162, 3981, 5011, 6309, 7943} = floor(1000 * 10^(r / 10));              */
/*   qv = the largest q in [0, qmax] with (against + 1) * S[q] <=            */
/*   (N + 2) * 1000 in u64: the Laplace estimate (against + 1) / (N + 2) on  */
/*   the Phred scale, rounded down.  qmax in [0, PBA_QUAL_QMAX].             */
/* The own base won iff the output base equals input base src.               */
/* ------------------------------------------------------------------------ */
#define PBA_QUAL_QMAX 60
#define PBA_QUAL_QCAP 93            /* largest qv a pba_qual may hold: '!' + 93 = '~' */
#define PBA_QUAL_SUP  0x80000000u
typedef struct pba_qual pba_qual;   /* per-base evidence of one evolved set, resident on the device: 9 bytes a base */

/* host arithmetic; -1 for qmax outside [0, 60] */
int pba_qual_phred(uint32_t agree, uint64_t n, int qmax);
/* the DEVICE function on host arrays, so the rule is pinned apart from the pile-ups (as pba_windows_trim) */
int pba_qual_phred_device(pba_ctx *ctx, const uint32_t *agree, const uint64_t *n, uint64_t count, int qmax, uint8_t *qv);
/* pba_pileup_evolve with the evidence of every character: the set and rows_out are byte for byte pba_pileup_evolve's, *qual
 * has the set's count and lengths, the pile-up is spent afterwards.  A qmax outside [0, 60] is PBA_E_INVALID before anything
 * happens: the pile-up stays usable. */
int pba_pileup_evolve_qual(pba_ctx *ctx, pba_pileup *p, int qmax, pba_seqs **corrected, pba_correct_row *rows_out /* nullable */,
                           pba_qual **qual);
/* Evidence from host arrays, sequence k at [sum of lengths[0 .. k), + lengths[k]) of each.  A qv above PBA_QUAL_QCAP is
 * PBA_E_INVALID, a total of 2^32 bases or more PBA_E_TOOLONG; n == 0 and empty sequences are legal. */
int pba_qual_create(pba_ctx *ctx, const uint32_t *lengths, uint32_t n, const uint8_t *qv, const uint16_t *depth /* nullable: 0 */,
                    const uint16_t *agree /* nullable: 0 */, const uint32_t *src /* nullable: position in its sequence */, pba_qual **out);
uint32_t pba_qual_count(const pba_qual *q);
int pba_qual_lengths(const pba_qual *q, uint32_t *len, uint32_t cap);
/* sequences [lo, hi) back to back; every array nullable; *n always set; cap below *n: PBA_E_INVALID, nothing written */
int pba_qual_get(pba_ctx *ctx, const pba_qual *q, uint32_t lo, uint32_t hi, uint8_t *qv, uint16_t *depth, uint16_t *agree, uint32_t *src,
                 uint64_t cap, uint64_t *n);
typedef struct { int32_t seq, len, n_sel, n_sup, n_unvoted /* depth == 0 */, n_below /* qv < qmin */, n_low_runs, min_qv /* -1: empty */,
                 max_depth, pad; uint64_t sum_qv, sum_depth; } pba_qual_row;
/* One row per sequence, reduced on the device (a long sequence by tiles of 4 096 bases): the per-base arrays do not cross to
 * the host.  n_low_runs: the maximal runs of qv < qmin (the spans pba_qual_low_spans reports at min_run = 1).  qmin outside
 * [0, 94] is PBA_E_INVALID; cap: entries of rows, at least the count. */
int pba_qual_summary(pba_ctx *ctx, const pba_qual *q, int qmin, pba_qual_row *rows, uint32_t cap);
typedef struct { int32_t seq, beg, end, min_qv; } pba_qual_span;
/* The low spans: a span is a maximal run of positions with qv < qmin inside one sequence (a run never crosses into the next
 * sequence); one of length end - beg >= min_run is reported with the smallest qv in it, sorted by (seq, beg).  Found, ranked,
 * reduced and filtered on the device.  *n_out may exceed cap; then only cap spans are written.  qmin outside [0, 94] or
 * min_run < 1 is PBA_E_INVALID. */
int pba_qual_low_spans(pba_ctx *ctx, const pba_qual *q, int qmin, int min_run, pba_qual_span *out, uint64_t cap, uint64_t *n_out);
/* Sequences [lo, hi) of s as one FASTQ image: record k is '@' name '\n' bases '\n' "+\n" quals '\n', the bases on one line,
 * qual = '!' + qv.  Names as pba_seqs_write_fasta (the decimal id when both are NULL), code 3 prints as T, an empty sequence
 * gives two empty lines.  *n_bytes is host arithmetic and always set; out == NULL asks for the size only; cap below the size is
 * PBA_E_INVALID and nothing is written.  qual must have the set's count and lengths, else PBA_E_INVALID.  One kernel writes
 * bases, quality characters and line ends into a device image, one copy brings it out, the host fills in the headers;
 * pba_seqs_from_fastx reads the image back into the same set. */
int pba_seqs_write_fastq(pba_ctx *ctx, const pba_seqs *s, const pba_qual *qual, uint32_t lo, uint32_t hi, const char *names,
                         const uint64_t *name_off, char *out, uint64_t cap, uint64_t *n_bytes);
void pba_qual_destroy(pba_qual *q);
/* The three drivers with the evidence of what they return: the set, rows, log and stats are exactly those of
 * pba_correct_reads_budget / pba_polish_contigs_budget / pba_layout_consensus, and *qual belongs to the returned set whatever
 * the chunk or range cut.  A qmax outside [0, 60] is PBA_E_INVALID before anything happens.  pba_polish_contigs_qual returns
 * the evidence of the LAST round: src addresses the contigs that entered that round (the caller's target when rounds == 1). */
int pba_correct_reads_qual(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                           uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                           uint64_t max_boxes, pba_seqs **corrected, pba_correct_row *rows_out, pba_overlap_stats stats[2], int qmax,
                           pba_qual **qual);
int pba_polish_contigs_qual(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc /* nullable */,
                            uint32_t mask, double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands,
                            int overlap_min, int weight, int rounds, uint64_t max_boxes, pba_seqs **polished,
                            pba_polish_row *rows_out /* nullable */, pba_polish_round_log *log /* nullable */, int log_cap, int qmax,
                            pba_qual **qual);
int pba_layout_consensus_qual(pba_ctx *ctx, const pba_layout *lay, const pba_seqs *reads, const pba_seqs *reads_rc /* nullable */,
                              const pba_strand_overlap *rows, uint64_t n_rows, double R, int overlap_min, int weight,
                              uint64_t max_boxes, pba_seqs **consensus, pba_polish_row *rows_out /* nullable */,
                              pba_layout_cons_stats *stats /* nullable */, int qmax, pba_qual **qual);

/* ------------------------------------------------------------------------ */
/* Clipping: reads cut to the span their overlap rows support (overlap ->    */
/* CLIP -> overlap -> layout -> consensus; DESIGN §5.8, tests/clip_ref.py    */
/* restates the rule).  A row is a semi-global alignment under the ratio R,  */
/* so it breaks at a chimeric junction or a junk end whenever the foreign    */
/* part costs more than R leaves room for: no row spans such a place, and a  */
/* per-base count of the row intervals that span a position with a margin on */
/* both sides drops to zero there (the coverage rule of miniasm's read       */
/* selection).  A deterministic function of the rows, exactly as good as     */
/* they are: what an alignment swallows -- true error that leaves R's budget */
/* unused lets rows run across a junction -- this rule does not see.         */
/* ("clip", not "trim": pba_ctx_trim releases the ctx's pooled buffers.)     */
/* ------------------------------------------------------------------------ */
enum { PBA_CLIP_DROPPED = 0, PBA_CLIP_WHOLE = 1, PBA_CLIP_CUT = 2 };
#define PBA_CLIP_TARGETS     1u   /* count [t_beg, t_end) on the row's target */
#define PBA_CLIP_QUERIES     2u   /* count [q_beg, q_end) on the row's query (forward-strand ends as the row carries them:
                                     nothing is flipped for strand -1) */
#define PBA_CLIP_KEEP_UNSEEN 4u   /* a read no counted interval lies on stays WHOLE instead of DROPPED */
typedef struct {
    int32_t read, state;
    int32_t beg, end;        /* kept interval, forward strand, half-open; DROPPED: 0, 0 */
    int32_t n_iv;            /* intervals counted on this read (before the margin test) */
    int32_t n_runs;          /* maximal runs of positions with coverage >= min_cov; >= 2: suspect chimera */
    int32_t max_cov;         /* largest coverage of any position (0 for an empty read) */
    int32_t n_covered;       /* positions with coverage >= min_cov */
} pba_clip_row;
typedef struct {
    uint64_t n_rows, n_iv, n_iv_short;     /* n_iv_short: counted intervals of length <= 2 * margin (they cover nothing) */
    uint32_t n_whole, n_cut, n_dropped, n_multi_run, n_unseen, n_chunks;   /* n_multi_run: reads with n_runs >= 2, in any state */
    uint64_t n_bases_in, n_bases_out;
    float events_ms, sweep_ms, gather_ms;  /* HIP events on the ctx's stream; gather_ms is filled by pba_clip_apply */
} pba_clip_stats;
typedef struct pba_clip pba_clip;
/* The clip table of `reads` from n_rows overlap rows (host array, any order; only target, query, strand and the four
 * interval ends are read).  With L a read's length, m = margin, c = min_cov:
 *   counted     every row counts [t_beg, t_end) on its target (PBA_CLIP_TARGETS) and [q_beg, q_end) on its query
 *               (PBA_CLIP_QUERIES); n_iv goes up by one for each.  NOTHING is de-duplicated: a pair of reads seen from both
 *               roles, or on both strands, counts once per row.
 *   coverage    a counted [b, e) with e - b > 2m adds one to cov[p] for p in [b + m, e - m); a shorter one adds nothing
 *               (n_iv_short).  cov[p] = the intervals that span p with at least m bases on both sides.
 *   runs        maximal [s, e) with cov >= c throughout (n_runs, n_covered, max_cov); the winner is the longest, then the
 *               one with the smallest s.
 *   kept        [max(s - m, 0), min(e + m, L)): the c intervals that cover s after shrinking reach m further out, so the
 *               unshrunk coverage is >= c on the extension, and an interval that ends at a junction J shrinks to J - m,
 *               so the extension never crosses J.
 *   state       DROPPED (beg = end = 0) without a run or with a kept length below min_len; with PBA_CLIP_KEEP_UNSEEN a read
 *               with n_iv == 0 is WHOLE, [0, L), whatever its length (n_unseen); else WHOLE if kept == [0, L), else CUT.
 *               An empty read without the flag is DROPPED.
 * On the device: the rows go up once (the ctx's pooled row buffer); the reads are cut into consecutive ranges whose int32
 * difference arenas (L + 1 entries a read, rounded up to a multiple of 4) hold at most max_bases entries -- 0: a quarter of
 * the free device memory over 4 bytes an entry; always fewer than 2^31; a range holds one read at least -- and for every
 * range a lane per row adds +1 / -1 with global atomics, then a workgroup per read scans its arena and reduces the runs
 * (a read of any length is swept by its one workgroup: correct, not fast, for a very long one).  The answer does not depend
 * on the cut.  Work arrays are pooled (pba_ctx_trim).  Checked on the host before anything is uploaded: the rows as
 * pba_layout_create checks them (PBA_E_INVALID; none of its PBA_E_TOOLONG limits applies: nothing here is packed into a key);
 * PBA_E_INVALID also for margin < 0, min_cov < 1, min_len < 0, neither role flag, unknown flag bits.  No reads and no rows
 * are legal.  A set with bytes outside ACGT is legal here: only the lengths are read. */
int pba_clip_create(pba_ctx *ctx, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows, int margin, int min_cov,
                    int min_len, uint32_t flags, uint64_t max_bases /* 0 = default */, pba_clip **out,
                    pba_clip_stats *stats /* nullable */);
/* the per-read table, out[r] for read r; cap below the number of reads: PBA_E_INVALID */
int pba_clip_rows(pba_ctx *ctx, const pba_clip *clip, pba_clip_row *out /* one per read */, uint32_t cap);
/* cov[0 .. L) of one read: *n = L, at most cap entries written.  The event kernel of pba_clip_create on the one-read range
 * and the same scan, so that a test can pin the events apart from the sweep (as pba_pileup_dump does for the votes).  Checks
 * as pba_clip_create; read outside the set: PBA_E_INVALID.  PBA_CLIP_KEEP_UNSEEN is accepted and changes nothing. */
int pba_clip_coverage(pba_ctx *ctx, const pba_seqs *reads, const pba_strand_overlap *rows, uint64_t n_rows, int margin, uint32_t flags,
                      uint32_t read, int32_t *cov, uint32_t cap, uint32_t *n);
/* The clipped reads as a NEW set of the same count and ids: sequence i is bases [beg, end) of read i, a DROPPED read an
 * empty sequence (as an emptied contig stays in pba_polish_contigs).  ASCII is written on the device from the packed arena
 * and packed by pba_seqs_from_device_text: byte for byte what pba_seqs_from_text makes of the sliced texts; no base crosses
 * the host.  `reads` must be the set the table was made from (another count or other lengths: PBA_E_INVALID);
 * PBA_E_ALPHABET for a set with bytes outside ACGT (code 3 would come back as T).
 * AFTER CLIPPING THE OLD ROWS ARE STALE: their alignments end at read ends that no longer exist.  Run the overlapper again
 * on the clipped set; no row remapping is offered. */
int pba_clip_apply(pba_ctx *ctx, const pba_clip *clip, const pba_seqs *reads, pba_seqs **clipped);
int pba_clip_last_stats(const pba_clip *clip, pba_clip_stats *out);
void pba_clip_destroy(pba_clip *clip);

/* ------------------------------------------------------------------------ */
/* Homopolymer compression (HPC).  Not a step the reference has.  Long-read  */
/* errors concentrate in the LENGTH of homopolymer runs; a 16-base seed       */
/* window that spans a run with a length error does not hit, and the banded  */
/* aligner spends its R budget on such errors.  So: seed and align on the     */
/* sequence with every run collapsed to one base, and carry the coordinates   */
/* back.  For a sequence x of L bases over ACGT:                              */
/*   head     position p is a run head iff p == 0 or x[p] != x[p - 1]         */
/*   hpc(x)   the bases at the heads, in order; H = their number              */
/*   S        S[k] = the position of head k, k < H; S[H] = L; strictly        */
/*            increasing; L == 0: H == 0 and S == [0]                         */
/* Two facts the row rules rest on: hpc(rc(x)) == rc(hpc(x)), and             */
/* hpc(x[S[b]:S[e]]) == hpc(x)[b:e].  (tests/hpc_ref.py restates */
/* all of this in plain numpy.)                                               */
/* ------------------------------------------------------------------------ */
typedef struct pba_hpc pba_hpc;            /* the run starts of one compression, resident on the device */
typedef struct {
    uint32_t n_seqs, max_len_in, max_len_out, n_chunks;
    uint64_t n_bases_in, n_bases_out;
    float heads_ms, emit_ms, pack_ms;      /* HIP events on the ctx's stream, summed over the chunks */
} pba_hpc_stats;
/* *out: hpc of every sequence of src as a NEW plain set of the same count and ids, in pba_seqs_from_text's layout -- byte for
 * byte what pba_seqs_from_text makes of the compressed texts -- whatever layout src has (a binary read file's records
 * included, as for pba_seqs_revcomp): the kernels read the bit planes.  An empty sequence stays an empty sequence; a set of 0
 * sequences is legal.  PBA_E_ALPHABET if src holds bytes outside ACGT (code 3 stands for N as well as T: a run of TNT would
 * collapse).  No base crosses the host.
 * *map (nullable: not wanted): S of every sequence, for the lift calls below.  It costs 4 bytes per compressed base plus 8 per
 * sequence, in one device allocation (a bitmap-and-select form would be smaller: not offered); the lengths stay on the host.
 * src goes through in chunks of consecutive sequences of at most max_bases input bases -- 0: the largest that keeps every
 * 32-bit counter of a chunk below 2^31; a chunk holds one sequence at least -- and the answer does not depend on the cut.
 * Work buffers come from the ctx's pool (pba_ctx_trim). */
int pba_seqs_hpc(pba_ctx *ctx, const pba_seqs *src, uint64_t max_bases /* 0 = default */,
                 pba_seqs **out, pba_hpc **map /* nullable */, pba_hpc_stats *stats /* nullable */);
uint32_t pba_hpc_count(const pba_hpc *m);
/* L and H of every sequence, at most cap entries each */
int pba_hpc_lengths(const pba_hpc *m, uint32_t *len_in, uint32_t *len_out, uint32_t cap);   /* either nullable */
/* S[0 .. H] of one sequence: *n = H + 1, at most cap entries written; seq outside the set: PBA_E_INVALID */
int pba_hpc_run_starts(pba_ctx *ctx, const pba_hpc *m, uint32_t seq, uint32_t *starts, uint32_t cap, uint32_t *n);
/* Rows of pba_overlap_strands on the COMPRESSED set (m: its map) into rows on the original set.  A half-open interval [b, e)
 * on the forward strand of hpc(x) lifts to [S[b], S[e]) on the forward strand of x; because rc and hpc commute, a strand -1
 * row lifts with the same forward-strand S of each read (the ends it carries are forward-strand already).  Lq = the
 * original query length:
 *   target, query, strand, dir, cost   copied: THE COST STAYS THAT OF THE COMPRESSED ALIGNMENT
 *   t_beg, t_end through S of the target, q_beg, q_end through S of the query
 *   matlen_a = t_end - t_beg, matlen_b = q_end - q_beg
 *   ref_pos  dir +1: t_beg;  dir -1: t_end - 16 (not clamped)
 *   j        with [qb, qe) the walked query interval -- strand +1: [q_beg, q_end); strand -1: [Lq - q_end, Lq - q_beg) --
 *            dir +1: qb;  dir -1: Lq - qe
 * so the interval identities stated for pba_strand_overlap hold of the lifted row, and pba_overlap_row_pair and
 * pba_layout_place's anchor arithmetic work on it.  pba_clip_*, pba_layout_create, pba_layout_place, pba_pileup_vote_placed
 * (so pba_layout_consensus) take lifted rows: they read ids, strand, dir, cost and the interval ends, and do not hold a row to
 * its cost or match lengths.  pba_pileup_vote and pba_overlap_rows_cigar DO hold a row to its cost: they refuse lifted rows as
 * they refuse any row that is not an alignment of the sets given.  Re-aligning lifted rows in original space is not offered.
 * Checked on the host before anything is uploaded, against the compressed lengths the map remembers: ids, self pairs,
 * strand, dir, intervals non-empty and inside (PBA_E_INVALID).  The rows go up once through the ctx's pooled row buffer, a
 * lane per row, and come back; out may alias rows; n == 0 is legal. */
int pba_hpc_lift_overlaps(pba_ctx *ctx, const pba_hpc *m, const pba_strand_overlap *rows, uint64_t n,
                          pba_strand_overlap *out /* may alias rows */);
/* Rows of pba_map_reads of the compressed reads (reads_map) against the compressed contigs (target_map).  found == 0 rows are
 * copied unchanged.  Otherwise read, nseq, found, strand, contig, cost, n_pairs, diag_cost are copied (the cost stays that of
 * the compressed alignment); r_beg / r_end go through the read's S, c_beg / c_end through the contig's; pos = c_beg;
 * matlen_b = c_end - c_beg, matlen_a = r_end - r_beg; j = r_beg for strand +1, Lr - r_end for strand -1 (Lr = the original
 * read length); seglen = Lr - j.  pba_pileup_vote_mapped takes lifted rows; pba_map_rows_cigar holds a row to its cost and
 * refuses them.  Checked on the host: a found row with a strand other than +1 / -1, a read or contig outside its map, or an
 * interval empty or outside its compressed sequence is PBA_E_INVALID.  n == 0 is legal. */
int pba_hpc_lift_map_rows(pba_ctx *ctx, const pba_hpc *reads_map, const pba_hpc *target_map,
                          const pba_map_row *rows, uint64_t n, pba_map_row *out /* may alias rows */);
int pba_hpc_last_stats(const pba_hpc *m, pba_hpc_stats *out);
void pba_hpc_destroy(pba_hpc *m);

/* ------------------------------------------------------------------------ */
/* Seed-key census and repeat masking of overlap probes.  Not a step the     */
/* reference has.  A probe that lands in a transposon, an rRNA operon or a   */
/* satellite matches every copy in every read that covers one: candidates    */
/* grow with the square of the copy number and the layout is handed rows     */
/* between reads that share a repeat but no locus.  Every overlapper caps    */
/* seed occurrence (minimap2 -f, MHAP's k-mer filter, daligner -t).  Here:   */
/* count the keys, overwrite the probe entries of over-frequent keys with    */
/* the all-ones padding the probe table skips, build the table as before.    */
/* No existing kernel changes.  (tests/census_ref.py restates  */
/* the rule in plain numpy.)                                                 */
/* ------------------------------------------------------------------------ */
/* A census belongs to a mask m (m != 0, at most 26 care bits: the probe table's direct addressing, one u32 counter per value
 * of the care bits) and a visiting mode (pba_index_mode).  count[key], key != 0, is the number of (sequence, visited position)
 * pairs whose window & m equals key; the visited positions of a sequence are exactly those its seed index visits in that mode
 * (PBA_INDEX_HEAD_TAIL: ref_seq::get_seedmap's; PBA_INDEX_ALL: every position [0, len), windows past the end padded with code
 * 3).  In PBA_INDEX_HEAD_TAIL mode over a read set that is the number of target positions a probe with that key would match in
 * an all-vs-all call, the probing read's own positions included.  A zero key is never counted (n_zero_keys).  Sequences are
 * counted as packed: a byte outside ACGT is code 3, as in the index; no set is refused for its alphabet.
 * Refusals, decided on the host before any launch: PBA_E_INVALID for a NULL, lo > hi or hi beyond the set, mask 0, a mode
 * other than the two; PBA_E_TOOLONG for a mask with more than 26 care bits and for a census whose visited positions would reach
 * 2^32 (a counter is 32 bits; summed in 64 bits from the host lengths).  The counters belong to the census; scratch comes from
 * the ctx's pool: a repeated add / lookup / mask_probes allocates nothing. */
typedef struct pba_census pba_census;
typedef struct {
    uint32_t n_seqs, bits;                       /* sequences counted so far (create and every add); care bits of the mask */
    uint64_t n_visited, n_counted, n_zero_keys;  /* n_visited = n_counted + n_zero_keys, over create and every add */
    float count_ms;                              /* HIP events on the ctx's stream around the count kernels, summed */
} pba_census_stats;
/* sequences [lo, hi) of s counted into new counters */
int pba_census_create(pba_ctx *ctx, const pba_seqs *s, uint32_t lo, uint32_t hi, uint32_t mask, int mode, pba_census **out);
/* further ranges, or ranges of other sets, into the same counters */
int pba_census_add(pba_ctx *ctx, pba_census *c, const pba_seqs *s, uint32_t lo, uint32_t hi);
/* counts[i] = count[keys[i] & mask]; a key whose masked value is 0 gives 0 */
int pba_census_lookup(pba_ctx *ctx, const pba_census *c, const uint32_t *keys, uint32_t n, uint32_t *counts);
/* hist: cap >= 2 slots.  hist[0] = counters never counted (2^bits - n_distinct, the zero key's among them); hist[v] for
 * 1 <= v < cap - 1 = distinct keys with count exactly v; hist[cap - 1] = keys with count >= cap - 1.  n_distinct and max_count
 * (both nullable) are exact whatever cap is. */
int pba_census_histogram(pba_ctx *ctx, const pba_census *c, uint64_t *hist, uint32_t cap, uint64_t *n_distinct, uint32_t *max_count);
/* Host arithmetic, no ctx: the occurrence cutoff that gives up at most `fraction` of the distinct keys.  With
 * n_distinct = hist[1] + .. + hist[cap - 1] and budget = (uint64_t)(fraction * n_distinct) in FP64 as written: *max_occ = the
 * smallest c in [max(floor, 1), cap - 2] for which the distinct keys with count > c number at most budget.  No such c (too many
 * keys sit in the lumped last slot, or the interval is empty): PBA_E_TOOLONG, ask for a longer histogram.  fraction outside
 * [0, 1] or NaN, cap < 2, a NULL: PBA_E_INVALID. */
int pba_census_cutoff(const uint64_t *hist, uint32_t cap, double fraction, uint32_t floor, uint32_t *max_occ);
/* Per sequence of s (any set, not only the one counted; the census's mode): n_over[i] = visited positions whose key is nonzero
 * with count > max_occ, n_visited[i] = visited positions.  cap below the number of sequences: PBA_E_INVALID.  For flagging reads
 * that are mostly repeat. */
int pba_census_read_repeats(pba_ctx *ctx, const pba_census *c, const pba_seqs *s, uint32_t max_occ, uint32_t *n_over,
                            uint32_t *n_visited, uint32_t cap);
/* In place on the DEVICE buffer pba_overlap_probes filled (or an all-gathered one), n_slots entries: an entry that is not
 * all-ones and whose key has count > max_occ becomes all-ones; *n_masked = entries changed.  Idempotent.  mask must be the
 * census's (PBA_E_INVALID). */
int pba_census_mask_probes(pba_ctx *ctx, const pba_census *c, void *d_entries, uint64_t n_slots, uint32_t mask, uint32_t max_occ,
                           uint64_t *n_masked);
/* pba_overlap_strands with the probes of over-frequent keys left out of both probe tables.  Composed of public calls only:
 * pba_seqs_revcomp (reads_rc == NULL), then per strand pba_overlap_probes, pba_census_mask_probes, pba_probe_table_create, and
 * pba_overlap_strands_table.  One census of the FORWARD reads serves both strands: targets are always forward, and the probes
 * of rc(q) are looked up in the same counters.  c must be a PBA_INDEX_HEAD_TAIL census under `mask` (PBA_E_INVALID).  Rows, order,
 * stats and refusals are pba_overlap_strands'; stats[s].n_probe_entries is what the masked table holds; n_masked[s] (nullable)
 * the entries taken out.  max_occ = UINT32_MAX masks nothing: the call equals pba_overlap_strands row for row.  A probe whose
 * key no read's index visits (count 0) is never masked and never matches. */
int pba_overlap_strands_masked(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc /* nullable: built inside */,
                               uint32_t t_lo, uint32_t t_hi, uint32_t mask, double R, int max_trial, int overlap_min, int kernel,
                               int strands, const pba_census *c, uint32_t max_occ, pba_strand_overlap *out, uint64_t cap,
                               uint64_t *n_out, pba_overlap_stats stats[2], uint64_t n_masked[2]);
int pba_census_last_stats(const pba_census *c, pba_census_stats *out);
void pba_census_destroy(pba_census *c);

/* ---- variant sites from pile-ups, and every row's allele at each site ----
 * A box where a second allele holds a share of the depth is a site: a heterozygous position, or a column where the copies of
 * a repeat differ.  The rule looks at box i of a target as it stands BEFORE evolve, `weight` the pile-up's:
 *   N = tot - 1 + weight (pba_qual_phred's N); c[A], c[C], c[G], c[T] = the four sel counters (the target's own base carries
 *   weight), c[DEL] = N - (c[A] + c[C] + c[G] + c[T]); major = the first maximal allele in the order A, C, G, T, DEL; minor =
 *   the first maximal allele among the other four; own = the target's own base.
 * Box i is a selection site (PBA_SITE_SEL) iff N >= min_depth, c[minor] >= min_alt and c[minor] * 1000 >= min_permille * N.
 * It is a supply site (PBA_SITE_SUP) under the same three tests with max4(sup) in place of c[minor]: its minor is the winning
 * sup base, n_minor that counter, n_major 0 (major stays the box's major allele).  A box can be both: two records, SEL first.
 * Alleles are codes 0..3 = A, C, G, T and PBA_ALLELE_DEL.  The limits of the boxes apply unchanged (no counter above 65 535). */
#define PBA_SITE_SEL 1
#define PBA_SITE_SUP 2
#define PBA_ALLELE_DEL 4
typedef struct { int32_t target, pos; uint8_t kind, own, major, minor; uint32_t n, n_major, n_minor; } pba_site;
typedef struct pba_sites pba_sites;   /* the sites of a target range, resident on the device, independent of the pile-up */
/* One flag pass over the flat arena of a live pile-up (20 bytes a box), a scan of the per-word counts, one compaction pass:
 * the records of targets [t_lo, t_hi) sorted by (target, pos, kind).  `target` is the set the pile-up was made from (the boxes
 * keep no text: own is read from it; another count or other lengths: PBA_E_INVALID).  The pile-up is only read: dump and evolve
 * afterwards give what they gave before.  A spent pile-up, min_depth < 1, min_alt < 1 or min_permille outside [0, 1000]:
 * PBA_E_INVALID, nothing is made.  The object owns its arrays and survives the pile-up's evolve and destroy. */
int pba_pileup_sites(pba_ctx *ctx, const pba_pileup *p, const pba_seqs *target, int min_depth, int min_alt, int min_permille,
                     pba_sites **out);
/* The same object from a caller's list for the sequences [t_lo, t_hi) of seqs (known sites; pba_qual_create's counterpart).
 * Checked on the host: sorted strictly by (target, pos, kind), targets in the range, positions inside their sequences, kind
 * SEL or SUP, own and a SUP's minor 0..3, major and a SEL's minor 0..4; else PBA_E_INVALID and no object.  2^32 sites or more:
 * PBA_E_TOOLONG.  n == 0 is legal. */
int pba_sites_create(pba_ctx *ctx, const pba_seqs *seqs, uint32_t t_lo, uint32_t t_hi, const pba_site *recs, uint64_t n, pba_sites **out);
uint64_t pba_sites_count(const pba_sites *s);
/* records [*lo, *hi) are target's; a target outside the range: PBA_E_INVALID */
int pba_sites_target_range(const pba_sites *s, uint32_t target, uint64_t *lo, uint64_t *hi);
/* records [lo, hi) from the device; lo > hi or hi beyond the count: PBA_E_INVALID */
int pba_sites_get(pba_ctx *ctx, const pba_sites *s, uint64_t lo, uint64_t hi, pba_site *out);
void pba_sites_destroy(pba_sites *s);

/* Every row's allele at the SEL sites of its target, from the traceback walk of the row's re-run: no script, no temporary.  a is
 * the target (the side the boxes belong to): a MATCH gives the row's base (0..3) at the site, a DELETE PBA_ALLELE_DEL; an
 * INSERT consumes no target base and gives nothing.  A row has exactly one record per SEL site inside the target interval its
 * path covers, in ascending site order whatever its dir.  SUP sites get NO per-row record (a row can supply one box several
 * times).  site: index into the object's records.  sum[k]: the row's totals; n_own / n_major / n_minor count the records whose
 * allele is the site's own / major / minor (own usually is one of the two), n_other those that are neither major nor minor.
 *   pba_overlap_rows_alleles: the pairs are pba_overlap_row_pair's, every row held to its own cost and matlens (a
 *     disagreement is PBA_E_INVALID), as pba_overlap_rows_cigar holds it.
 *   pba_map_rows_alleles: the VOTING roles of a mapped row, pba_map_row_pair's (a = contig), under pba_pileup_vote_mapped's
 *     gate (rc >= 0 and matlen_a >= overlap_min), not held to the row's cost: the records then match, vote for vote, the boxes
 *     the sites were read from.  found == 0 rows and rows that miss the gate: no records, zero totals.
 * off (n + 1 entries) is always complete and *n_total the total; records are copied for the rows, in order, up to the first
 * row whose end exceeds cap (pba_map_rows_cigar's contract).  `sites` must be made from the target set (count and lengths; else
 * PBA_E_INVALID) and a row's target must lie in its range.  _budget: max_slots bounded slots per chunk (0: the default). */
typedef struct { uint32_t site; uint32_t allele; } pba_allele;
typedef struct { int32_t n_sites, n_own, n_major, n_minor, n_other; } pba_allele_counts;
int pba_overlap_rows_alleles(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                             double R, const pba_sites *sites, pba_allele *out, uint64_t cap, uint64_t *off, uint64_t *n_total,
                             pba_allele_counts *sum, pba_result *res);
int pba_overlap_rows_alleles_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                    uint64_t n, double R, const pba_sites *sites, pba_allele *out, uint64_t cap, uint64_t *off,
                                    uint64_t *n_total, pba_allele_counts *sum, pba_result *res, uint64_t max_slots);
int pba_map_rows_alleles(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_map_row *rows,
                         uint64_t n, double R, int overlap_min, const pba_sites *sites, pba_allele *out, uint64_t cap, uint64_t *off,
                         uint64_t *n_total, pba_allele_counts *sum, pba_result *res);
int pba_map_rows_alleles_budget(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                                const pba_map_row *rows, uint64_t n, double R, int overlap_min, const pba_sites *sites, pba_allele *out,
                                uint64_t cap, uint64_t *off, uint64_t *n_total, pba_allele_counts *sum, pba_result *res,
                                uint64_t max_slots);

/* ---- overlap rows phased by their alleles; reads corrected from their own copy ----
 * At a SEL site the rows of a target split into those that come from the target's own copy (haplotype, repeat copy) and those
 * that come from the other one.  The phase rule decides which, from allele records alone, in integers:
 *   v         of a record, from its site: +1 if allele == major, -1 if allele == minor, else 0
 *   o0[s]     the seed orientation of SEL site s: +1 if own == major, -1 if own == minor, else 0; o = +1 reads "major is the
 *             allele of the target's own copy"
 *   lab(g)    sign(g) if |g| >= min_margin, else 0; sign(0) = 0
 *   o(0) = o0; for k = 1 .. n_iter:  h(k)[r] = lab(sum over the records of row r of o(k-1)[site] * v)
 *                                    f(k)[s] = self_weight * o0[s] + sum over the records at s of h(k)[row] * v
 *                                    o(k)    = sign(f(k))
 *   g[r] = sum over the records of row r of o(n_iter)[site] * v; label[r] = lab(g[r]).  There is no early stop.
 * label +1: the row is from the target's own copy; -1: from the other copy; 0: undecided.  n_iter in [0, PBA_PHASE_MAX_ITER],
 * min_margin >= 1, self_weight in [0, 65535]; else PBA_E_INVALID.
 *   pba_phase_row   per row: label, score = g, n_informative = the records with v != 0 at a site whose final o != 0, n_records
 *   pba_phase_site  per SEL site of the object, in SEL-rank order (pba_sites_count_sel of them): site = index into the records,
 *                   orient = o(n_iter), score = the last f (self_weight * o0 for n_iter == 0), n_agree / n_disagree = the
 *                   records with label[row] * v * orient > 0 / < 0 under the final labels
 *   pba_phase_stats n_same / n_other / n_unphased: rows with label +1 / -1 / 0; n_sites: SEL sites; n_flipped_last: sites with
 *                   o(n_iter) != o(n_iter - 1), 0 for n_iter == 0; HIP events on the ctx's stream: the traced passes (0 for
 *                   pba_alleles_phase), the phase kernels */
#define PBA_PHASE_MAX_ITER 64
typedef struct { int32_t n_iter, min_margin, self_weight; } pba_phase_params;
typedef struct { int32_t label, score, n_informative, n_records; } pba_phase_row;
typedef struct { uint32_t site; int32_t orient, score, n_agree, n_disagree; } pba_phase_site;
typedef struct {
    uint64_t n_rows, n_same, n_other, n_unphased, n_sites, n_records, n_flipped_last;
    float alleles_ms, phase_ms;
} pba_phase_stats;
/* the SEL records of the object: what sites_out of the calls below holds */
uint64_t pba_sites_count_sel(const pba_sites *s);
/* The phase kernels on records the caller supplies (row r: rec[off[r] .. off[r + 1]), so that the rule can be pinned apart from
 * the aligner (pba_windows_trim's counterpart).  Checked on the host, each PBA_E_INVALID: off must not decrease; a record's
 * site must be below pba_sites_count and a SEL record, its allele <= PBA_ALLELE_DEL; a row's sites strictly ascending and of
 * one target; the parameters in range.  n == 0 is legal (the sites then keep their seed orientation). */
int pba_alleles_phase(pba_ctx *ctx, const pba_sites *sites, const pba_allele *rec, const uint64_t *off, uint64_t n,
                      const pba_phase_params *params, pba_phase_row *rows_out, pba_phase_site *sites_out /* nullable */,
                      pba_phase_stats *stats /* nullable */);
/* Overlap rows phased.  The records are made as pba_overlap_rows_alleles makes them (every row held to its cost and matlens;
 * `sites` of the target set, every row's target in their range), gathered chunk after chunk into one device buffer and phased
 * there: no record crosses the host.  rows_out: n entries; res (nullable) as pba_overlap_rows_alleles returns it. */
int pba_overlap_rows_phase(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows, uint64_t n,
                           double R, const pba_sites *sites, const pba_phase_params *params, pba_phase_row *rows_out,
                           pba_phase_site *sites_out /* nullable */, pba_phase_stats *stats /* nullable */, pba_result *res /* nullable */);
int pba_overlap_rows_phase_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, const pba_strand_overlap *rows,
                                  uint64_t n, double R, const pba_sites *sites, const pba_phase_params *params, pba_phase_row *rows_out,
                                  pba_phase_site *sites_out /* nullable */, pba_phase_stats *stats /* nullable */,
                                  pba_result *res /* nullable */, uint64_t max_slots);
/* Host: the rows with label > 0, and those with label == 0 when keep_unphased, in order and unchanged; returns their number
 * (out_rows holds up to n; may alias rows), -1 for a NULL.  Unlike trimmed rows these stay valid for every call that re-runs
 * the alignment (votes, cigars, windows, alleles, layout). */
int64_t pba_phase_rows_apply(const pba_strand_overlap *rows, const pba_phase_row *phase, uint64_t n, int keep_unphased,
                             pba_strand_overlap *out_rows);
/* pba_correct_reads with every target voted by the rows of its own copy only.  Per chunk of targets: overlaps, a pile-up voted
 * by all rows, pba_pileup_sites under (min_depth, min_alt, min_permille), that pile-up destroyed, the rows phased
 * (pba_overlap_rows_phase), pba_phase_rows_apply under keep_unphased, a fresh pile-up voted by the kept rows only, evolve; the
 * texts stitched as pba_correct_reads stitches them.  rows_out[].n_rows counts the rows kept; *phase_stats (nullable) is summed
 * over the chunks.  Arguments, limits and stats otherwise as pba_correct_reads_budget; the answer does not depend on the cut.
 * Without a SEL site every label is 0: with keep_unphased the result is pba_correct_reads', byte for byte.  An inconsistency
 * among the engine's own rows is PBA_E_HIP, as there. */
int pba_correct_reads_phased(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                             uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                             int min_depth, int min_alt, int min_permille, const pba_phase_params *params, int keep_unphased,
                             pba_seqs **corrected, pba_correct_row *rows_out, pba_phase_stats *phase_stats /* nullable */,
                             pba_overlap_stats stats[2]);
int pba_correct_reads_phased_budget(pba_ctx *ctx, const pba_seqs *reads, const pba_seqs *reads_rc, uint32_t t_lo, uint32_t t_hi,
                                    uint32_t mask, double R, int max_trial, int overlap_min, int kernel, int strands, int weight,
                                    uint64_t max_boxes, int min_depth, int min_alt, int min_permille, const pba_phase_params *params,
                                    int keep_unphased, pba_seqs **corrected, pba_correct_row *rows_out,
                                    pba_phase_stats *phase_stats /* nullable */, pba_overlap_stats stats[2]);

const char *pba_strerror(int status);

#ifdef __cplusplus
}
#endif
#endif
