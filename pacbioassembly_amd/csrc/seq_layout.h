// seq_layout.h -- where the sequences of a set lie, stated once for every maker of a pba_seqs (pba_core.hip), the slots of a
// stream (pba_stream.hip) and the staged pair of pba_align_text* (pba_align.hip).  Plain C++ without HIP: a host program can
// compile it alone (tests/test_seq_layout_cpu.py does).
//   text layout     (from text, from device text, revcomp, a stream's text form) four bases per byte, every sequence at the
//                   next 16-byte boundary of the packed arena
//   bytes as given  (from records, from device-packed bytes, a stream's records form) the caller's bytes are the arena
// In both, a sequence owns whole words of the bit planes, 32 bases per word, and entry n of every prefix is the end.
#ifndef PBA_SEQ_LAYOUT_H
#define PBA_SEQ_LAYOUT_H

#include <algorithm>
#include <cstddef>
#include <cstdint>

static const int kMaxSeqLen = 65000;            // engine limit -- u16 DP costs: D(i,j) <= max(i,j) < 65535
static const size_t kSlack = 1024;              // zero bytes around the packed bytes (the bit-vector kernel streams a few hundred bases past an accessor)
static const size_t kPlaneSlack = 64;           // zero word pairs before the first and after the last sequence of the bit planes
static const uint64_t kRecordSlack = 65536;     // zero bytes behind a binary read file, for seed_at's byte-offset reads
#define PBA_PP_BASES 2048                       // bases per work item of k_pack_planes: 64 lanes x 32

static inline uint64_t seq_packed_bytes(uint64_t L) { return ((L + 3) / 4 + 15) & ~15ull; }   // text layout: 16-byte aligned
static inline uint64_t seq_plane_words(uint64_t L) { return (L + 31) / 32; }

// The one walk over n lengths.  Writes entries 0 .. n of the prefixes asked for (null = not wanted) -- off: packed byte offsets
// of the text layout; poff: plane word offsets; item: work items of k_pack_planes before each sequence -- and returns the totals.
struct SeqTotals { uint64_t packed, words, items; uint32_t max_len; };
static inline SeqTotals seq_layout(const uint32_t *len, size_t n, uint64_t *off, uint64_t *poff, uint32_t *item) {
    SeqTotals t = {0, 0, 0, 0};
    for (size_t i = 0;; ++i) {
        if (off) off[i] = t.packed;
        if (poff) poff[i] = t.words;
        if (item) item[i] = (uint32_t)t.items;
        if (i == n) return t;
        const uint64_t L = len[i];
        t.packed += seq_packed_bytes(L);
        t.words += seq_plane_words(L);
        t.items += (L + PBA_PP_BASES - 1) / PBA_PP_BASES;
        t.max_len = std::max(t.max_len, len[i]);
    }
}

// What a stream's slot reserves for any batch of at most slot_bytes input bytes and slot_reads reads (text_form: ASCII, else a
// binary read file): upper bounds of seq_layout's totals, tests/test_seq_layout_cpu.py holds the two against each other.
// plane_cap: word pairs between the slacks; rc_cap: the text-layout arena of the reverse complements, where the slot keeps one.
struct SlotCaps { uint64_t pk_cap, rc_cap, plane_cap; };
static inline SlotCaps slot_caps(bool text_form, uint64_t slot_bytes, uint32_t slot_reads, bool rc) {
    SlotCaps k;
    if (text_form) {                       // every read rounds up to 16 packed bytes and to one plane word
        k.pk_cap = ((slot_bytes + 3) / 4 + 16ull * slot_reads + 15) & ~15ull;
        k.rc_cap = k.pk_cap;
        k.plane_cap = slot_bytes / 32 + slot_reads + 1;
    } else {                               // the file is the arena; four bases per payload byte
        k.pk_cap = (slot_bytes + 15) & ~15ull;
        k.rc_cap = (slot_bytes + 16ull * slot_reads + 15) & ~15ull;      // (rc: every payload rounds up to 16 bytes)
        k.plane_cap = slot_bytes / 8 + slot_reads + 1;
    }
    if (!rc) k.rc_cap = 0;
    return k;
}

// Bytes allocated for an arena of `bytes` packed bytes: kSlack in front of them, the kind's slack behind.
enum ArenaKind { ARENA_TEXT, ARENA_RECORDS, ARENA_DEVICE_PACKED };
static inline size_t arena_bytes(ArenaKind kind, uint64_t bytes) { return kSlack + bytes + (kind == ARENA_RECORDS ? kRecordSlack : kSlack); }

#endif
