// seq_layout_main.cpp -- csrc/seq_layout.h alone, as a host program (tests/test_seq_layout_cpu.py builds it, with the
// sanitizers where the compiler has them).  Every line of stdin is a batch: n, the slot_bytes of its text form and of its
// records form, then n lengths.  Per batch it prints the three prefixes of seq_layout (n + 1 entries each, in exact-size heap
// arrays), the totals, the totals with no prefix asked for, and slot_caps of both forms with slot_reads = n, with and without rc.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "seq_layout.h"

static void caps_line(const char *tag, bool text_form, uint64_t slot_bytes, uint32_t n) {
    const SlotCaps k = slot_caps(text_form, slot_bytes, n, true), f = slot_caps(text_form, slot_bytes, n, false);
    printf("%s %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", tag, k.pk_cap, k.rc_cap, k.plane_cap,
           f.pk_cap, f.rc_cap, f.plane_cap);
}

int main() {
    printf("consts %d %zu %zu %" PRIu64 " %d %" PRIu64 " %" PRIu64 " %zu %zu %zu\n", kMaxSeqLen, kSlack, kPlaneSlack, kRecordSlack,
           PBA_PP_BASES, seq_packed_bytes(65), seq_plane_words(65), arena_bytes(ARENA_TEXT, 100), arena_bytes(ARENA_RECORDS, 100),
           arena_bytes(ARENA_DEVICE_PACKED, 100));
    size_t n;
    uint64_t sb_text, sb_rec;
    while (scanf("%zu %" SCNu64 " %" SCNu64, &n, &sb_text, &sb_rec) == 3) {
        std::vector<uint32_t> len(n), item(n + 1);
        std::vector<uint64_t> off(n + 1), poff(n + 1);
        for (uint32_t &L : len)
            if (scanf("%" SCNu32, &L) != 1) return 2;
        const SeqTotals t = seq_layout(len.data(), n, off.data(), poff.data(), item.data());
        const SeqTotals bare = seq_layout(len.data(), n, nullptr, nullptr, nullptr);
        printf("off");
        for (uint64_t v : off) printf(" %" PRIu64, v);
        printf("\npoff");
        for (uint64_t v : poff) printf(" %" PRIu64, v);
        printf("\nitem");
        for (uint32_t v : item) printf(" %u", v);
        printf("\ntotals %" PRIu64 " %" PRIu64 " %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", t.packed, t.words, t.items,
               t.max_len, bare.packed, bare.words, bare.items, bare.max_len);
        caps_line("caps_text", true, sb_text, (uint32_t)n);
        caps_line("caps_records", false, sb_rec, (uint32_t)n);
    }
    return 0;
}
