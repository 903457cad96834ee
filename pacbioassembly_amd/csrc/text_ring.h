// text_ring.h -- the arithmetic of the bit-vector sweep's text ring (align_bitvec.h: bitvec_pass<.., RING = true>), stated
// once for the kernel and for a host program.  Plain C++ without HIP: a host program can compile it alone
// (tests/test_text_ring_cpu.py does).
//
// In the sweep superblock s processes text element t - 1 - s at step t (element e is column e + 1 of the DP matrix), so the
// 0 / ~0 mask pair a lane needs at step t is the one the lane above needed at step t - 1: one stream of (low, high) values
// per sweep, tapped at 64 delays.  The ring keeps that stream in the wavefront's LDS, one 8-byte cell per element: the two
// masks as the step uses them, low word and high word.  A lane's step reads its cell with one 64-bit LDS read -- two steps'
// cells with one ds_read2_b64 -- at an address that advances by one cell per step.  (One byte per element and plane, read
// sign-extended, was built first: two LDS instructions per step cost the step what the two v_bfe_i32 they replaced had,
// DESIGN.md 4.3 round 10.)
// In rings 1 and 2 the match masks themselves come from a table in LDS (eq_table.h): there a cell is 4 bytes, the byte
// offset of the letter's rows in the lane's table, and two steps' cells come with one ds_read2_b32.  Slots, mirror,
// addresses and the writer are the same; only the cell's size and value differ.
//
// Elements.  The lanes hold the 64 superblocks s_cl .. s_cl + 63 (s_cl: the next superblock to close, align_bitvec.h's
// schedule), so step t reads the 64 consecutive elements t - 1 - s_cl - 63 .. t - 1 - s_cl.
//
// Writer.  The sweep runs in chunks of 32 steps tb .. tb + 31 (tb = 1, 33, ..).  In front of a chunk the wavefront fetches the
// 32 elements txr_fetch_first(tb, s_cl) .. + 31 -- what the lane of superblock s_cl will read in the chunk -- and lane i
// writes element first + i.  s_cl only grows, so every other lane reads older elements and the fetches of consecutive
// chunks overlap or abut: the frontier after the write is element tb + 30 - s_cl (column min(m, tb + 31 - s_cl) where it
// matters), no element below it is missing.
//
// Live window.  s_cl grows by at most one per step (a superblock closes at a step that strictly increases with it), so
// t - s_cl(t) never falls, and from the write at tb (which saw s_cl = c, before the events of step tb) on no lane reads an
// element below tb - 1 - (c + 1) - 63 = first - 64.  The write puts elements first .. first + 31 over first - C ..
// first + 31 - C: dead when first + 31 - C < first - 64, i.e. C >= 96.  C = 128 is the next power of two (the slot is a
// mask); 256 would buy nothing.
//
// No wrap in the step.  A lane's address is set at the start of a chunk and when the lane takes its next superblock
// (64 elements back), to the slot of the element of that step; up to the end of the chunk it then advances by at most 31.  So
// the ring is C + 32 cells, and an element whose slot is below 32 is written a second time C cells up: slot .. slot + 31
// hold consecutive elements for every slot, and the step adds one to the address without a mask.
#ifndef PBA_TEXT_RING_H
#define PBA_TEXT_RING_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PBA_TXR_FN __host__ __device__ __forceinline__
#else
#define PBA_TXR_FN static inline
#endif

#define PBA_TXR_COLS 128                                   // C: elements the ring holds
#define PBA_TXR_CHUNK 32                                   // steps per chunk == elements per write == the mirrored head
#define PBA_TXR_SLOTS (PBA_TXR_COLS + PBA_TXR_CHUNK)       // cells of the ring, second copies included
#define PBA_TXR_CELL 8                                     // bytes of a cell: the low plane's mask, then the high plane's
#define PBA_TXR_BYTES (PBA_TXR_SLOTS * PBA_TXR_CELL)       // per wavefront

// slot of element e (e may be negative: elements in front of the text are fetched like any other and never used)
PBA_TXR_FN int txr_slot(int e) { return e & (PBA_TXR_COLS - 1); }
// where the slot's second copy goes, or -1: it has none
PBA_TXR_FN int txr_mirror(int slot) { return slot < PBA_TXR_CHUNK ? slot + PBA_TXR_COLS : -1; }
// the element the lane of superblock s reads at step t
PBA_TXR_FN int txr_elem(int t, int s) { return t - 1 - s; }
// first of the 32 elements written in front of the chunk that starts at step tb, s_cl being the next superblock to close
PBA_TXR_FN int txr_fetch_first(int tb, int s_cl) { return txr_elem(tb, s_cl); }
// a lane's address (in cells) for step t, set at a chunk's first step and at the step the lane takes superblock s; it
// advances by one per step until the next of the two
PBA_TXR_FN int txr_addr(int t, int s) { return txr_slot(txr_elem(t, s)); }
// the lowest element any lane still reads once the chunk at tb has been written with s_cl = c
PBA_TXR_FN int txr_oldest_live(int tb, int c) { return txr_fetch_first(tb, c) - 64; }

#endif
