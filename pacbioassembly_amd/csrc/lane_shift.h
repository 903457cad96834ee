// lane_shift.h -- which lane of the wavefront holds which superblock in the bit-vector sweep's shifted form (align_bitvec.h:
// bitvec_pass with SHIFT, the table forms of eq_table.h), stated once for the kernel and for a host program.  Plain C++
// without HIP, like text_ring.h and eq_table.h: tests/test_lane_shift_cpu.py compiles it alone.
//
// Lane and column.  The lanes hold the superblocks s_cl .. s_cl + 63 in order (s_cl: the next superblock to close): lane k
// holds superblock s_cl + k, so lane 0 is always the top of the band -- the one lane whose hin is the border "+1 per column"
// and not its neighbour's hout.  The COLUMN of a superblock in LDS (its table rows, its fin words, its fin superblock word:
// eq_table.h) stays s & 63 for as long as the superblock lives; a lane reads column (lane + s_cl) & 63.  A rotation of the
// lanes: 64 lanes, 64 columns, 64 banks.
//
// Hand-off.  hpm / hnm are last step's carries, bit k from lane k.  Lane k >= 1 has superblock s - 1 right above it, and
// close(s - 1) has not fired (else s would be in lane 0): it takes a window cell, or garbage its own open still resets.
// Lane 0's upper neighbour has closed or never existed: it takes the border.  Lanes that hold nothing (superblocks >= S)
// only feed lanes that hold nothing.  No mask, no wrap:
//     hp = (hpm << 1) | 1;  hn = hnm << 1;  ... blocks ...  hpm = hp;  hnm = hn;
//
// Close of s = s_cl, in front of step T = close(s): lane 0 puts its last column aside into column s & 63 (when s >= s_m);
// every lane takes the registers of the lane below it (lsh_src_lane); the last lane takes superblock s + 64 (when < S) and
// fills its rows into column s & 63, which is its column from now on; s_cl grows by one and every lane forms its table and
// ring addresses again.
// The step behind a close takes the carries as they are, unshifted (lsh_hin_*_closed): the lanes moved one up, so bit k of
// last step's carries -- handed out by what was lane k -- is what the superblock now in lane k has above it.  That holds
// for lane 0 too: step T - 1 was the LAST column of s's window, and superblock s + 1 takes that column at step T with a
// window cell above it, not yet the border (the ring form masks lane s & 63's carries from step T on, not from T - 1).  It
// holds for the last lane, whose superblock s + 64 may open at T itself and takes what s + 63 handed out.  From step
// T + 1 on lane 0 takes the border.
#ifndef PBA_LANE_SHIFT_H
#define PBA_LANE_SHIFT_H

#include <stdint.h>

#include "eq_table.h"

#define PBA_LSH_LANES 64

// the superblock lane k holds, the lane that holds superblock s, and the column of LDS a lane works in
PBA_TXR_FN int lsh_sb(int lane, int s_cl) { return s_cl + lane; }
PBA_TXR_FN int lsh_lane(int s, int s_cl) { return s - s_cl; }
PBA_TXR_FN int lsh_col(int lane, int s_cl) { return (lane + s_cl) & (PBA_LSH_LANES - 1); }
// the close: the lane whose registers lane k takes (the last lane takes lane 0's: garbage until its open resets them)
PBA_TXR_FN int lsh_src_lane(int lane) { return (lane + 1) & (PBA_LSH_LANES - 1); }
// the hand-off: what the lanes take, from what they handed out in the step before
PBA_TXR_FN uint64_t lsh_hin_plus(uint64_t hpm) { return (hpm << 1) | 1ull; }
PBA_TXR_FN uint64_t lsh_hin_minus(uint64_t hnm) { return hnm << 1; }
// the step behind a close: the lanes moved instead of the carries
PBA_TXR_FN uint64_t lsh_hin_plus_closed(uint64_t hpm) { return hpm; }
PBA_TXR_FN uint64_t lsh_hin_minus_closed(uint64_t hnm) { return hnm; }
// a lane's ring address (cells) and table dword for step t
PBA_TXR_FN int lsh_ring_addr(int t, int lane, int s_cl) { return txr_addr(t, lsh_sb(lane, s_cl)); }
PBA_TXR_FN int lsh_read_word(int cell, int b, int lane, int s_cl) { return eqt_read_word(cell, b, lsh_col(lane, s_cl)); }

#endif
