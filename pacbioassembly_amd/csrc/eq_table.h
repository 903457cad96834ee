// eq_table.h -- where the bit-vector sweep's match-mask table lives in a wavefront's LDS (align_bitvec.h: bitvec_pass with
// the table, the RING forms at one and two blocks per lane), stated once for the kernel and for a host program.  Plain C++
// without HIP, like text_ring.h: tests/test_eq_table_cpu.py compiles it alone.
//
// The match mask of a block, Eq = ~(Plo ^ mask(l0)) & ~(Phi ^ mask(l1)), depends on the lane's row planes and on the text
// letter l = l0 + 2 l1 of the step alone: four values per block for as long as the lane holds its superblock.  A lane
// writes them when it loads its row planes (in front of the sweep, and at the close event that hands it its next
// superblock) and the step reads the letter's row instead of computing it.
//
// Layout, in dwords from the start of the wavefront's LDS:
//   table   [letter 0..3][block 0..NB-1][lane 0..63]      4 NB rows of 64 dwords.  A lane's blocks of one letter are 64
//                                                         dwords apart (one ds_read2_b32 takes both), a letter's stride is
//                                                         NB * 64 dwords, a multiple of the 64 banks: lane k always reads
//                                                         bank k, whatever letters the lanes hold
//   ring    PBA_TXR_SLOTS cells of 4 bytes                the text ring (text_ring.h).  A cell holds eqt_cell(letter): the
//                                                         byte offset of the letter's rows, ready to be added to the
//                                                         lane's own address.  Every cell is written with a letter in front
//                                                         of the sweep, so whatever a lane reads -- in front of the text,
//                                                         past its end, with its window closed -- stays inside the table
//   sb      [lane]                                        the `fin` superblock word (bitvec_pass): "none" from the start of
//                                                         the sweep to its end, so it has room of its own
// The fin Pv / Mv words have no room of their own: word k (2 nb: Pv, 2 nb + 1: Mv) of a lane is the lane's own table row k.
// A lane writes them at the close of a superblock s >= s_m (the superblock of row m), or after the last step.  The windows
// of the sweep span at most bv_max_span = 63 RB + 64 rows and their narrow side is at least half the wide one (align_bitvec:
// bv_pass1_wl, bv_full_wl), so the nr - m <= wleft rows below row m are fewer than 43 RB + 43 and S - s_m < 64 (the host
// program checks it for every geometry it plays): that lane takes no further superblock (s + 64 >= S), its
// rows are never filled again, the lane's window stays closed, what it reads there afterwards feeds steps whose hand-off
// is masked (`live`), and the diagonal ended in row m.  No other lane ever reads or writes the lane's column of the table.
#ifndef PBA_EQ_TABLE_H
#define PBA_EQ_TABLE_H

#include "text_ring.h"

#define PBA_EQT_LETTERS 4
#define PBA_EQT_LANES 64
#define PBA_EQT_CELL 4                                     // bytes of a ring cell in the table forms

// dwords of the table, and where the ring and the superblock word start
PBA_TXR_FN int eqt_table_words(int nb) { return PBA_EQT_LETTERS * nb * PBA_EQT_LANES; }
PBA_TXR_FN int eqt_ring_word(int nb) { return eqt_table_words(nb); }
PBA_TXR_FN int eqt_sb_word(int nb) { return eqt_table_words(nb) + PBA_TXR_SLOTS; }
PBA_TXR_FN int eqt_lds_words(int nb) { return eqt_sb_word(nb) + PBA_EQT_LANES; }
// the value of a ring cell: byte offset of the letter's rows from the lane's own address (table + 4 * lane)
PBA_TXR_FN int eqt_cell(int letter, int nb) { return letter * nb * PBA_EQT_LANES * 4; }
// dword a lane finds block b's match mask in, given its cell
PBA_TXR_FN int eqt_read_word(int cell, int b, int lane) { return cell / 4 + b * PBA_EQT_LANES + lane; }
// dword a lane writes its row (letter, block b) to
PBA_TXR_FN int eqt_row_word(int letter, int b, int nb, int lane) { return (letter * nb + b) * PBA_EQT_LANES + lane; }
// dword of a lane's fin word k (0 .. 2 nb - 1), aliased onto the table
PBA_TXR_FN int eqt_fin_word(int k, int lane) { return k * PBA_EQT_LANES + lane; }

#endif
