"""ctypes binding of libpba.so (include/pba.h).  No fallback: a missing library is an error."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PBA_LIB_PATH") or os.path.join(HERE, "lib", "libpba.so")   # (PBA_LIB_PATH: a tuning build, tools/build_variant.py)

PBA_OK = 0
PBA_E_INVALID, PBA_E_NOMEM, PBA_E_HIP, PBA_E_TOOLONG, PBA_E_NODEVICE, PBA_E_ALPHABET = -1, -2, -3, -4, -5, -6
PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL = 0, 1
PBA_KERNEL_AUTO, PBA_KERNEL_ROWSWEEP, PBA_KERNEL_BITVEC = 0, 1, 2
PBA_A_BACKWARD, PBA_B_BACKWARD = 1, 2
PBA_STREAM_TEXT, PBA_STREAM_RECORDS = 0, 1
PBA_CIG_INS, PBA_CIG_DEL, PBA_CIG_EQ, PBA_CIG_X = 1, 2, 7, 8
PBA_CIG_REVERSED, PBA_CIG_B_IS_QUERY = 1, 2


class PbaPair(C.Structure):
    _fields_ = [("a_seq", C.c_uint32), ("a_pos", C.c_int32), ("a_len", C.c_int32),
                ("b_seq", C.c_uint32), ("b_pos", C.c_int32), ("b_len", C.c_int32), ("flags", C.c_uint32)]


class PbaResult(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rc", "cost", "matlen_a", "matlen_b", "len_a", "len_b", "max_dst", "diag_cost")]


class PbaAlnCounts(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_eq", "n_x", "n_ins", "n_del")]


class PbaLocRow(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("read", "nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs", "diag_cost")]


class PbaLocStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_reads_kept", "n_probe_hits", "n_pairs", "n_located", "n_cells")]


class PbaMapRow(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("read", "nseq", "found", "strand", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "diag_cost",
                 "n_pairs", "r_beg", "r_end", "c_beg", "c_end")]


class PbaMapStats(C.Structure):
    _fields_ = [("strand", PbaLocStats * 2), ("n_second_walk", C.c_uint32)]


class PbaOverlapStats(C.Structure):
    _fields_ = [("n_probe_entries", C.c_uint64), ("n_candidates", C.c_uint64), ("n_pairs", C.c_uint64),
                ("n_overlaps", C.c_uint64), ("n_redo", C.c_uint64), ("scan_ms", C.c_float), ("sort_ms", C.c_float),
                ("walk_ms", C.c_float), ("wide_first", C.c_uint32), ("table_ms", C.c_float), ("n_big_targets", C.c_uint32),
                ("n_prefiltered", C.c_uint64), ("cap_fill", C.c_uint32), ("cap_overflow", C.c_uint32), ("n_listed", C.c_uint64)]


class PbaProfile(C.Structure):
    _fields_ = [("index_ms", C.c_float), ("align_ms", C.c_float), ("align_redo_ms", C.c_float),
                ("nb_first", C.c_uint32), ("nb_redo", C.c_uint32), ("n_first", C.c_uint32), ("n_redo", C.c_uint32)]


class PbaPolishRoundLog(C.Structure):
    _fields_ = [("round", C.c_int32), ("n_mapped", C.c_uint32), ("n_voted", C.c_uint32), ("n_chunks", C.c_uint32),
                ("n_bases_in", C.c_uint64), ("n_bases_out", C.c_uint64), ("index_ms", C.c_float), ("map_ms", C.c_float),
                ("vote_ms", C.c_float), ("evolve_ms", C.c_float)]


class PbaCorrectProfile(C.Structure):
    _fields_ = [("overlap_ms", C.c_float), ("vote_ms", C.c_float), ("evolve_ms", C.c_float), ("n_chunks", C.c_uint32),
                ("n_rows", C.c_uint64), ("n_bases_in", C.c_uint64), ("n_bases_out", C.c_uint64)]


class PbaStreamProfile(C.Structure):
    _fields_ = [("h2d_ms", C.c_float), ("pack_ms", C.c_float), ("locate_ms", C.c_float), ("stall_ms", C.c_float),
                ("n_reads", C.c_uint32), ("n_bytes", C.c_uint64)]


class PbaLayoutStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "n_internal", "n_contain", "n_contain_refused", "n_dovetail", "n_dovetail_dropped")] + \
               [(n, C.c_uint32) for n in ("n_contained", "n_mated_ends", "n_cycles", "n_contigs", "n_placed", "n_unplaced")] + \
               [("n_bases", C.c_uint64), ("classify_ms", C.c_float), ("chain_ms", C.c_float), ("stitch_ms", C.c_float)]


class PbaPlaceStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "n_target_not_placed", "n_outside", "n_eligible")] + \
               [(n, C.c_uint32) for n in ("n_found", "n_found_placed", "n_found_contained", "n_found_unplaced")] + [("place_ms", C.c_float)]


class PbaLayoutConsStats(C.Structure):
    _fields_ = [("place", PbaPlaceStats), ("n_voted", C.c_uint64), ("n_bases_in", C.c_uint64), ("n_bases_out", C.c_uint64),
                ("n_chunks", C.c_uint32), ("n_contigs", C.c_uint32), ("stitch_ms", C.c_float), ("vote_ms", C.c_float),
                ("evolve_ms", C.c_float)]


class PbaClipStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "n_iv", "n_iv_short")] + \
               [(n, C.c_uint32) for n in ("n_whole", "n_cut", "n_dropped", "n_multi_run", "n_unseen", "n_chunks")] + \
               [("n_bases_in", C.c_uint64), ("n_bases_out", C.c_uint64), ("events_ms", C.c_float), ("sweep_ms", C.c_float),
                ("gather_ms", C.c_float)]


class PbaTrimStats(C.Structure):
    _fields_ = [("n_rows", C.c_uint64), ("n_windows", C.c_uint64)] + \
               [(n, C.c_uint32) for n in ("n_whole", "n_cut", "n_dropped", "n_chunks")] + \
               [("windows_ms", C.c_float), ("trim_ms", C.c_float)]


PBA_TRIM_DROPPED, PBA_TRIM_WHOLE, PBA_TRIM_CUT = 0, 1, 2


class PbaHpcStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_seqs", "max_len_in", "max_len_out", "n_chunks")] + \
               [("n_bases_in", C.c_uint64), ("n_bases_out", C.c_uint64), ("heads_ms", C.c_float), ("emit_ms", C.c_float),
                ("pack_ms", C.c_float)]


class PbaCensusStats(C.Structure):
    _fields_ = [("n_seqs", C.c_uint32), ("bits", C.c_uint32), ("n_visited", C.c_uint64), ("n_counted", C.c_uint64),
                ("n_zero_keys", C.c_uint64), ("count_ms", C.c_float)]


PBA_CLIP_DROPPED, PBA_CLIP_WHOLE, PBA_CLIP_CUT = 0, 1, 2
PBA_CLIP_TARGETS, PBA_CLIP_QUERIES, PBA_CLIP_KEEP_UNSEEN = 1, 2, 4
PBA_FX_AUTO, PBA_FX_FASTA, PBA_FX_FASTQ = 0, 1, 2
PBA_FX_KEEP_CASE, PBA_FX_STRICT_ACGT = 1, 2
PBA_QUAL_QMAX, PBA_QUAL_QCAP, PBA_QUAL_SUP = 60, 93, 0x80000000


class PbaFastxRec(C.Structure):
    _fields_ = [("hdr_off", C.c_uint64), ("seq_off", C.c_uint64), ("qual_off", C.c_uint64), ("hdr_len", C.c_uint32),
                ("name_len", C.c_uint32), ("seq_len", C.c_uint32), ("n_seq_lines", C.c_uint32)]


class PbaFastxStats(C.Structure):
    _fields_ = [("format", C.c_int32), ("n_records", C.c_uint32), ("n_pieces", C.c_uint32), ("max_len", C.c_uint32),
                ("n_bytes", C.c_uint64), ("n_lines", C.c_uint64), ("n_bases", C.c_uint64), ("n_folded", C.c_uint64),
                ("h2d_ms", C.c_float), ("parse_ms", C.c_float), ("pack_ms", C.c_float)]


# the ctx's pool slots (csrc/pba_host.h: the POOL_* enum, in its order), as pba_kept_bytes.pool[] lists them
POOL_SLOTS = ("POOL_OVL_CAND", "POOL_OVL_TMP", "POOL_OVL_ITEMS", "POOL_OVL_REDO", "POOL_OVL_REDO_IN", "POOL_OVL_OUT", "POOL_OVL_SMALL",
              "POOL_LOC_ROWS", "POOL_LOC_AUX", "POOL_REDO_IDS", "POOL_IX_OFFS", "POOL_IX_WORK",
              "POOL_TXT_IN", "POOL_TXT_OUT", "POOL_TXT_PAR", "POOL_TXT_CST", "POOL_LOC_IDS", "POOL_LOC_CTG", "POOL_LAY_WORK", "POOL_LAY_ROWS",
              "POOL_FX_FILE", "POOL_FX_TILES", "POOL_FX_LINES", "POOL_FX_RECS", "POOL_FX_IMG", "POOL_CLIP_ARENA", "POOL_CLIP_WORK",
              "POOL_CLIP_TEXT", "POOL_HPC_WORK", "POOL_HPC_TEXT")
IX_CACHE_SLOTS = ("ix_ent", "ix_off", "ix_ent2")


class PbaKeptBytes(C.Structure):
    _fields_ = [("n_pool", C.c_uint32), ("pool", C.c_uint64 * 32), ("ix_cache", C.c_uint64 * 3), ("scratch", C.c_uint64),
                ("stage", C.c_uint64), ("queue", C.c_uint64)]


class PbaSsRow(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("read", "found", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b", "n_trials", "n_pairs")]


# every symbol include/pba.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "pba_encode16": (C.c_uint32, [C.c_char_p]),
    "pba_decode16": (None, [C.c_uint32, C.c_char_p]),
    "pba_text2bin": (C.c_size_t, [C.c_char_p, C.c_size_t, _P, C.c_size_t]),
    "pba_bin2text": (C.c_size_t, [_P, C.c_char_p, C.c_size_t]),
    "pba_seed_at": (C.c_uint32, [_P, C.c_int]),
    "pba_seed_at_fixed": (C.c_uint32, [_P, C.c_int]),
    "pba_mask_from_pattern": (C.c_uint32, [C.c_char_p]),
    "pba_value_at": (C.c_char, [C.c_uint8, C.c_int]),
    "pba_open_binary": (C.c_size_t, [_P, C.c_size_t, C.c_uint32, C.c_uint32, _P, C.c_size_t, _P]),
    "pba_synth_genome": (None, [C.c_uint64, _P, C.c_size_t]),
    "pba_synth_reads": (C.c_int, [C.c_uint64, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_double, C.c_double,
                                  C.c_double, _P, _P, C.c_int]),
    "pba_synth_reads_range": (C.c_int, [C.c_uint64, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double,
                                        C.c_double, _P, _P, C.c_int]),
    "pba_ctx_create": (C.c_int, [C.c_int, C.POINTER(_P)]),
    "pba_ctx_destroy": (None, [_P]),
    "pba_ctx_error": (C.c_char_p, [_P]),
    "pba_ctx_set_stream": (C.c_int, [_P, _P]),
    "pba_ctx_sync": (C.c_int, [_P]),
    "pba_ctx_trim": (C.c_int, [_P]),
    "pba_ctx_kept_bytes": (C.c_int, [_P, _P]),
    "pba_ctx_scribble": (C.c_int, [_P, C.c_int]),
    "pba_ctx_last_profile": (C.c_int, [_P, _P]),
    "pba_ctx_device_info": (C.c_int, [_P, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_uint64)]),
    "pba_seqs_from_text": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_seqs_from_device_text": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(_P)]),
    "pba_seqs_from_records": (C.c_int, [_P, _P, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(_P)]),
    "pba_seqs_export": (C.c_int, [_P, _P, _P, C.c_uint64, _P]),
    "pba_seqs_from_device_packed": (C.c_int, [_P, _P, C.c_uint64, _P, _P, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_seqs_non_acgt": (C.c_int, [_P]),
    "pba_seqs_destroy": (None, [_P]),
    "pba_seqs_count": (C.c_uint32, [_P]),
    "pba_seqs_max_len": (C.c_uint32, [_P]),
    "pba_seqs_packed_bytes": (C.c_uint64, [_P]),
    "pba_seqs_lengths": (C.c_int, [_P, _P, C.c_uint32]),
    "pba_seqs_get_text": (C.c_int, [_P, _P, C.c_uint32, C.c_char_p, C.c_size_t]),
    "pba_seqs_revcomp": (C.c_int, [_P, _P, _P, C.POINTER(_P)]),
    "pba_seqs_from_fastx": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(_P), C.POINTER(_P), _P]),
    "pba_seqs_from_fastx_budget": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(_P), C.POINTER(_P), _P, C.c_uint64]),
    "pba_fastx_index_count": (C.c_uint32, [_P]),
    "pba_fastx_index_recs": (C.c_int, [_P, _P, C.c_uint32]),
    "pba_fastx_index_destroy": (None, [_P]),
    "pba_fastx_sniff": (C.c_int, [_P, C.c_uint64]),
    "pba_fastx_cut": (C.c_int, [_P, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pba_seqs_write_fasta": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pba_index_build": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_index_scan": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, _P, C.c_uint64,
                                 C.POINTER(C.c_uint64)]),
    "pba_index_from_entries": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, C.POINTER(_P)]),
    "pba_index_build_set": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(_P)]),
    "pba_index_seqs": (C.c_uint32, [_P]),
    "pba_index_destroy": (None, [_P]),
    "pba_index_entries": (C.c_uint64, [_P]),
    "pba_index_visited": (C.c_uint32, [_P]),
    "pba_index_dump": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pba_index_find": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, C.c_uint64]),
    "pba_align_batch": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_int, _P]),
    "pba_align_text": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _P]),
    "pba_align_text_trace": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _P, _P,
                                       C.c_int32, C.POINTER(C.c_int32)]),
    "pba_align_text_matrix": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _P, _P, _P,
                                        C.c_uint64, C.POINTER(C.c_int32)]),
    "pba_align_batch_trace": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    "pba_locate": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                             _P, _P]),
    "pba_map_reads": (C.c_int, [_P, _P, _P, _P, _P, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    "pba_loc_stream_create": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64,
                                        C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_loc_stream_buffer": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "pba_loc_stream_submit": (C.c_int, [_P, C.c_uint32]),
    "pba_loc_stream_collect": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32), _P]),
    "pba_loc_stream_pending": (C.c_int, [_P, C.POINTER(_P)]),
    "pba_loc_stream_last_profile": (C.c_int, [_P, _P]),
    "pba_loc_stream_destroy": (None, [_P]),
    "pba_map_stream_create": (C.c_int, [_P, _P, _P, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64,
                                        C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_map_stream_buffer": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "pba_map_stream_submit": (C.c_int, [_P, C.c_uint32]),
    "pba_map_stream_collect": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(C.c_uint32), _P]),
    "pba_map_stream_pending": (C.c_int, [_P, C.POINTER(_P), C.POINTER(_P)]),
    "pba_map_stream_last_profile": (C.c_int, [_P, _P]),
    "pba_map_stream_destroy": (None, [_P]),
    "pba_spaced_round": (C.c_int, [_P, _P, _P, C.c_uint32, _P, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "pba_spaced_multi": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_int,
                                   C.c_int, _P, _P, _P, C.c_int, C.POINTER(C.c_int)]),
    "pba_overlap_all": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, _P,
                                  C.c_uint64, C.POINTER(C.c_uint64), _P]),
    "pba_overlap_probes": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pba_overlap_all_probes": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.c_uint32, C.c_double, C.c_int, C.c_int,
                                         C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64), _P]),
    "pba_probe_table_create": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_probe_table_destroy": (None, [_P]),
    "pba_probe_table_entries": (C.c_uint64, [_P]),
    "pba_overlap_all_table": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_double, C.c_int, C.c_int, _P, C.c_uint64,
                                        C.POINTER(C.c_uint64), _P]),
    "pba_overlap_strands": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int,
                                      C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64), _P]),
    "pba_overlap_strands_table": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, C.c_double, C.c_int, C.c_int, _P,
                                            C.c_uint64, C.POINTER(C.c_uint64), _P]),
    "pba_cons_create": (C.c_int, [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "pba_cons_destroy": (None, [_P]),
    "pba_cons_extent": (C.c_int, [_P, _P]),
    "pba_cons_append": (C.c_int, [_P, _P, C.c_char_p, C.c_int]),
    "pba_cons_prepend": (C.c_int, [_P, _P, C.c_char_p, C.c_int]),
    "pba_cons_elect": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "pba_cons_vote_pairs": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_int, _P]),
    "pba_cons_round": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                 C.c_int, _P, _P]),
    "pba_cons_assemble": (C.c_int, [_P, _P, _P, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int,
                                    _P, C.c_int, C.c_int, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_int)]),
    "pba_cons_evolve": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int32)]),
    "pba_cons_dump": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.POINTER(C.c_int32)]),
    "pba_cons_text": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int32)]),
    "pba_overlap_row_pair": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P]),
    "pba_pileup_create": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_pileup_destroy": (None, [_P]),
    "pba_pileup_vote": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, _P]),
    "pba_pileup_dump": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, C.c_int, C.POINTER(C.c_int32)]),
    "pba_pileup_evolve": (C.c_int, [_P, _P, C.POINTER(_P), _P]),
    "pba_correct_reads": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                    C.c_int, C.POINTER(_P), _P, _P]),
    "pba_correct_reads_budget": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_uint64, C.POINTER(_P), _P, _P]),
    "pba_ctx_last_correct_profile": (C.c_int, [_P, _P]),
    "pba_map_row_pair": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_double, _P]),
    "pba_pileup_vote_mapped": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, _P, C.POINTER(C.c_uint64)]),
    "pba_polish_contigs": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_int, C.POINTER(_P), _P, _P, C.c_int]),
    "pba_polish_contigs_budget": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(_P), _P, _P, C.c_int]),
    "pba_layout_create": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.c_int, C.POINTER(_P), _P]),
    "pba_layout_rows": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "pba_layout_contigs": (C.c_uint32, [_P]),
    "pba_layout_contig_info": (C.c_int, [_P, _P, _P, _P, C.c_uint32]),
    "pba_layout_stitch": (C.c_int, [_P, _P, _P, C.POINTER(_P)]),
    "pba_layout_last_stats": (C.c_int, [_P, _P]),
    "pba_layout_destroy": (None, [_P]),
    "pba_layout_place": (C.c_int, [_P, _P, _P, _P, C.c_uint64, _P, C.c_uint32, _P]),
    "pba_place_row_pair": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_double, _P]),
    "pba_pileup_vote_placed": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, _P, C.POINTER(C.c_uint64)]),
    "pba_layout_consensus": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, C.c_int, C.c_uint64, C.POINTER(_P), _P, _P]),
    "pba_clip_create": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint64, C.POINTER(_P), _P]),
    "pba_clip_rows": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "pba_clip_coverage": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "pba_clip_apply": (C.c_int, [_P, _P, _P, C.POINTER(_P)]),
    "pba_clip_last_stats": (C.c_int, [_P, _P]),
    "pba_clip_destroy": (None, [_P]),
    "pba_seqs_hpc": (C.c_int, [_P, _P, C.c_uint64, C.POINTER(_P), C.POINTER(_P), _P]),
    "pba_hpc_count": (C.c_uint32, [_P]),
    "pba_hpc_lengths": (C.c_int, [_P, _P, _P, C.c_uint32]),
    "pba_hpc_run_starts": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint32, C.POINTER(C.c_uint32)]),
    "pba_hpc_lift_overlaps": (C.c_int, [_P, _P, _P, C.c_uint64, _P]),
    "pba_hpc_lift_map_rows": (C.c_int, [_P, _P, _P, _P, C.c_uint64, _P]),
    "pba_hpc_last_stats": (C.c_int, [_P, _P]),
    "pba_hpc_destroy": (None, [_P]),
    "pba_census_create": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_census_add": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32]),
    "pba_census_lookup": (C.c_int, [_P, _P, _P, C.c_uint32, _P]),
    "pba_census_histogram": (C.c_int, [_P, _P, _P, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "pba_census_cutoff": (C.c_int, [_P, C.c_uint32, C.c_double, C.c_uint32, C.POINTER(C.c_uint32)]),
    "pba_census_read_repeats": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, C.c_uint32]),
    "pba_census_mask_probes": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "pba_overlap_strands_masked": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int,
                                             C.c_int, _P, C.c_uint32, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, _P]),
    "pba_census_last_stats": (C.c_int, [_P, _P]),
    "pba_census_destroy": (None, [_P]),
    "pba_cigar_bound": (C.c_uint32, [C.c_int, C.c_int, C.c_double]),
    "pba_align_batch_cigar": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_uint32, _P, _P, _P, _P, _P]),
    "pba_cigar_from_script": (C.c_int, [_P, C.c_int32, _P, _P, C.c_uint32, _P, C.c_int32, _P]),
    "pba_cigar_string": (C.c_int, [_P, C.c_int32, C.c_char_p, C.c_int32]),
    "pba_map_row_aln_pair": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_double, _P]),
    "pba_map_rows_cigar": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P]),
    "pba_map_rows_cigar_budget": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P,
                                            C.c_uint64]),
    "pba_overlap_rows_cigar": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P]),
    "pba_overlap_rows_cigar_budget": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P,
                                                C.c_uint64]),
    "pba_windows_bound": (C.c_uint32, [C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int]),
    "pba_windows_from_script": (C.c_int, [_P, C.c_int32, _P, _P, C.c_int, C.c_int, C.c_int, C.c_uint32, _P, C.c_int32]),
    "pba_align_batch_windows": (C.c_int, [_P, _P, _P, _P, C.c_size_t, C.c_double, C.c_int, C.c_int, C.c_int, C.c_uint32, _P, _P, _P, _P, _P]),
    "pba_map_rows_windows": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P]),
    "pba_map_rows_windows_budget": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, _P, C.c_uint64, _P, C.POINTER(C.c_uint64),
                                              _P, _P, C.c_uint64]),
    "pba_overlap_rows_windows": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P]),
    "pba_overlap_rows_windows_budget": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, _P, C.c_uint64, _P, C.POINTER(C.c_uint64),
                                                  _P, _P, C.c_uint64]),
    "pba_windows_trim": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, C.c_double, C.c_int, _P]),
    "pba_overlap_rows_trim": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, C.c_double, C.c_int, _P, _P]),
    "pba_overlap_rows_trim_budget": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, C.c_double, C.c_int, _P, _P, C.c_uint64]),
    "pba_trim_rows_apply": (C.c_int64, [_P, _P, C.c_uint64, _P]),
    "pba_qual_phred": (C.c_int, [C.c_uint32, C.c_uint64, C.c_int]),
    "pba_qual_phred_device": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int, _P]),
    "pba_pileup_evolve_qual": (C.c_int, [_P, _P, C.c_int, C.POINTER(_P), _P, C.POINTER(_P)]),
    "pba_qual_create": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P, C.POINTER(_P)]),
    "pba_qual_count": (C.c_uint32, [_P]),
    "pba_qual_lengths": (C.c_int, [_P, _P, C.c_uint32]),
    "pba_qual_get": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pba_qual_summary": (C.c_int, [_P, _P, C.c_int, _P, C.c_uint32]),
    "pba_qual_low_spans": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pba_seqs_write_fastq": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]),
    "pba_qual_destroy": (None, [_P]),
    "pba_correct_reads_qual": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_uint64, C.POINTER(_P), _P, _P, C.c_int, C.POINTER(_P)]),
    "pba_polish_contigs_qual": (C.c_int, [_P, _P, _P, _P, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(_P), _P, _P, C.c_int, C.c_int,
                                          C.POINTER(_P)]),
    "pba_layout_consensus_qual": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, C.c_int, C.c_uint64, C.POINTER(_P), _P, _P,
                                            C.c_int, C.POINTER(_P)]),
    "pba_pileup_sites": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(_P)]),
    "pba_sites_create": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.POINTER(_P)]),
    "pba_sites_count": (C.c_uint64, [_P]),
    "pba_sites_target_range": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pba_sites_get": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _P]),
    "pba_sites_destroy": (None, [_P]),
    "pba_overlap_rows_alleles": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, _P, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P]),
    "pba_overlap_rows_alleles_budget": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, _P, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P, C.c_uint64]),
    "pba_map_rows_alleles": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, _P, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P]),
    "pba_map_rows_alleles_budget": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int, _P, _P, C.c_uint64, _P, C.POINTER(C.c_uint64), _P, _P, C.c_uint64]),
    "pba_sites_count_sel": (C.c_uint64, [_P]),
    "pba_alleles_phase": (C.c_int, [_P, _P, _P, _P, C.c_uint64, _P, _P, _P, _P]),
    "pba_overlap_rows_phase": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, _P, _P, _P, _P, _P, _P]),
    "pba_overlap_rows_phase_budget": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, _P, _P, _P, _P, _P, _P, C.c_uint64]),
    "pba_phase_rows_apply": (C.c_int64, [_P, _P, C.c_uint64, C.c_int, _P]),
    "pba_correct_reads_phased": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.POINTER(_P), _P, _P, _P]),
    "pba_correct_reads_phased_budget": (C.c_int, [_P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int,
                                                  C.c_int, C.c_int, C.c_uint64, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.POINTER(_P), _P,
                                                  _P, _P]),
    "pba_strerror": (C.c_char_p, [C.c_int]),
}

# include/pba_dist.h (libpba_dist.so: the exchange over RCCL for C / C++ hosts)
DIST_LIB_PATH = os.path.join(os.path.dirname(LIB_PATH), "libpba_dist.so")
DIST_SYMBOLS = {
    "pba_dist_unique_id": (C.c_int, [_P]),
    "pba_dist_comm_create": (C.c_int, [_P, C.c_int, C.c_int, _P, C.POINTER(_P)]),
    "pba_dist_comm_destroy": (None, [_P]),
    "pba_dist_rank": (C.c_int, [_P]),
    "pba_dist_world": (C.c_int, [_P]),
    "pba_dist_shard": (None, [C.c_uint64, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "pba_dist_all_gather": (C.c_int, [_P, _P, C.c_uint64, _P]),
    "pba_dist_all_reduce_u64": (C.c_int, [_P, _P, C.c_uint32, C.c_int]),
    "pba_dist_index_build": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
    "pba_dist_gather_reads": (C.c_int, [_P, _P, C.POINTER(_P)]),
    "pba_dist_probe_table": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(_P)]),
}

_lib = None
_dist = None


def load_dist() -> C.CDLL:
    """Load libpba_dist.so (after libpba.so, so that both bind the HIP runtime and the RCCL torch has mapped)."""
    global _dist
    if _dist is not None:
        return _dist
    load()
    if not os.path.exists(DIST_LIB_PATH):
        raise RuntimeError(f"{DIST_LIB_PATH} is missing: build it with `python -m pacbioassembly_amd.build`")
    lib = C.CDLL(DIST_LIB_PATH)
    for name, (res, args) in DIST_SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _dist = lib
    return lib


def load() -> C.CDLL:
    """Load libpba.so and bind every declared symbol.  Raises if the library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m pacbioassembly_amd.build` "
            "(there is no CPU fallback for the HIP path)")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64 and
    # libpba.so needs the same SONAME.  Importing torch first makes the loader bind libpba.so to the
    # copy torch already mapped, so torch tensors, streams and RCCL share one runtime with our kernels
    # (two HSA runtimes in one process leave the second without a GPU).
    if os.environ.get("PBA_NO_TORCH", "0") != "1":
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)       # AttributeError if the .so does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
