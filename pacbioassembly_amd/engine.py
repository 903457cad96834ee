"""Thin Python host layer over the C ABI (include/pba.h) -- used by tests/ and bench.py.

The reference is C++; its drop-in host API is the compat headers in include/compat/.  This module
only wraps the same C entry points for pytest and the benchmark: numpy arrays in, numpy arrays
out, every non-zero status raised as PbaError.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import (PBA_INDEX_ALL, PBA_INDEX_HEAD_TAIL, PBA_KERNEL_AUTO, PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP,
                   PBA_STREAM_RECORDS, PBA_STREAM_TEXT, PbaLocRow, PbaLocStats, PbaMapRow, PbaMapStats, PbaPair, PbaResult, PbaSsRow)

PAIR_DTYPE = np.dtype([("a_seq", "<u4"), ("a_pos", "<i4"), ("a_len", "<i4"), ("b_seq", "<u4"), ("b_pos", "<i4"),
                       ("b_len", "<i4"), ("flags", "<u4")])
RESULT_DTYPE = np.dtype([(n, "<i4") for n in ("rc", "cost", "matlen_a", "matlen_b", "len_a", "len_b", "max_dst", "diag_cost")])
LOC_ROW_DTYPE = np.dtype([(n, "<i4") for n in
                          ("read", "nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs", "diag_cost")])
# pba_map_row: a locate row with its strand, its contig and half-open intervals on the forward strand of read and contig
MAP_ROW_DTYPE = np.dtype([(n, "<i4") for n in
                          ("read", "nseq", "found", "strand", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b",
                           "diag_cost", "n_pairs", "r_beg", "r_end", "c_beg", "c_end")])
SS_ROW_DTYPE = np.dtype([(n, "<i4") for n in
                         ("read", "found", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b", "n_trials",
                          "n_pairs")])
OVERLAP_DTYPE = np.dtype([(n, "<i4") for n in ("target", "query", "j", "dir", "ref_pos", "cost", "matlen_a", "matlen_b")])
# pba_strand_overlap: a pba_overlap row with its strand and half-open intervals on the forward strand of each read
STRAND_OVERLAP_DTYPE = np.dtype([(n, "<i4") for n in ("target", "query", "strand", "j", "dir", "ref_pos", "cost", "matlen_a",
                                                     "matlen_b", "t_beg", "t_end", "q_beg", "q_end")])
# pba_correct_row: one per target of a corrected range
CORRECT_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("target", "n_rows", "len_in", "len_out")])
POLISH_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("contig", "n_rows", "len_in", "len_out")])
POLISH_LOG_DTYPE = np.dtype([("round", "<i4"), ("n_mapped", "<u4"), ("n_voted", "<u4"), ("n_chunks", "<u4"), ("n_bases_in", "<u8"),
                             ("n_bases_out", "<u8"), ("index_ms", "<f4"), ("map_ms", "<f4"), ("vote_ms", "<f4"), ("evolve_ms", "<f4")])
# pba_layout_row: one per read of a layout
LAYOUT_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("read", "state", "contig", "rank", "orient", "offset", "skip", "adv", "container")])
LAYOUT_CONTIG_DTYPE = np.dtype([(n, "<i4") for n in ("head_read", "n_reads", "length")])
PBA_LAY_UNPLACED, PBA_LAY_PLACED, PBA_LAY_CONTAINED = 0, 1, 2
# pba_place_row: one per read, where it votes on its layout's contigs
PLACE_ROW_DTYPE = np.dtype([("read", "<i4"), ("found", "<i4"), ("row", "<u4"), ("contig", "<i4"), ("pos", "<i4"), ("dir", "<i4"),
                            ("strand", "<i4"), ("j", "<i4")])
# pba_clip_row: one per read of a clip table
CLIP_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("read", "state", "beg", "end", "n_iv", "n_runs", "max_cov", "n_covered")])
PBA_CLIP_DROPPED, PBA_CLIP_WHOLE, PBA_CLIP_CUT = _lib.PBA_CLIP_DROPPED, _lib.PBA_CLIP_WHOLE, _lib.PBA_CLIP_CUT
PBA_CLIP_TARGETS, PBA_CLIP_QUERIES, PBA_CLIP_KEEP_UNSEEN = _lib.PBA_CLIP_TARGETS, _lib.PBA_CLIP_QUERIES, _lib.PBA_CLIP_KEEP_UNSEEN
assert CLIP_ROW_DTYPE.itemsize == 32 and C.sizeof(_lib.PbaClipStats) == 80
assert PAIR_DTYPE.itemsize == C.sizeof(PbaPair) and RESULT_DTYPE.itemsize == C.sizeof(PbaResult)
assert LOC_ROW_DTYPE.itemsize == C.sizeof(PbaLocRow) and SS_ROW_DTYPE.itemsize == C.sizeof(PbaSsRow)
assert MAP_ROW_DTYPE.itemsize == C.sizeof(PbaMapRow)
assert POLISH_LOG_DTYPE.itemsize == C.sizeof(_lib.PbaPolishRoundLog)
assert PLACE_ROW_DTYPE.itemsize == 32
# pba_aln_counts: the bases of each kind of a run-length alignment; a run is len << 4 | op
ALN_COUNTS_DTYPE = np.dtype([(n, "<i4") for n in ("n_eq", "n_x", "n_ins", "n_del")])
PBA_CIG_INS, PBA_CIG_DEL, PBA_CIG_EQ, PBA_CIG_X = _lib.PBA_CIG_INS, _lib.PBA_CIG_DEL, _lib.PBA_CIG_EQ, _lib.PBA_CIG_X
PBA_CIG_REVERSED, PBA_CIG_B_IS_QUERY = _lib.PBA_CIG_REVERSED, _lib.PBA_CIG_B_IS_QUERY
assert ALN_COUNTS_DTYPE.itemsize == C.sizeof(_lib.PbaAlnCounts)
# pba_trim_span: the trim rule's answer for one item's windows; pba_trim_row: the same as a row's trimmed intervals
TRIM_SPAN_DTYPE = np.dtype([(n, "<i4") for n in ("state", "n_win", "n_good", "n_runs", "w_beg", "w_end", "a0", "b0", "na", "nb", "cost")])
TRIM_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("state", "n_win", "n_good", "n_runs", "w_beg", "w_end", "t_beg", "t_end", "q_beg", "q_end",
                                                "cost")])
PBA_TRIM_DROPPED, PBA_TRIM_WHOLE, PBA_TRIM_CUT = _lib.PBA_TRIM_DROPPED, _lib.PBA_TRIM_WHOLE, _lib.PBA_TRIM_CUT
assert TRIM_SPAN_DTYPE.itemsize == 44 and TRIM_ROW_DTYPE.itemsize == 44 and C.sizeof(_lib.PbaTrimStats) == 40
# pba_fastx_rec: one per record of a parsed FASTA / FASTQ file, offsets into the file image
PBA_FX_AUTO, PBA_FX_FASTA, PBA_FX_FASTQ = _lib.PBA_FX_AUTO, _lib.PBA_FX_FASTA, _lib.PBA_FX_FASTQ
PBA_FX_KEEP_CASE, PBA_FX_STRICT_ACGT = _lib.PBA_FX_KEEP_CASE, _lib.PBA_FX_STRICT_ACGT
FASTX_REC_DTYPE = np.dtype([("hdr_off", "<u8"), ("seq_off", "<u8"), ("qual_off", "<u8"), ("hdr_len", "<u4"), ("name_len", "<u4"),
                            ("seq_len", "<u4"), ("n_seq_lines", "<u4")])
assert FASTX_REC_DTYPE.itemsize == C.sizeof(_lib.PbaFastxRec) == 40
# pba_qual_row: one per sequence of a Qual; pba_qual_span: a maximal run of qv < qmin inside one sequence
PBA_QUAL_QMAX, PBA_QUAL_QCAP, PBA_QUAL_SUP = _lib.PBA_QUAL_QMAX, _lib.PBA_QUAL_QCAP, _lib.PBA_QUAL_SUP
QUAL_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("seq", "len", "n_sel", "n_sup", "n_unvoted", "n_below", "n_low_runs", "min_qv",
                                                "max_depth", "pad")] + [("sum_qv", "<u8"), ("sum_depth", "<u8")])
QUAL_SPAN_DTYPE = np.dtype([(n, "<i4") for n in ("seq", "beg", "end", "min_qv")])
assert QUAL_ROW_DTYPE.itemsize == 56 and QUAL_SPAN_DTYPE.itemsize == 16
# pba_site: one per (box, kind) the site rule calls; pba_allele: a row's allele at a SEL site; pba_allele_counts: a row's totals
PBA_SITE_SEL, PBA_SITE_SUP, PBA_ALLELE_DEL = 1, 2, 4
SITE_DTYPE = np.dtype([("target", "<i4"), ("pos", "<i4"), ("kind", "u1"), ("own", "u1"), ("major", "u1"), ("minor", "u1"), ("n", "<u4"),
                       ("n_major", "<u4"), ("n_minor", "<u4")])
ALLELE_DTYPE = np.dtype([("site", "<u4"), ("allele", "<u4")])
ALLELE_COUNTS_DTYPE = np.dtype([(n, "<i4") for n in ("n_sites", "n_own", "n_major", "n_minor", "n_other")])
assert SITE_DTYPE.itemsize == 24 and ALLELE_DTYPE.itemsize == 8 and ALLELE_COUNTS_DTYPE.itemsize == 20
# pba_phase_row: a row's label under the phase rule; pba_phase_site: a SEL site's orientation; pba_phase_stats: one call's totals
PBA_PHASE_MAX_ITER = 64
PHASE_PARAMS_DTYPE = np.dtype([(n, "<i4") for n in ("n_iter", "min_margin", "self_weight")])
PHASE_ROW_DTYPE = np.dtype([(n, "<i4") for n in ("label", "score", "n_informative", "n_records")])
PHASE_SITE_DTYPE = np.dtype([("site", "<u4")] + [(n, "<i4") for n in ("orient", "score", "n_agree", "n_disagree")])
PHASE_STATS_DTYPE = np.dtype([(n, "<u8") for n in ("n_rows", "n_same", "n_other", "n_unphased", "n_sites", "n_records", "n_flipped_last")] +
                             [("alleles_ms", "<f4"), ("phase_ms", "<f4")])
assert PHASE_PARAMS_DTYPE.itemsize == 12 and PHASE_ROW_DTYPE.itemsize == 16 and PHASE_SITE_DTYPE.itemsize == 20 and PHASE_STATS_DTYPE.itemsize == 64


class PbaError(RuntimeError):
    def __init__(self, status: int, detail: str = ""):
        self.status = status
        msg = _lib.load().pba_strerror(status).decode()
        super().__init__(f"pba status {status} ({msg})" + (f": {detail}" if detail else ""))


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


# ----------------------------------------------------------------------------- host codec
def encode(text16: bytes) -> int:
    assert len(text16) >= 16
    return _lib.load().pba_encode16(text16)


def decode(code: int) -> bytes:
    buf = C.create_string_buffer(17)
    _lib.load().pba_decode16(code, buf)
    return buf.raw[:16]


def text2bin(text: bytes) -> bytes:
    cap = 4 + (len(text) + 3) // 4
    out = np.zeros(cap, np.uint8)
    n = _lib.load().pba_text2bin(text, len(text), _ptr(out), cap)
    assert n == cap
    return out.tobytes()


def bin2text(record: bytes) -> bytes:
    rec = np.frombuffer(record, np.uint8)
    ln = int(np.frombuffer(record[:4], "<u4")[0])
    buf = C.create_string_buffer(ln + 1)
    n = _lib.load().pba_bin2text(_ptr(rec), buf, ln + 1)
    return buf.raw[:n]


def seed_at(record: bytes, pos: int, fixed: bool = False) -> int:
    rec = np.frombuffer(record + b"\0" * 64, np.uint8)   # seed_at reads past short records (B1)
    lib = _lib.load()
    return (lib.pba_seed_at_fixed if fixed else lib.pba_seed_at)(_ptr(rec), pos)


def mask_from_pattern(pattern: str) -> int:
    return _lib.load().pba_mask_from_pattern(pattern.encode())


def open_binary(file: bytes, min_excl: int = 500, max_excl: int = 20000):
    buf = np.frombuffer(file, np.uint8)
    total = C.c_size_t(0)
    lib = _lib.load()
    kept = lib.pba_open_binary(_ptr(buf), len(file), min_excl, max_excl, None, 0, C.byref(total))
    offs = np.zeros(max(kept, 1), np.uint64)
    lib.pba_open_binary(_ptr(buf), len(file), min_excl, max_excl, _ptr(offs), kept, None)
    return offs[:kept], int(total.value)


# ----------------------------------------------------------------------------- synthetic data
def synth_genome(seed: int, n: int) -> np.ndarray:
    out = np.empty(n, np.uint8)
    _lib.load().pba_synth_genome(seed, _ptr(out), n)
    return out


def synth_reads(seed: int, genome: np.ndarray, n_reads: int, read_len: int, p_ins: float = 0.05,
                p_del: float = 0.05, p_sub: float = 0.05, nthreads: int = 8):
    """Returns (text[n_reads*read_len] uint8, offsets[n_reads+1] uint64, starts[n_reads] uint32)."""
    genome = np.ascontiguousarray(genome, np.uint8)
    out = np.empty(n_reads * read_len, np.uint8)
    starts = np.empty(max(n_reads, 1), np.uint32)
    st = _lib.load().pba_synth_reads(seed, _ptr(genome), genome.size, n_reads, read_len, p_ins, p_del, p_sub,
                                     _ptr(out), _ptr(starts), nthreads)
    if st != 0:
        raise PbaError(st, "pba_synth_reads")
    offs = (np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(read_len))
    return out, offs, starts[:n_reads]


def synth_reads_range(seed: int, genome: np.ndarray, r_lo: int, r_hi: int, read_len: int, p_ins: float = 0.05,
                      p_del: float = 0.05, p_sub: float = 0.05, nthreads: int = 8):
    """Reads [r_lo, r_hi) of the set synth_reads(seed, ...) makes: (text, offsets) of just those reads."""
    genome = np.ascontiguousarray(genome, np.uint8)
    n = r_hi - r_lo
    out = np.empty(max(n, 0) * read_len, np.uint8)
    st = _lib.load().pba_synth_reads_range(seed, _ptr(genome), genome.size, r_lo, r_hi, read_len, p_ins, p_del, p_sub,
                                           _ptr(out), None, nthreads)
    if st != 0:
        raise PbaError(st, "pba_synth_reads_range")
    return out, (np.arange(n + 1, dtype=np.uint64) * np.uint64(read_len))


def concat(seqs: Sequence[bytes]):
    """Concatenate byte strings into (text uint8[], offsets uint64[n+1])."""
    offs = np.zeros(len(seqs) + 1, np.uint64)
    if seqs:
        offs[1:] = np.cumsum([len(s) for s in seqs], dtype=np.uint64)
    text = np.frombuffer(b"".join(seqs), np.uint8).copy() if seqs else np.zeros(0, np.uint8)
    return text, offs


# ----------------------------------------------------------------------------- FASTA / FASTQ
def _u8(data) -> np.ndarray:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, np.uint8)
    a = np.asarray(data)
    if a.dtype != np.uint8 or not a.flags.c_contiguous:
        a = np.ascontiguousarray(a, np.uint8)
    return a.reshape(-1)


def fastx_sniff(data) -> int:
    """PBA_FX_FASTA / PBA_FX_FASTQ by the first byte of the first non-blank line, 0 for no such line (host arithmetic)"""
    buf = _u8(data)
    st = _lib.load().pba_fastx_sniff(_ptr(buf) if buf.size else None, buf.size)
    if st < 0:
        raise PbaError(st, "fastx_sniff")
    return st


def fastx_cut(data, want: int, format: int = PBA_FX_AUTO) -> int:
    """the largest record start p with 0 < p <= want; len(data) if want >= len(data); 0 if there is none (host arithmetic)"""
    buf = _u8(data)
    cut = C.c_uint64()
    st = _lib.load().pba_fastx_cut(_ptr(buf) if buf.size else None, buf.size, format, want, C.byref(cut))
    if st != 0:
        raise PbaError(st, "fastx_cut")
    return cut.value


class FastxIndex:
    """The records of one parse (pba_fastx_index, copied to the host): recs() as FASTX_REC_DTYPE, offsets into the file image."""

    def __init__(self, recs: np.ndarray, stats: dict):
        self._recs, self.stats = recs, stats

    def __len__(self):
        return len(self._recs)

    def recs(self) -> np.ndarray:
        return self._recs

    def names(self, data) -> list:
        buf = _u8(data)
        return [bytes(buf[int(r["hdr_off"]) + 1:int(r["hdr_off"]) + 1 + int(r["name_len"])]).decode("latin-1") for r in self._recs]


# ----------------------------------------------------------------------------- device objects
class Context:
    """One GPU, one stream (pba_ctx).  Raises PbaError(PBA_E_NODEVICE) without a gfx950 device."""

    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = C.c_void_p()
        st = self.lib.pba_ctx_create(device, C.byref(h))
        if st != 0:
            raise PbaError(st, "pba_ctx_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.pba_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    def check(self, st: int, what: str = ""):
        if st != 0:
            raise PbaError(st, f"{what}: {self.lib.pba_ctx_error(self.h).decode()}")

    def set_stream(self, stream_handle: Optional[int]):
        """Run on a caller-owned stream (pba_ctx_set_stream; include/pba.h: "Streams"): its handle, e.g. the cuda_stream of a
        torch.cuda.Stream(); None = back to the ctx's own.  Every call enqueues on the stream set when it is made and returns
        with that work complete (LocStream / MapStream.submit excepted).  A device buffer handed in must have been written on
        that stream, or be complete before the call.  The ctx's own stream is non-blocking: it is not ordered against the
        legacy default stream, which is torch's default stream.  That stream's handle is 0, which the library reads as "the
        own stream": it cannot be selected.  So 0 is refused here (ValueError) rather than taken for None --
        set_stream(torch.cuda.current_stream().cuda_stream) on torch's default stream would silently run the engine unordered
        against the work queued there.  A host on the default stream synchronises before a call, or works on a created stream.
        LocStream / MapStream objects are tied to the stream the ctx was on when they were made."""
        if stream_handle is not None and int(stream_handle) == 0:
            raise ValueError("set_stream(0): 0 is the legacy default stream's handle, which cannot be selected "
                             "(None selects the ctx's own stream; use a created stream, or synchronise)")
        self.check(self.lib.pba_ctx_set_stream(self.h, C.c_void_p(stream_handle)), "set_stream")

    def sync(self):
        self.check(self.lib.pba_ctx_sync(self.h), "sync")

    def trim(self):
        """Give the work buffers kept between calls back to the device (pba_ctx_trim)."""
        self.check(self.lib.pba_ctx_trim(self.h), "trim")

    def kept_bytes(self) -> dict:
        """Test support: the capacity in bytes of every buffer the ctx keeps between calls (pba_ctx_kept_bytes), keyed by
        _lib.POOL_SLOTS, "ix_ent" / "ix_off" / "ix_ent2", "scratch", "stage" and "queue"; 0 = not allocated."""
        kb = _lib.PbaKeptBytes()
        self.check(self.lib.pba_ctx_kept_bytes(self.h, C.byref(kb)), "kept_bytes")
        if kb.n_pool != len(_lib.POOL_SLOTS):
            raise PbaError(_lib.PBA_E_INVALID, f"kept_bytes: the library has {kb.n_pool} pool slots, _lib.POOL_SLOTS names {len(_lib.POOL_SLOTS)}")
        out = {name: int(kb.pool[i]) for i, name in enumerate(_lib.POOL_SLOTS)}
        out["scratch"] = int(kb.scratch)
        out.update({name: int(kb.ix_cache[i]) for i, name in enumerate(_lib.IX_CACHE_SLOTS)})
        out.update(queue=int(kb.queue), stage=int(kb.stage))
        return out

    def scribble(self, byte: int):
        """Test support: every kept buffer, over its whole capacity, set to `byte` (pba_ctx_scribble).  No call may be in
        flight and open streams must be idle."""
        self.check(self.lib.pba_ctx_scribble(self.h, int(byte) & 0xFF), "scribble")

    def last_profile(self) -> dict:
        pr = _lib.PbaProfile()
        self.check(self.lib.pba_ctx_last_profile(self.h, C.byref(pr)), "last_profile")
        return {n: getattr(pr, n) for n, _ in _lib.PbaProfile._fields_}

    def device_info(self):
        name = C.create_string_buffer(256)
        ncu, mhz, hbm = C.c_int(), C.c_int(), C.c_uint64()
        self.check(self.lib.pba_ctx_device_info(self.h, name, 256, C.byref(ncu), C.byref(mhz), C.byref(hbm)))
        return {"name": name.value.decode(), "n_cu": ncu.value, "clock_mhz": mhz.value, "hbm_bytes": hbm.value}

    # -- sequence sets
    def seqs_from_text(self, text: np.ndarray, offsets: np.ndarray, strict_acgt: bool = False) -> "SeqSet":
        text = np.ascontiguousarray(text, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        h = C.c_void_p()
        self.check(self.lib.pba_seqs_from_text(self.h, _ptr(text), _ptr(offsets), offsets.size - 1,
                                               int(strict_acgt), C.byref(h)), "seqs_from_text")
        return SeqSet(self, h)

    def seqs_from_list(self, seqs: Sequence[bytes], strict_acgt: bool = False) -> "SeqSet":
        return self.seqs_from_text(*concat(seqs), strict_acgt=strict_acgt)

    def seqs_from_device_text(self, d_text_ptr: int, d_offsets_ptr: int, n: int, total_bytes: int,
                              max_len: int) -> "SeqSet":
        h = C.c_void_p()
        self.check(self.lib.pba_seqs_from_device_text(self.h, C.c_void_p(d_text_ptr), C.c_void_p(d_offsets_ptr), n,
                                                      total_bytes, max_len, C.byref(h)), "seqs_from_device_text")
        return SeqSet(self, h)

    def seqs_from_records(self, file: bytes, min_excl: int = 500, max_excl: int = 20000) -> "SeqSet":
        buf = np.frombuffer(file, np.uint8)
        h = C.c_void_p()
        self.check(self.lib.pba_seqs_from_records(self.h, _ptr(buf), len(file), min_excl, max_excl, C.byref(h)),
                   "seqs_from_records")
        return SeqSet(self, h)

    def seqs_from_device_packed(self, d_packed_ptr: int, n_bytes: int, offsets: np.ndarray, lengths: np.ndarray,
                                non_acgt: bool = False) -> "SeqSet":
        """A set over packed bytes already on the device (the all-gathered read shards): no re-packing."""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        lengths = np.ascontiguousarray(lengths, np.uint32)
        h = C.c_void_p()
        self.check(self.lib.pba_seqs_from_device_packed(self.h, C.c_void_p(d_packed_ptr), n_bytes, _ptr(offsets), _ptr(lengths),
                                                        lengths.size, int(non_acgt), C.byref(h)), "seqs_from_device_packed")
        return SeqSet(self, h)

    def seqs_revcomp(self, S: "SeqSet", flip=None) -> "SeqSet":
        """A new set whose sequence i is the reverse complement of S's where flip is None or flip[i] (pba_seqs_revcomp: on the
        device, in pba_seqs_from_text's layout); the other sequences are copied as they are."""
        h = C.c_void_p()
        if flip is None:
            fp = None
        else:
            flip = np.ascontiguousarray(flip, np.uint8)
            if flip.size != S.count:
                raise ValueError(f"flip has {flip.size} entries for {S.count} sequences")
            fp = _ptr(flip)
        self.check(self.lib.pba_seqs_revcomp(self.h, S.h, fp, C.byref(h)), "seqs_revcomp")
        return SeqSet(self, h)

    def seqs_from_fastx(self, data, format: int = PBA_FX_AUTO, flags: int = 0, max_piece: int = 0):
        """(SeqSet, FastxIndex) of a FASTA / FASTQ file image (pba_seqs_from_fastx: line ends, headers and sequence lines are
        found on the device).  data: bytes or a u8 array, np.memmap included."""
        buf = _u8(data)
        h, ih, st = C.c_void_p(), C.c_void_p(), _lib.PbaFastxStats()
        self.check(self.lib.pba_seqs_from_fastx_budget(self.h, _ptr(buf) if buf.size else None, buf.size, format, flags, C.byref(h),
                                                       C.byref(ih), C.byref(st), max_piece), "seqs_from_fastx")
        try:
            n = self.lib.pba_fastx_index_count(ih)
            recs = np.zeros(max(n, 1), FASTX_REC_DTYPE)
            self.check(self.lib.pba_fastx_index_recs(ih, _ptr(recs), n), "fastx_index_recs")
        finally:
            self.lib.pba_fastx_index_destroy(ih)
        return SeqSet(self, h), FastxIndex(recs[:n], {k: getattr(st, k) for k, _ in _lib.PbaFastxStats._fields_})

    def read_fastx(self, path: str, format: int = PBA_FX_AUTO, flags: int = 0, max_piece: int = 0):
        """seqs_from_fastx of a file, mapped rather than read"""
        import os
        data = np.memmap(path, np.uint8, "r") if os.path.getsize(path) else np.zeros(0, np.uint8)
        return self.seqs_from_fastx(data, format, flags, max_piece)

    # -- index
    def index_build(self, target: "SeqSet", seq: int, mask: int, mode: int = PBA_INDEX_ALL) -> "SeedIndex":
        h = C.c_void_p()
        self.check(self.lib.pba_index_build(self.h, target.h, seq, mask, mode, C.byref(h)), "index_build")
        return SeedIndex(self, h)

    def index_build_set(self, target: "SeqSet", mask: int) -> "SeedIndex":
        """PBA_INDEX_ALL over every sequence of `target` (pba_index_build_set): hits are global positions, for map_reads."""
        h = C.c_void_p()
        self.check(self.lib.pba_index_build_set(self.h, target.h, mask, C.byref(h)), "index_build_set")
        return SeedIndex(self, h)

    def index_scan(self, target: "SeqSet", seq: int, mask: int, mode: int, part: int, nparts: int,
                   d_entries_ptr: int, cap: int) -> int:
        """Rank `part`'s slice of the index entries into a device buffer; returns how many were written."""
        n = C.c_uint64()
        self.check(self.lib.pba_index_scan(self.h, target.h, seq, mask, mode, part, nparts, C.c_void_p(d_entries_ptr),
                                           cap, C.byref(n)), "index_scan")
        return int(n.value)

    def index_from_entries(self, d_entries_ptr: int, n: int, mask: int, mode: int, seq_len: int) -> "SeedIndex":
        h = C.c_void_p()
        self.check(self.lib.pba_index_from_entries(self.h, C.c_void_p(d_entries_ptr), n, mask, mode, seq_len,
                                                   C.byref(h)), "index_from_entries")
        return SeedIndex(self, h)

    # -- alignment
    def align_batch(self, A: "SeqSet", B: "SeqSet", pairs: np.ndarray, R: float, maxn: int = 0, maxm: int = 0,
                    kernel: int = PBA_KERNEL_AUTO) -> np.ndarray:
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        out = np.zeros(pairs.size, RESULT_DTYPE)
        self.check(self.lib.pba_align_batch(self.h, A.h, B.h, _ptr(pairs), pairs.size, R, maxn, maxm, kernel,
                                            _ptr(out)), "align_batch")
        return out

    def align_text(self, a: bytes, b: bytes, R: float, a_fwd: bool = True, b_fwd: bool = True, maxn: int = 0,
                   maxm: int = 0) -> np.ndarray:
        """a/b hold the accessor's elements in memory order; a backward accessor starts at the last byte."""
        abuf = np.frombuffer(a + b"\0", np.uint8)
        bbuf = np.frombuffer(b + b"\0", np.uint8)
        pa = abuf.ctypes.data + (0 if a_fwd or not a else len(a) - 1)
        pb = bbuf.ctypes.data + (0 if b_fwd or not b else len(b) - 1)
        out = np.zeros(1, RESULT_DTYPE)
        self.check(self.lib.pba_align_text(self.h, C.c_void_p(pa), int(a_fwd), len(a), C.c_void_p(pb), int(b_fwd),
                                           len(b), R, maxn, maxm, _ptr(out)), "align_text")
        return out[0]

    def align_text_trace(self, a: bytes, b: bytes, R: float, a_fwd: bool = True, b_fwd: bool = True, maxn: int = 0,
                         maxm: int = 0):
        """align_text plus the edit script: returns (result, ops uint8[nedit]) with 1 MATCH, 2 INSERT, 3 DELETE."""
        abuf = np.frombuffer(a + b"\0", np.uint8)
        bbuf = np.frombuffer(b + b"\0", np.uint8)
        pa = abuf.ctypes.data + (0 if a_fwd or not a else len(a) - 1)
        pb = bbuf.ctypes.data + (0 if b_fwd or not b else len(b) - 1)
        out = np.zeros(1, RESULT_DTYPE)
        cap = len(a) + len(b) + 1
        ops = np.zeros(cap, np.uint8)
        ne = C.c_int32()
        self.check(self.lib.pba_align_text_trace(self.h, C.c_void_p(pa), int(a_fwd), len(a), C.c_void_p(pb), int(b_fwd), len(b),
                                                 R, maxn, maxm, _ptr(out), _ptr(ops), cap, C.byref(ne)), "align_text_trace")
        return out[0], ops[:ne.value].copy()

    def align_text_matrix(self, a: bytes, b: bytes, R: float, a_fwd: bool = True, b_fwd: bool = True, maxn: int = 0, maxm: int = 0):
        """The DP matrix of one pair (pba_align_text_matrix): returns (result, cost uint16[len_a+1, 2*max_dst+1], parent
        uint8[same], rows swept); cell (i, j) sits at [i, j - i + max_dst]."""
        abuf = np.frombuffer(a + b"\0", np.uint8)
        bbuf = np.frombuffer(b + b"\0", np.uint8)
        pa = abuf.ctypes.data + (0 if a_fwd or not a else len(a) - 1)
        pb = bbuf.ctypes.data + (0 if b_fwd or not b else len(b) - 1)
        la, lb = len(a), len(b)
        md = 1 + int((la if lb >= la else lb) * R)
        len_a = la if lb >= la else min(la, lb + md)
        W = 2 * md + 1
        cost = np.zeros((len_a + 1, W), np.uint16)
        par = np.zeros((len_a + 1, W), np.uint8)
        out = np.zeros(1, RESULT_DTYPE)
        rows = C.c_int32()
        self.check(self.lib.pba_align_text_matrix(self.h, C.c_void_p(pa), int(a_fwd), la, C.c_void_p(pb), int(b_fwd), lb, R, maxn, maxm,
                                                  _ptr(out), _ptr(cost), _ptr(par), cost.size, C.byref(rows)), "align_text_matrix")
        return out[0], cost, par, rows.value

    def align_batch_trace(self, A: "SeqSet", B: "SeqSet", pairs: np.ndarray, R: float, maxn: int = 0, maxm: int = 0,
                          kernel: int = PBA_KERNEL_AUTO):
        """Returns (results, list of ops arrays)."""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        out = np.zeros(pairs.size, RESULT_DTYPE)
        off = np.zeros(pairs.size + 1, np.uint64)
        off[1:] = np.cumsum(pairs["a_len"].astype(np.int64) + pairs["b_len"].astype(np.int64)).astype(np.uint64)
        ops = np.zeros(int(off[-1]) + 1, np.uint8)
        ne = np.zeros(max(pairs.size, 1), np.int32)
        self.check(self.lib.pba_align_batch_trace(self.h, A.h, B.h, _ptr(pairs), pairs.size, R, maxn, maxm, kernel, _ptr(out), _ptr(ops),
                                                  _ptr(off), _ptr(ne)), "align_batch_trace")
        return out, [ops[int(off[q]):int(off[q]) + int(ne[q])].copy() for q in range(pairs.size)]

    def align_batch_cigar(self, A: "SeqSet", B: "SeqSet", pairs: np.ndarray, R: float, maxn: int = 0, maxm: int = 0, flags: int = 0):
        """The alignments of a batch as runs (pba_align_batch_cigar), made on the device from the traceback walk.  Returns
        (results, list of run arrays -- views into one array --, counts of ALN_COUNTS_DTYPE)."""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        n = pairs.size
        out = np.zeros(n, RESULT_DTYPE)
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([cigar_bound(int(p["a_len"]), int(p["b_len"]), R) for p in pairs], dtype=np.uint64) if n else 0
        cig = np.zeros(int(off[-1]) + 1, np.uint32)
        ncig = np.zeros(max(n, 1), np.int32)
        counts = np.zeros(max(n, 1), ALN_COUNTS_DTYPE)
        self.check(self.lib.pba_align_batch_cigar(self.h, A.h, B.h, _ptr(pairs), n, R, maxn, maxm, flags, _ptr(out), _ptr(cig), _ptr(off),
                                                  _ptr(ncig), _ptr(counts)), "align_batch_cigar")
        return out, [cig[int(off[q]):int(off[q]) + int(ncig[q])] for q in range(n)], counts[:n]

    # -- drivers
    def locate(self, ix: "SeedIndex", target: "SeqSet", target_seq: int, reads: "SeqSet", R: float,
               trials: int = 50, min_len: int = 500, maxn: int = 0, maxm: int = 0, kernel: int = PBA_KERNEL_AUTO):
        rows = np.zeros(max(reads.count, 1), LOC_ROW_DTYPE)
        stats = PbaLocStats()
        self.check(self.lib.pba_locate(self.h, ix.h, target.h, target_seq, reads.h, R, trials, min_len, maxn, maxm,
                                       kernel, _ptr(rows), C.byref(stats)), "locate")
        return rows[:reads.count], {n: getattr(stats, n) for n, _ in PbaLocStats._fields_}

    def map_reads(self, ix: "SeedIndex", target: "SeqSet", reads: "SeqSet", R: float, trials: int = 50, min_len: int = 500,
                  maxn: int = 0, maxm: int = 0, kernel: int = PBA_KERNEL_AUTO, strands: int = 3,
                  reads_rc: Optional["SeqSet"] = None):
        """Locate against every sequence of `target` (ix: index_build_set of it) on the strands asked for (pba_map_reads):
        1 = the reads as given, 2 = their reverse complement, 3 = + first, then - for what + left.  Returns (rows of
        MAP_ROW_DTYPE, {"strand": [stats of the + walk, of the - walk], "n_second_walk": n})."""
        rows = np.zeros(max(reads.count, 1), MAP_ROW_DTYPE)
        st = PbaMapStats()
        self.check(self.lib.pba_map_reads(self.h, ix.h, target.h, reads.h, reads_rc.h if reads_rc is not None else None, R, trials,
                                          min_len, maxn, maxm, kernel, strands, _ptr(rows), C.byref(st)), "map_reads")
        per = [{n: getattr(st.strand[k], n) for n, _ in PbaLocStats._fields_} for k in range(2)]
        return rows[:reads.count], {"strand": per, "n_second_walk": int(st.n_second_walk)}

    def spaced_round(self, ix: "SeedIndex", ref: "SeqSet", ref_seq: int, reads: "SeqSet", R: float,
                     max_trial: int = 32, overlap_min: int = 64, buggy_seed_at: bool = False,
                     kernel: int = PBA_KERNEL_AUTO) -> np.ndarray:
        rows = np.zeros(max(reads.count, 1), SS_ROW_DTYPE)
        self.check(self.lib.pba_spaced_round(self.h, ix.h, ref.h, ref_seq, reads.h, R, max_trial, overlap_min,
                                             int(buggy_seed_at), kernel, _ptr(rows)), "spaced_round")
        return rows[:reads.count]


def _spaced_multi(self, ref, ref_seq, reads, R, masks, picks, max_round=100, max_trial=32, overlap_min=64,
                  buggy_seed_at=False, kernel=PBA_KERNEL_AUTO):
    """spaced_seed's main loop for a locked reference; returns (rows, found_round, log list of dicts)."""
    n = max(reads.count, 1)
    rows = np.zeros(n, SS_ROW_DTYPE)
    fr = np.zeros(n, np.int32)
    log = np.zeros(max(max_round, 1), np.dtype([("round", "<i4"), ("mask", "<u4"), ("n_tried", "<i4"), ("n_found", "<i4")]))
    masks = np.ascontiguousarray(masks, np.uint32); picks = np.ascontiguousarray(picks, np.uint32)
    nr = C.c_int()
    self.check(self.lib.pba_spaced_multi(self.h, ref.h, ref_seq, reads.h, R, max_trial, overlap_min, int(buggy_seed_at), kernel,
                                         _ptr(masks), masks.size, _ptr(picks), picks.size, max_round, _ptr(rows), _ptr(fr),
                                         _ptr(log), log.size, C.byref(nr)), "spaced_multi")
    return rows[:reads.count], fr[:reads.count], [dict(zip(log.dtype.names, (int(x) for x in l))) for l in log[:nr.value]]


Context.spaced_multi = _spaced_multi


def _overlap_all(self, reads, mask, R, max_trial=32, overlap_min=64, t_lo=0, t_hi=None, kernel=PBA_KERNEL_AUTO,
                 cap=None):
    """All-vs-all overlap of a read set (targets t_lo..t_hi); returns (overlaps sorted by (target, query), stats)."""
    t_hi = reads.count if t_hi is None else t_hi
    cap = cap if cap is not None else max(1, (t_hi - t_lo) * max(reads.count - 1, 1))
    out = np.empty(cap, OVERLAP_DTYPE)                 # (not zeroed: 320 MB per target range at ten million reads; rows beyond n are never handed out)
    n = C.c_uint64()
    st = _lib.PbaOverlapStats()
    self.check(self.lib.pba_overlap_all(self.h, reads.h, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, _ptr(out), cap,
                                        C.byref(n), C.byref(st)), "overlap_all")
    return out[:min(int(n.value), cap)], {k: getattr(st, k) for k, _ in _lib.PbaOverlapStats._fields_}


def _overlap_probes(self, reads, q_lo, q_hi, mask, max_trial, d_entries_ptr, cap):
    """Probe entries of queries [q_lo, q_hi) into a device buffer (multi-GPU exchange form); returns the count."""
    n = C.c_uint64()
    self.check(self.lib.pba_overlap_probes(self.h, reads.h, q_lo, q_hi, mask, max_trial, C.c_void_p(d_entries_ptr), cap,
                                           C.byref(n)), "overlap_probes")
    return int(n.value)


def _overlap_all_probes(self, reads, d_entries_ptr, n_slots, mask, R, max_trial=32, overlap_min=64, t_lo=0, t_hi=None,
                        kernel=PBA_KERNEL_AUTO, cap=None):
    t_hi = reads.count if t_hi is None else t_hi
    cap = cap if cap is not None else max(1, (t_hi - t_lo) * max(reads.count - 1, 1))
    out = np.empty(cap, OVERLAP_DTYPE)                 # (not zeroed: 320 MB per target range at ten million reads; rows beyond n are never handed out)
    n = C.c_uint64()
    st = _lib.PbaOverlapStats()
    self.check(self.lib.pba_overlap_all_probes(self.h, reads.h, t_lo, t_hi, C.c_void_p(d_entries_ptr), n_slots, mask, R, max_trial,
                                               overlap_min, kernel, _ptr(out), cap, C.byref(n), C.byref(st)), "overlap_all_probes")
    return out[:min(int(n.value), cap)], {k: getattr(st, k) for k, _ in _lib.PbaOverlapStats._fields_}


class ProbeTable:
    """The probe table of a read set (pba_probe_table): built once from a device entry list, scanned by every target range."""

    def __init__(self, ctx, d_entries_ptr, n_slots, mask, max_trial):
        self.ctx = ctx
        self.h = C.c_void_p()
        ctx.check(ctx.lib.pba_probe_table_create(ctx.h, C.c_void_p(d_entries_ptr), n_slots, mask, max_trial, C.byref(self.h)),
                  "probe_table_create")

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_probe_table_destroy(self.h)
        self.h = None

    __del__ = close

    @property
    def entries(self) -> int:
        return self.ctx.lib.pba_probe_table_entries(self.h)


def _overlap_all_table(self, reads, table, R, overlap_min=64, t_lo=0, t_hi=None, kernel=PBA_KERNEL_AUTO, cap=None):
    t_hi = reads.count if t_hi is None else t_hi
    cap = cap if cap is not None else max(1, (t_hi - t_lo) * max(reads.count - 1, 1))
    out = np.empty(cap, OVERLAP_DTYPE)                 # (not zeroed: 320 MB per target range at ten million reads; rows beyond n are never handed out)
    n = C.c_uint64()
    st = _lib.PbaOverlapStats()
    self.check(self.lib.pba_overlap_all_table(self.h, reads.h, t_lo, t_hi, table.h, R, overlap_min, kernel, _ptr(out), cap,
                                              C.byref(n), C.byref(st)), "overlap_all_table")
    return out[:min(int(n.value), cap)], {k: getattr(st, k) for k, _ in _lib.PbaOverlapStats._fields_}


def _overlap_all_sharded(self, reads, mask, R, max_trial=32, overlap_min=64, targets_per_call=10000, kernel=PBA_KERNEL_AUTO,
                         cap_per_target=None, t_lo=0, t_hi=None, table=None):
    """pba_overlap_all for read sets whose candidate lists do not fit one call (false candidates grow with the square of
    the read count; a call takes at most 2^32): the probe table is built once on the device (or handed in: the multi-GPU
    form builds it from the all-gathered entries), the targets [t_lo, t_hi) go through in ranges.  Same result as one call
    (the ranges are independent: this is also what ranks of a multi-GPU run do)."""
    import torch
    n = reads.count
    t_hi = n if t_hi is None else t_hi
    own = table is None
    if own:
        slots = n * 2 * max_trial
        probes = torch.full((max(slots, 1),), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()      # the fill runs on torch's stream, the emit on the ctx's: without this it can land on top of the entries
        self.overlap_probes(reads, 0, n, mask, max_trial, probes.data_ptr(), slots)
        torch.cuda.synchronize()
        table = ProbeTable(self, probes.data_ptr(), probes.numel(), mask, max_trial)
        del probes
    parts, total = [], None
    for lo in range(t_lo, t_hi, targets_per_call):
        hi = min(t_hi, lo + targets_per_call)
        cap = (hi - lo) * (cap_per_target or max(n - 1, 1))
        ov, st = self.overlap_all_table(reads, table, R, overlap_min, lo, hi, kernel, cap)
        parts.append(ov)
        if total is None:
            total = dict(st)
        else:
            for k in ("n_candidates", "n_pairs", "n_overlaps", "n_redo", "scan_ms", "sort_ms", "walk_ms", "n_big_targets", "n_prefiltered", "cap_fill", "cap_overflow", "n_listed"):
                total[k] += st[k]
            total["wide_first"] = max(total["wide_first"], st["wide_first"])
    if own:
        table.close()
    out = np.concatenate(parts) if parts else np.zeros(0, OVERLAP_DTYPE)
    return out, (total or {})


def _stats_pair(st2):
    return [{k: getattr(st, k) for k, _ in _lib.PbaOverlapStats._fields_} for st in st2]


def _overlap_strands(self, reads, mask, R, max_trial=32, overlap_min=64, strands=3, t_lo=0, t_hi=None, kernel=PBA_KERNEL_AUTO,
                     cap=None, reads_rc=None):
    """Overlaps on both strands (pba_overlap_strands): strands 1 = +1 only, 2 = -1 only (the queries reverse-complemented),
    3 = both.  Returns (rows of STRAND_OVERLAP_DTYPE sorted by (target, query, strand), [stats of the +1 pass, of the -1 pass])."""
    t_hi = reads.count if t_hi is None else t_hi
    cap = cap if cap is not None else max(1, 2 * (t_hi - t_lo) * max(reads.count - 1, 1))
    out = np.empty(cap, STRAND_OVERLAP_DTYPE)
    n = C.c_uint64()
    st2 = (_lib.PbaOverlapStats * 2)()
    self.check(self.lib.pba_overlap_strands(self.h, reads.h, reads_rc.h if reads_rc is not None else None, t_lo, t_hi, mask, R,
                                            max_trial, overlap_min, kernel, strands, _ptr(out), cap, C.byref(n), C.byref(st2)),
               "overlap_strands")
    return out[:min(int(n.value), cap)], _stats_pair(st2)


def _overlap_strands_table(self, reads, reads_rc, tab_fwd, tab_rc, R, overlap_min=64, t_lo=0, t_hi=None, kernel=PBA_KERNEL_AUTO,
                           cap=None):
    """pba_overlap_strands_table: targets [t_lo, t_hi) against the probe table of the reads (tab_fwd) and of their reverse
    complement reads_rc (tab_rc); either table may be None to skip its strand."""
    t_hi = reads.count if t_hi is None else t_hi
    cap = cap if cap is not None else max(1, 2 * (t_hi - t_lo) * max(reads.count - 1, 1))
    out = np.empty(cap, STRAND_OVERLAP_DTYPE)
    n = C.c_uint64()
    st2 = (_lib.PbaOverlapStats * 2)()
    self.check(self.lib.pba_overlap_strands_table(self.h, reads.h, reads_rc.h if reads_rc is not None else None, t_lo, t_hi,
                                                  tab_fwd.h if tab_fwd is not None else None, tab_rc.h if tab_rc is not None else None,
                                                  R, overlap_min, kernel, _ptr(out), cap, C.byref(n), C.byref(st2)), "overlap_strands_table")
    return out[:min(int(n.value), cap)], _stats_pair(st2)


def _overlap_strands_sharded(self, reads, mask, R, max_trial=32, overlap_min=64, targets_per_call=10000, kernel=PBA_KERNEL_AUTO,
                             cap_per_target=None, t_lo=0, t_hi=None, strands=3, reads_rc=None, tables=None):
    """overlap_all_sharded on both strands: the reverse complement of the reads (built here unless given) and the two probe
    tables (built once here unless given as (tab_fwd, tab_rc), the multi-GPU form), then the targets [t_lo, t_hi) in ranges.
    Same rows as one overlap_strands call."""
    import torch
    n = reads.count
    t_hi = n if t_hi is None else t_hi
    if strands not in (1, 2, 3):
        raise ValueError("strands must be 1, 2 or 3")
    if strands & 2 and reads_rc is None:
        reads_rc = self.seqs_revcomp(reads)
    own = tables is None
    if own:
        tables = []
        for k, S in ((1, reads), (2, reads_rc)):
            if not strands & k:
                tables.append(None)
                continue
            slots = n * 2 * max_trial
            probes = torch.full((max(slots, 1),), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()  # the fill runs on torch's stream, the emit on the ctx's: without this it can land on top of the entries
            self.overlap_probes(S, 0, n, mask, max_trial, probes.data_ptr(), slots)
            torch.cuda.synchronize()
            tables.append(ProbeTable(self, probes.data_ptr(), probes.numel(), mask, max_trial))
            del probes
    tab_fwd, tab_rc = tables
    parts, total = [], None
    for lo in range(t_lo, t_hi, targets_per_call):
        hi = min(t_hi, lo + targets_per_call)
        cap = 2 * (hi - lo) * (cap_per_target or max(n - 1, 1))
        ov, st2 = self.overlap_strands_table(reads, reads_rc if tab_rc is not None else None, tab_fwd, tab_rc, R, overlap_min,
                                             lo, hi, kernel, cap)
        parts.append(ov)
        if total is None:
            total = [dict(s) for s in st2]
        else:
            for tot, st in zip(total, st2):
                for k in ("n_candidates", "n_pairs", "n_overlaps", "n_redo", "scan_ms", "sort_ms", "walk_ms", "n_big_targets",
                          "n_prefiltered", "cap_fill", "cap_overflow", "n_listed"):
                    tot[k] += st[k]
                tot["wide_first"] = max(tot["wide_first"], st["wide_first"])
    if own:
        for t in tables:
            if t is not None:
                t.close()
    out = np.concatenate(parts) if parts else np.zeros(0, STRAND_OVERLAP_DTYPE)
    return out, (total or [{}, {}])


def overlap_row_pair(row, target_len: int, query_len: int) -> np.ndarray:
    """The pair of accessors an overlap_strands row stands for (pba_overlap_row_pair; host arithmetic): one PAIR_DTYPE
    record with a_seq = the target, b_seq = the query -- for a strand -1 row an index into the reverse-complemented set."""
    r = np.zeros(1, STRAND_OVERLAP_DTYPE)
    for f in STRAND_OVERLAP_DTYPE.names:
        r[f] = row[f]
    out = np.zeros(1, PAIR_DTYPE)
    st = _lib.load().pba_overlap_row_pair(_ptr(r), target_len, query_len, _ptr(out))
    if st != 0:
        raise PbaError(st, "overlap_row_pair")
    return out[0]


def map_row_pair(row, contig_len: int, read_len: int, R: float) -> np.ndarray:
    """The pair a found map_reads row votes with (pba_map_row_pair; host arithmetic): one PAIR_DTYPE record with a = the
    contig from pos, clipped to b_len + max_dst, b = the read from j -- for a strand -1 row an index into the
    reverse-complemented set."""
    r = np.zeros(1, MAP_ROW_DTYPE)
    for f in ("read", "found", "strand", "contig", "j", "pos"):          # what the pair is made of
        r[f] = row[f]
    out = np.zeros(1, PAIR_DTYPE)
    st = _lib.load().pba_map_row_pair(_ptr(r), contig_len, read_len, R, _ptr(out))
    if st != 0:
        raise PbaError(st, "map_row_pair")
    return out[0]


def map_row_aln_pair(row, contig_len: int, read_len: int, R: float) -> np.ndarray:
    """The pair the mapper itself aligned for a found map_reads row (pba_map_row_aln_pair; host arithmetic): one PAIR_DTYPE
    record with a = the read from j, b = the contig from pos, each clipped as align clips it -- for a strand -1 row a
    indexes the reverse-complemented set."""
    r = np.zeros(1, MAP_ROW_DTYPE)
    for f in ("read", "found", "strand", "contig", "j", "pos"):          # what the pair is made of
        r[f] = row[f]
    out = np.zeros(1, PAIR_DTYPE)
    st = _lib.load().pba_map_row_aln_pair(_ptr(r), contig_len, read_len, R, _ptr(out))
    if st != 0:
        raise PbaError(st, "map_row_aln_pair")
    return out[0]


def cigar_bound(a_len: int, b_len: int, R: float) -> int:
    """Upper bound on the runs of a successful pair (pba_cigar_bound; host arithmetic)."""
    return int(_lib.load().pba_cigar_bound(a_len, b_len, R))


def cigar_from_script(ops, a_elems: bytes, b_elems: bytes, flags: int = 0):
    """(runs, counts) of a script and the elements of its two accessors in element order (pba_cigar_from_script)."""
    ops = np.ascontiguousarray(ops, np.uint8)
    cig = np.zeros(max(ops.size, 1), np.uint32)
    counts = np.zeros(1, ALN_COUNTS_DTYPE)
    n = _lib.load().pba_cigar_from_script(_ptr(ops), ops.size, a_elems, b_elems, flags, _ptr(cig), cig.size, _ptr(counts))
    if n < 0:
        raise PbaError(_lib.PBA_E_INVALID, "cigar_from_script")
    return cig[:n], counts[0]


def cigar_string(cigar) -> str:
    """"12=1X3I..." of an array of runs (pba_cigar_string)."""
    cigar = np.ascontiguousarray(cigar, np.uint32)
    buf = C.create_string_buffer(11 * cigar.size + 1)
    n = _lib.load().pba_cigar_string(_ptr(cigar), cigar.size, buf, len(buf))
    return buf.raw[:n].decode()


def _rows_cigar(self, fn, what, head, rows, dtype, R, cap, max_slots):
    rows = np.ascontiguousarray(rows, dtype)
    n = rows.size
    off = np.zeros(n + 1, np.uint64)
    counts = np.zeros(max(n, 1), ALN_COUNTS_DTYPE)
    res = np.zeros(max(n, 1), RESULT_DTYPE)
    total = C.c_uint64()
    if cap is None:                                  # one call to learn the total, one to fetch: the runs are not kept between
        self.check(fn(self.h, *head, _ptr(rows), n, R, None, 0, _ptr(off), C.byref(total), None, None, max_slots), what)
        cap = total.value
    cig = np.zeros(max(int(cap), 1), np.uint32)
    self.check(fn(self.h, *head, _ptr(rows), n, R, _ptr(cig), int(cap), _ptr(off), C.byref(total), _ptr(counts), _ptr(res), max_slots), what)
    runs, pos_ok = [], True
    for k in range(n):
        pos_ok = pos_ok and int(off[k + 1]) <= int(cap)
        runs.append(cig[int(off[k]):int(off[k + 1])] if pos_ok else None)
    return runs, counts[:n], off, res[:n], total.value


def _map_cigar(self, target, reads, rows, R, reads_rc=None, cap=None, max_slots=0):
    """Run-length alignments of map_reads rows (pba_map_rows_cigar_budget): SAM's CIGAR, the read (rc(read) for strand -1) is
    the query, the contig the reference.  Returns (runs per row -- views into one array, None for a row beyond cap --, counts of
    ALN_COUNTS_DTYPE, offsets, results, total runs).  max_slots: bounded slots of one chunk on the device (0: the default)."""
    head = (target.h, reads.h, reads_rc.h if reads_rc is not None else None)
    return _rows_cigar(self, self.lib.pba_map_rows_cigar_budget, "map_cigar", head, rows, MAP_ROW_DTYPE, R, cap, max_slots)


def _overlap_cigar(self, reads, rows, R, reads_rc=None, cap=None, max_slots=0):
    """Run-length alignments of overlap_strands rows (pba_overlap_rows_cigar_budget): the query read is the CIGAR's query, runs
    in the target's forward order.  Returns what map_cigar returns."""
    head = (reads.h, reads_rc.h if reads_rc is not None else None)
    return _rows_cigar(self, self.lib.pba_overlap_rows_cigar_budget, "overlap_cigar", head, rows, STRAND_OVERLAP_DTYPE, R, cap, max_slots)


def _paf(qname, qlen, qbeg, qend, strand, tname, tlen, tbeg, tend, c, nm, cigar):
    block = int(c["n_eq"]) + int(c["n_x"]) + int(c["n_ins"]) + int(c["n_del"])
    return "\t".join(str(x) for x in (qname, qlen, qbeg, qend, "+" if strand == 1 else "-", tname, tlen, tbeg, tend, int(c["n_eq"]),
                                      block, 255, f"NM:i:{nm}", "cg:Z:" + cigar_string(cigar)))


def paf_map_lines(rows, counts, cigars, read_lens, contig_lens, read_names=None, contig_names=None):
    """One PAF line (twelve columns, NM:i: and cg:Z:) per found map_reads row.  Default names: read<i> / contig<c>."""
    out = []
    for k, r in enumerate(rows):
        if not r["found"]:
            continue
        q, t = int(r["read"]), int(r["contig"])
        out.append(_paf(read_names[q] if read_names is not None else f"read{q}", int(read_lens[q]), int(r["r_beg"]), int(r["r_end"]),
                        int(r["strand"]), contig_names[t] if contig_names is not None else f"contig{t}", int(contig_lens[t]),
                        int(r["c_beg"]), int(r["c_end"]), counts[k], int(r["cost"]), cigars[k]))
    return out


def paf_overlap_lines(rows, counts, cigars, read_lens, read_names=None):
    """One PAF line per overlap_strands row: the query read is the PAF query, the target read the PAF target."""
    name = (lambda i: read_names[i]) if read_names is not None else (lambda i: f"read{i}")
    return [_paf(name(int(r["query"])), int(read_lens[int(r["query"])]), int(r["q_beg"]), int(r["q_end"]), int(r["strand"]),
                 name(int(r["target"])), int(read_lens[int(r["target"])]), int(r["t_beg"]), int(r["t_end"]), counts[k], int(r["cost"]),
                 cigars[k]) for k, r in enumerate(rows)]


def place_row_pair(row, contig_len: int, read_len: int, R: float) -> np.ndarray:
    """The pair a found placement votes with (pba_place_row_pair; host arithmetic): one PAIR_DTYPE record with a = the contig
    from pos, clipped to b_len + max_dst, b = the read from j, both backward for dir -1 -- for a strand -1 row b indexes the
    reverse-complemented set."""
    r = np.zeros(1, PLACE_ROW_DTYPE)
    for f in PLACE_ROW_DTYPE.names:
        r[f] = row[f]
    out = np.zeros(1, PAIR_DTYPE)
    st = _lib.load().pba_place_row_pair(_ptr(r), contig_len, read_len, R, _ptr(out))
    if st != 0:
        raise PbaError(st, "place_row_pair")
    return out[0]


def _polish_contigs(self, target, reads, mask, R, trials=50, min_len=500, maxn=0, maxm=0, kernel=PBA_KERNEL_AUTO, strands=3,
                    overlap_min=64, weight=1, rounds=1, reads_rc=None, max_boxes=0):
    """`rounds` rounds of index -> map_reads -> vote -> evolve over the contigs of `target` (pba_polish_contigs).  max_boxes: a
    ceiling on the bases of one internal range of contigs (0 = sized from the free device memory; pba_polish_contigs_budget).
    Returns (SeqSet of the polished contigs, rows of POLISH_ROW_DTYPE for the last round, log of POLISH_LOG_DTYPE per round)."""
    rows = np.zeros(max(target.count, 1), POLISH_ROW_DTYPE)
    log = np.zeros(max(rounds, 1), POLISH_LOG_DTYPE)
    h = C.c_void_p()
    rc_h = reads_rc.h if reads_rc is not None else None
    st = self.lib.pba_polish_contigs_budget(self.h, target.h, reads.h, rc_h, mask, R, trials, min_len, maxn, maxm, kernel, strands,
                                            overlap_min, weight, rounds, max_boxes, C.byref(h), _ptr(rows), _ptr(log), log.size)
    self.check(st, "polish_contigs")
    return SeqSet(self, h), rows[:target.count], log[:max(rounds, 0)]


def _correct_reads(self, reads, mask, R, max_trial=32, overlap_min=64, strands=3, weight=1, t_lo=0, t_hi=None,
                   kernel=PBA_KERNEL_AUTO, reads_rc=None, max_boxes=0):
    """Error-corrected reads of targets [t_lo, t_hi) (pba_correct_reads): overlaps on the strands asked for, every row voted
    into its target's boxes, evolve.  max_boxes: a ceiling on the bases of one internal chunk of targets (0 = sized from the
    free device memory; pba_correct_reads_budget).  Returns (SeqSet of the corrected reads, rows of CORRECT_ROW_DTYPE, [stats of the +1
    pass, of the -1 pass])."""
    t_hi = reads.count if t_hi is None else t_hi
    rows = np.zeros(max(t_hi - t_lo, 1), CORRECT_ROW_DTYPE)
    st2 = (_lib.PbaOverlapStats * 2)()
    h = C.c_void_p()
    rc_h = reads_rc.h if reads_rc is not None else None
    if max_boxes:
        st = self.lib.pba_correct_reads_budget(self.h, reads.h, rc_h, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, strands,
                                               weight, max_boxes, C.byref(h), _ptr(rows), C.byref(st2))
    else:
        st = self.lib.pba_correct_reads(self.h, reads.h, rc_h, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, strands,
                                        weight, C.byref(h), _ptr(rows), C.byref(st2))
    self.check(st, "correct_reads")
    return SeqSet(self, h), rows[:max(t_hi - t_lo, 0)], _stats_pair(st2)


def _last_correct_profile(self) -> dict:
    """HIP-event timings and counts of the most recent correct_reads on this context."""
    pr = _lib.PbaCorrectProfile()
    self.check(self.lib.pba_ctx_last_correct_profile(self.h, C.byref(pr)), "last_correct_profile")
    return {n: getattr(pr, n) for n, _ in _lib.PbaCorrectProfile._fields_}


Context.correct_reads = _correct_reads
Context.map_cigar = _map_cigar
Context.overlap_cigar = _overlap_cigar
Context.polish_contigs = _polish_contigs
Context.last_correct_profile = _last_correct_profile
Context.overlap_strands = _overlap_strands
Context.overlap_strands_table = _overlap_strands_table
Context.overlap_strands_sharded = _overlap_strands_sharded
Context.overlap_all = _overlap_all
Context.overlap_probes = _overlap_probes
Context.overlap_all_probes = _overlap_all_probes
Context.overlap_all_sharded = _overlap_all_sharded
Context.overlap_all_table = _overlap_all_table


class LocStream:
    """Streamed locate (pba_loc_stream): two slots of pinned and device storage made once; batch k+1 is copied and packed on
    a copy stream while the locate of batch k runs.  Per batch: fill buffer() (or submit_reads), submit, collect -- and submit
    the next batch before collecting this one to hide its upload.  The rows of all batches, concatenated, are the rows of
    one Context.locate over the concatenated reads."""
    _api = "pba_loc_stream"                             # (MapStream: the same protocol under another prefix)

    def _call(self, fn: str, *args):
        self.ctx.check(getattr(self.ctx.lib, f"{self._api}_{fn}")(self.h, *args), f"{self._api[4:]}_{fn}")

    def __init__(self, ctx: "Context", ix, target, target_seq: int, R: float, trials: int = 50, min_len: int = 500, maxn: int = 0,
                 maxm: int = 0, kernel: int = PBA_KERNEL_AUTO, slot_bytes: int = 1 << 20, slot_reads: int = 1024,
                 form: int = PBA_STREAM_TEXT):
        self.ctx, self.form, self.slot_bytes, self.slot_reads = ctx, form, int(slot_bytes), int(slot_reads)
        self._keep = (ix, target)                       # the stream looks into both until it is closed
        self.h = C.c_void_p()
        ctx.check(ctx.lib.pba_loc_stream_create(ctx.h, ix.h, target.h, target_seq, R, trials, min_len, maxn, maxm, kernel,
                                                self.slot_bytes, self.slot_reads, form, C.byref(self.h)), "loc_stream_create")

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            getattr(self.ctx.lib, self._api + "_destroy")(self.h)
        self.h = None

    __del__ = close

    def buffer(self):
        """(bytes uint8[slot_bytes], offsets uint64[max(slot_reads + 1, 3)]): numpy views of the next free slot's pinned memory,
        to be filled in place and left alone between submit and the collect of that batch."""
        b, o = C.c_void_p(), C.c_void_p()
        self._call("buffer", C.byref(b), C.byref(o))
        nb, no = max(self.slot_bytes, 1), max(self.slot_reads + 1, 3)
        return (np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_uint8)), shape=(nb,))[:self.slot_bytes],
                np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_uint64)), shape=(no,)))

    def submit(self, n: int = 0):
        self._call("submit", n)

    def submit_reads(self, reads: Sequence[bytes]):
        """Text form: write the reads into the slot and submit them."""
        buf, offs = self.buffer()
        total = sum(len(r) for r in reads)
        if total > self.slot_bytes or len(reads) > self.slot_reads:
            raise PbaError(_lib.PBA_E_TOOLONG, "loc_stream_submit: the batch does not fit the slot")
        offs[0] = 0
        if reads:
            offs[1:len(reads) + 1] = np.cumsum([len(r) for r in reads], dtype=np.uint64)
            buf[:total] = np.frombuffer(b"".join(reads), np.uint8)
        self.submit(len(reads))

    def submit_records(self, file: bytes, min_excl: int = 500, max_excl: int = 20000):
        """Records form: write a binary read file into the slot and submit it."""
        buf, offs = self.buffer()
        if len(file) > self.slot_bytes:
            raise PbaError(_lib.PBA_E_TOOLONG, "loc_stream_submit: the batch does not fit the slot")
        buf[:len(file)] = np.frombuffer(file, np.uint8)
        offs[0], offs[1], offs[2] = len(file), min_excl, max_excl
        self.submit(0)

    def collect(self):
        """(rows, stats) of the oldest pending batch."""
        rows = np.zeros(max(self.slot_reads, 1), LOC_ROW_DTYPE)
        stats, n = PbaLocStats(), C.c_uint32()
        self.ctx.check(self.ctx.lib.pba_loc_stream_collect(self.h, _ptr(rows), self.slot_reads, C.byref(n), C.byref(stats)),
                       "loc_stream_collect")
        return rows[:n.value].copy(), {k: getattr(stats, k) for k, _ in PbaLocStats._fields_}

    def pending(self) -> "SeqSet":
        """The set of the batch collect() would run next, borrowed from its slot (valid until that collect)."""
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pba_loc_stream_pending(self.h, C.byref(h)), "loc_stream_pending")
        return BorrowedSeqSet(self.ctx, h)

    def profile(self) -> dict:
        pr = _lib.PbaStreamProfile()
        self._call("last_profile", C.byref(pr))
        return {k: getattr(pr, k) for k, _ in _lib.PbaStreamProfile._fields_}


def _locate_stream(self, ix, target, target_seq, R, trials=50, min_len=500, maxn=0, maxm=0, kernel=PBA_KERNEL_AUTO,
                   slot_bytes=1 << 20, slot_reads=1024, form=PBA_STREAM_TEXT) -> LocStream:
    return LocStream(self, ix, target, target_seq, R, trials, min_len, maxn, maxm, kernel, slot_bytes, slot_reads, form)


Context.locate_stream = _locate_stream


class MapStream(LocStream):
    """Streamed mapping (pba_map_stream): LocStream's slots and protocol under Context.map_reads -- many contigs, both strands.
    With strands & 2 a slot also holds the reverse complement of its batch, packed on the copy stream behind the forward pack.
    The rows of all batches, concatenated, are the rows of one Context.map_reads over the concatenated reads, and the stats
    of the batches sum to that call's."""
    _api = "pba_map_stream"

    def __init__(self, ctx: "Context", ix, target, R: float, trials: int = 50, min_len: int = 500, maxn: int = 0, maxm: int = 0,
                 kernel: int = PBA_KERNEL_AUTO, strands: int = 3, slot_bytes: int = 1 << 20, slot_reads: int = 1024,
                 form: int = PBA_STREAM_TEXT):
        self.ctx, self.form, self.slot_bytes, self.slot_reads = ctx, form, int(slot_bytes), int(slot_reads)
        self._keep = (ix, target)                       # the stream looks into both until it is closed
        self.h = C.c_void_p()
        ctx.check(ctx.lib.pba_map_stream_create(ctx.h, ix.h, target.h, R, trials, min_len, maxn, maxm, kernel, strands,
                                                self.slot_bytes, self.slot_reads, form, C.byref(self.h)), "map_stream_create")

    def collect(self):
        """(rows of MAP_ROW_DTYPE, stats as Context.map_reads returns them) of the oldest pending batch."""
        rows = np.zeros(max(self.slot_reads, 1), MAP_ROW_DTYPE)
        st, n = PbaMapStats(), C.c_uint32()
        self._call("collect", _ptr(rows), self.slot_reads, C.byref(n), C.byref(st))
        per = [{k: getattr(st.strand[i], k) for k, _ in PbaLocStats._fields_} for i in range(2)]
        return rows[:n.value].copy(), {"strand": per, "n_second_walk": int(st.n_second_walk)}

    def pending(self):
        """(fwd, rc): both sets of the batch collect() would run next, borrowed from its slot (valid until that collect);
        rc is None with strands == 1."""
        f, r = C.c_void_p(), C.c_void_p()
        self._call("pending", C.byref(f), C.byref(r))
        return BorrowedSeqSet(self.ctx, f), (BorrowedSeqSet(self.ctx, r) if r.value else None)


def _map_stream(self, ix, target, R, trials=50, min_len=500, maxn=0, maxm=0, kernel=PBA_KERNEL_AUTO, strands=3,
                slot_bytes=1 << 20, slot_reads=1024, form=PBA_STREAM_TEXT) -> MapStream:
    return MapStream(self, ix, target, R, trials, min_len, maxn, maxm, kernel, strands, slot_bytes, slot_reads, form)


Context.map_stream = _map_stream


class SeqSet:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_seqs_destroy(self.h)
        self.h = None

    __del__ = close

    @property
    def count(self) -> int:
        return self.ctx.lib.pba_seqs_count(self.h)

    @property
    def max_len(self) -> int:
        return self.ctx.lib.pba_seqs_max_len(self.h)

    @property
    def packed_bytes(self) -> int:
        return self.ctx.lib.pba_seqs_packed_bytes(self.h)

    def lengths(self) -> np.ndarray:
        out = np.zeros(max(self.count, 1), np.uint32)
        self.ctx.check(self.ctx.lib.pba_seqs_lengths(self.h, _ptr(out), self.count))
        return out[:self.count]

    def export(self, d_dst_ptr: int, cap: int) -> np.ndarray:
        """Copy the packed arena into a device buffer; returns the byte offset of every sequence in it."""
        offs = np.zeros(max(self.count, 1), np.uint64)
        self.ctx.check(self.ctx.lib.pba_seqs_export(self.ctx.h, self.h, C.c_void_p(d_dst_ptr), cap, _ptr(offs)), "seqs_export")
        return offs[:self.count]

    @property
    def non_acgt(self) -> bool:
        return bool(self.ctx.lib.pba_seqs_non_acgt(self.h))

    def get_text(self, i: int) -> bytes:
        ln = int(self.lengths()[i])
        buf = C.create_string_buffer(ln + 1)
        self.ctx.check(self.ctx.lib.pba_seqs_get_text(self.ctx.h, self.h, i, buf, ln + 1), "get_text")
        return buf.raw[:ln]

    def write_fasta(self, names=None, width: int = 60, lo: int = 0, hi: Optional[int] = None) -> bytes:
        """Sequences [lo, hi) as one FASTA image (pba_seqs_write_fasta: one kernel, one copy, one synchronise).  names: one per
        sequence of the range (str or bytes); None: the decimal index.  Code 3 prints as T."""
        hi = self.count if hi is None else hi
        if names is None:
            nm = no = None
        else:
            bn = [x if isinstance(x, bytes) else str(x).encode("latin-1") for x in names]
            if len(bn) != hi - lo:
                raise ValueError(f"{len(bn)} names for {hi - lo} sequences")
            nm_a, no_a = concat(bn)
            nm_a = np.concatenate([nm_a, np.zeros(1, np.uint8)])
            nm, no = _ptr(nm_a), _ptr(no_a)
        size = C.c_uint64()
        self.ctx.check(self.ctx.lib.pba_seqs_write_fasta(self.ctx.h, self.h, lo, hi, nm, no, width, None, 0, C.byref(size)), "write_fasta")
        out = np.zeros(max(size.value, 1), np.uint8)
        self.ctx.check(self.ctx.lib.pba_seqs_write_fasta(self.ctx.h, self.h, lo, hi, nm, no, width, _ptr(out), size.value, C.byref(size)),
                       "write_fasta")
        return out[:size.value].tobytes()

    def write_fastq(self, qual: "Qual", names=None, lo: int = 0, hi: Optional[int] = None) -> bytes:
        """Sequences [lo, hi) with the qualities of `qual` as one FASTQ image (pba_seqs_write_fastq: one kernel, one copy, the
        bases on one line, quality character '!' + qv).  names: as write_fasta.  qual must have this set's count and lengths."""
        hi = self.count if hi is None else hi
        if names is None:
            nm = no = None
        else:
            bn = [x if isinstance(x, bytes) else str(x).encode("latin-1") for x in names]
            if len(bn) != hi - lo:
                raise ValueError(f"{len(bn)} names for {hi - lo} sequences")
            nm_a, no_a = concat(bn)
            nm_a = np.concatenate([nm_a, np.zeros(1, np.uint8)])
            nm, no = _ptr(nm_a), _ptr(no_a)
        size = C.c_uint64()
        self.ctx.check(self.ctx.lib.pba_seqs_write_fastq(self.ctx.h, self.h, qual.h, lo, hi, nm, no, None, 0, C.byref(size)), "write_fastq")
        out = np.zeros(max(size.value, 1), np.uint8)
        self.ctx.check(self.ctx.lib.pba_seqs_write_fastq(self.ctx.h, self.h, qual.h, lo, hi, nm, no, _ptr(out), size.value, C.byref(size)),
                       "write_fastq")
        return out[:size.value].tobytes()


def qual_phred(agree: int, n: int, qmax: int = PBA_QUAL_QMAX) -> int:
    """pba_qual_phred (host arithmetic): the largest q in [0, qmax] with (max(n - agree, 0) + 1) * S[q] <= (n + 2) * 1000;
    -1 for a qmax outside [0, 60]."""
    return int(_lib.load().pba_qual_phred(agree, n, qmax))


class Qual:
    """The per-base evidence of an evolved set, resident on the device (pba_qual): for every character its qv, the depth and
    agree of the box it came from and src, the input position (PBA_QUAL_SUP set for a character split from a suppliment)."""

    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h

    @classmethod
    def from_arrays(cls, ctx: "Context", lengths, qv, depth=None, agree=None, src=None) -> "Qual":
        """pba_qual_create: sequence k owns the next lengths[k] entries of every array.  depth / agree default to 0, src to the
        position in its sequence."""
        lengths = np.ascontiguousarray(lengths, np.uint32)
        total = int(lengths.astype(np.uint64).sum())
        arrs = []
        for a, dt in ((qv, np.uint8), (depth, np.uint16), (agree, np.uint16), (src, np.uint32)):
            if a is None:
                arrs.append(None)
                continue
            a = np.ascontiguousarray(a, dt)
            if a.size != total:
                raise ValueError(f"{a.size} entries for {total} bases")
            arrs.append(a)
        h = C.c_void_p()
        ctx.check(ctx.lib.pba_qual_create(ctx.h, _ptr(lengths) if lengths.size else None, lengths.size,
                                          *[_ptr(a) if a is not None and a.size else None for a in arrs], C.byref(h)), "qual_create")
        return cls(ctx, h)

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_qual_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def count(self) -> int:
        return self.ctx.lib.pba_qual_count(self.h)

    def lengths(self) -> np.ndarray:
        out = np.zeros(max(self.count, 1), np.uint32)
        self.ctx.check(self.ctx.lib.pba_qual_lengths(self.h, _ptr(out), self.count), "qual_lengths")
        return out[:self.count]

    def get(self, lo: int = 0, hi: Optional[int] = None) -> dict:
        """{"qv", "depth", "agree", "src"} of sequences [lo, hi), back to back."""
        hi = self.count if hi is None else hi
        n = C.c_uint64()
        st = self.ctx.lib.pba_qual_get(self.ctx.h, self.h, lo, hi, None, None, None, None, 1 << 62, C.byref(n))
        self.ctx.check(st, "qual_get")
        cap = n.value
        out = {"qv": np.zeros(max(cap, 1), np.uint8), "depth": np.zeros(max(cap, 1), np.uint16),
               "agree": np.zeros(max(cap, 1), np.uint16), "src": np.zeros(max(cap, 1), np.uint32)}
        self.ctx.check(self.ctx.lib.pba_qual_get(self.ctx.h, self.h, lo, hi, _ptr(out["qv"]), _ptr(out["depth"]), _ptr(out["agree"]),
                                                 _ptr(out["src"]), cap, C.byref(n)), "qual_get")
        return {k: v[:cap] for k, v in out.items()}

    def summary(self, qmin: int) -> np.ndarray:
        """One QUAL_ROW_DTYPE row per sequence, reduced on the device (pba_qual_summary)."""
        rows = np.zeros(max(self.count, 1), QUAL_ROW_DTYPE)
        self.ctx.check(self.ctx.lib.pba_qual_summary(self.ctx.h, self.h, qmin, _ptr(rows), self.count), "qual_summary")
        return rows[:self.count]

    def low_spans(self, qmin: int, min_run: int = 1, cap: Optional[int] = None) -> np.ndarray:
        """The maximal runs of qv < qmin of at least min_run bases as QUAL_SPAN_DTYPE rows sorted by (seq, beg)
        (pba_qual_low_spans).  cap: room for that many; None: all of them (a second call where the first guess was short)."""
        room = 1024 if cap is None else cap
        while True:
            out = np.zeros(max(room, 1), QUAL_SPAN_DTYPE)
            n = C.c_uint64()
            self.ctx.check(self.ctx.lib.pba_qual_low_spans(self.ctx.h, self.h, qmin, min_run, _ptr(out), room, C.byref(n)), "qual_low_spans")
            if cap is not None:
                self.n_low_spans = int(n.value)
                return out[:min(room, n.value)]
            if n.value <= room:
                return out[:n.value]
            room = int(n.value)


class BorrowedSeqSet(SeqSet):
    """A set that belongs to a LocStream slot (LocStream.pending): closing the wrapper frees nothing, and the handle must not
    be used after the collect of its batch or the close of its stream."""

    def close(self):
        self.h = None

    __del__ = close


class Consensus:
    """Vote boxes of an unlocked reference, resident in HBM (ref_seq.h: base_vote, vote_box, elect, evolve)."""

    def __init__(self, ctx: "Context", text: bytes, weight: int = 1, max_len: int = 0):
        self.ctx = ctx
        self.max_len = max_len or max(4 * len(text), 100000)
        self.h = C.c_void_p()
        ctx.check(ctx.lib.pba_cons_create(ctx.h, text, len(text), weight, self.max_len, C.byref(self.h)), "cons_create")

    def __del__(self):
        try:
            if self.h:
                self.ctx.lib.pba_cons_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def extent(self):
        e = np.zeros(3, np.int32)
        self.ctx.check(self.ctx.lib.pba_cons_extent(self.h, _ptr(e)))
        return e.tolist()

    def append(self, seg: bytes):
        self.ctx.check(self.ctx.lib.pba_cons_append(self.ctx.h, self.h, seg, len(seg)), "cons_append")

    def prepend(self, seg: bytes):
        self.ctx.check(self.ctx.lib.pba_cons_prepend(self.ctx.h, self.h, seg, len(seg)), "cons_prepend")

    def elect(self, pos, fwd, scripts, vals):
        """scripts / vals: one uint8 op array and one bytes object per script (vals[k] = the b element of op k)."""
        n = len(scripts)
        off = np.zeros(n + 1, np.uint64)
        off[1:] = np.cumsum([len(x) for x in scripts])
        ops = np.concatenate([np.asarray(x, np.uint8) for x in scripts] + [np.zeros(1, np.uint8)])
        vb = np.frombuffer(b"".join(vals) + b"\0", np.uint8)
        ne = np.array([len(x) for x in scripts], np.int32)
        pos = np.ascontiguousarray(pos, np.int32); fw = np.ascontiguousarray(fwd, np.uint8)
        self.ctx.check(self.ctx.lib.pba_cons_elect(self.ctx.h, self.h, n, _ptr(pos), _ptr(fw), _ptr(ops), _ptr(vb), _ptr(off),
                                                   _ptr(ne)), "cons_elect")

    def vote_pairs(self, A: "SeqSet", ref_seq: int, B: "SeqSet", pairs: np.ndarray, R: float, overlap_min: int = 64,
                   maxn: int = 0, maxm: int = 0) -> np.ndarray:
        """align + gate + elect for a batch, on the device (pba_cons_vote_pairs); returns the alignment results."""
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        out = np.zeros(max(pairs.size, 1), RESULT_DTYPE)
        self.ctx.check(self.ctx.lib.pba_cons_vote_pairs(self.ctx.h, self.h, A.h, ref_seq, B.h, _ptr(pairs), pairs.size, R, maxn, maxm,
                                                        overlap_min, _ptr(out)), "cons_vote_pairs")
        return out[:pairs.size]

    def round(self, reads: "SeqSet", pool, mask: int, R: float, max_trial: int = 32, overlap_min: int = 64,
              buggy_seed_at: bool = False, kernel: int = PBA_KERNEL_AUTO, maxn: int = 26000, maxm: int = 6000):
        """One unlocked round of spaced_seed.cpp:420-446 over the reads `pool` (ids, in order): pba_cons_round.
        Returns (rows of the pool's reads in pool order, stats dict); the caller evolves."""
        pool = np.ascontiguousarray(pool, np.uint32)
        rows = np.zeros(max(reads.count, 1), SS_ROW_DTYPE)
        st = np.zeros(6, np.int32)
        self.ctx.check(self.ctx.lib.pba_cons_round(self.ctx.h, self.h, reads.h, _ptr(pool), pool.size, mask, R, max_trial,
                                                   overlap_min, int(buggy_seed_at), kernel, maxn, maxm, _ptr(rows), _ptr(st)),
                       "cons_round")
        names = ("n_found", "n_batches", "n_grown_fwd", "n_grown_bwd", "n_deferred", "n_index")
        return rows[pool], dict(zip(names, (int(x) for x in st)))

    def assemble(self, reads: "SeqSet", R: float, masks, picks, max_round: int = 100, max_trial: int = 32,
                 overlap_min: int = 64, buggy_seed_at: bool = False, kernel: int = PBA_KERNEL_AUTO, maxn: int = 26000,
                 maxm: int = 6000):
        """spaced_seed's main loop without -l (pba_cons_assemble); returns (rows, found_round, log list of dicts)."""
        n = max(reads.count, 1)
        rows = np.zeros(n, SS_ROW_DTYPE)
        fr = np.zeros(n, np.int32)
        log = np.zeros(max(max_round, 1), np.dtype([("round", "<i4"), ("mask", "<u4"), ("n_tried", "<i4"), ("n_found", "<i4")]))
        rl = np.zeros(max(max_round, 1), np.int32)
        masks = np.ascontiguousarray(masks, np.uint32); picks = np.ascontiguousarray(picks, np.uint32)
        nr = C.c_int()
        self.ctx.check(self.ctx.lib.pba_cons_assemble(self.ctx.h, self.h, reads.h, R, max_trial, overlap_min, int(buggy_seed_at),
                                                      kernel, maxn, maxm, _ptr(masks), masks.size, _ptr(picks), picks.size,
                                                      max_round, _ptr(rows), _ptr(fr), _ptr(log), _ptr(rl), log.size,
                                                      C.byref(nr)), "cons_assemble")
        out = [dict(zip(log.dtype.names, (int(x) for x in l))) for l in log[:nr.value]]
        for k, d in enumerate(out):
            d["ref_len"] = int(rl[k])
        return rows[:reads.count], fr[:reads.count], out

    def evolve(self) -> bytes:
        cap = 3 * self.max_len
        buf = C.create_string_buffer(cap)
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.pba_cons_evolve(self.ctx.h, self.h, buf, cap, C.byref(n)), "cons_evolve")
        return buf.raw[:n.value]

    def dump(self):
        e = self.extent()
        cap = e[1] - e[0]
        sel = np.zeros((max(cap, 1), 4), np.uint16); sup = np.zeros((max(cap, 1), 4), np.uint16); tot = np.zeros(max(cap, 1), np.int32)
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.pba_cons_dump(self.ctx.h, self.h, _ptr(sel), _ptr(sup), _ptr(tot), cap, C.byref(n)), "cons_dump")
        return sel[:n.value], sup[:n.value], tot[:n.value], e

    def text(self) -> bytes:
        e = self.extent()
        cap = e[1] - e[0]
        buf = C.create_string_buffer(cap + 1)
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.pba_cons_text(self.ctx.h, self.h, buf, cap, C.byref(n)), "cons_text")
        return buf.raw[:n.value]


class Pileup:
    """Vote boxes of the reads [t_lo, t_hi) of a set, one segment per read, resident in HBM (pba_pileup): overlap rows vote
    into their target's segment, evolve gives the corrected reads.  No growth."""

    def __init__(self, ctx: "Context", reads: "SeqSet", t_lo: int = 0, t_hi: Optional[int] = None, weight: int = 1):
        self.ctx, self.reads = ctx, reads
        self.t_lo, self.t_hi = t_lo, reads.count if t_hi is None else t_hi
        self.h = C.c_void_p()
        ctx.check(ctx.lib.pba_pileup_create(ctx.h, reads.h, self.t_lo, self.t_hi, weight, C.byref(self.h)), "pileup_create")

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_pileup_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def vote(self, rows: np.ndarray, R: float, reads_rc: Optional["SeqSet"] = None) -> np.ndarray:
        """Vote overlap_strands rows (any order, any mix of strands); returns the re-run's alignment results."""
        rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
        res = np.zeros(max(rows.size, 1), RESULT_DTYPE)
        self.ctx.check(self.ctx.lib.pba_pileup_vote(self.ctx.h, self.h, self.reads.h, reads_rc.h if reads_rc is not None else None,
                                                    _ptr(rows), rows.size, R, _ptr(res)), "pileup_vote")
        return res[:rows.size]

    def vote_mapped(self, reads: "SeqSet", rows: np.ndarray, R: float, overlap_min: int = 64, reads_rc: Optional["SeqSet"] = None):
        """Vote map_reads rows of `reads` against the set this pile-up was made from (pba_pileup_vote_mapped): a found row
        votes if its contig-as-a alignment succeeds with matlen_a >= overlap_min.  Returns (results row by row, rows voted)."""
        rows = np.ascontiguousarray(rows, MAP_ROW_DTYPE)
        res = np.zeros(max(rows.size, 1), RESULT_DTYPE)
        n_voted = C.c_uint64()
        self.ctx.check(self.ctx.lib.pba_pileup_vote_mapped(self.ctx.h, self.h, self.reads.h, reads.h,
                                                           reads_rc.h if reads_rc is not None else None, _ptr(rows), rows.size, R,
                                                           overlap_min, _ptr(res), C.byref(n_voted)), "pileup_vote_mapped")
        return res[:rows.size], int(n_voted.value)

    def vote_placed(self, reads: "SeqSet", rows: np.ndarray, R: float, overlap_min: int = 64, reads_rc: Optional["SeqSet"] = None):
        """Vote placement rows (Layout.place, or any PLACE_ROW_DTYPE rows) of `reads` onto the contig set this pile-up was made
        from (pba_pileup_vote_placed): a found row votes if its alignment from the anchor succeeds with matlen_a >=
        overlap_min.  Returns (results row by row, rows voted)."""
        rows = np.ascontiguousarray(rows, PLACE_ROW_DTYPE)
        res = np.zeros(max(rows.size, 1), RESULT_DTYPE)
        n_voted = C.c_uint64()
        self.ctx.check(self.ctx.lib.pba_pileup_vote_placed(self.ctx.h, self.h, self.reads.h, reads.h,
                                                           reads_rc.h if reads_rc is not None else None, _ptr(rows), rows.size, R,
                                                           overlap_min, _ptr(res), C.byref(n_voted)), "pileup_vote_placed")
        return res[:rows.size], int(n_voted.value)

    def dump(self, target: int):
        """(sel[n, 4], sup[n, 4], tot[n]) of one target's boxes as they stand."""
        n = C.c_int32()
        self.ctx.check(self.ctx.lib.pba_pileup_dump(self.ctx.h, self.h, target, None, None, None, 0, C.byref(n)), "pileup_dump")
        cap = n.value
        sel = np.zeros((max(cap, 1), 4), np.uint16); sup = np.zeros((max(cap, 1), 4), np.uint16); tot = np.zeros(max(cap, 1), np.int32)
        self.ctx.check(self.ctx.lib.pba_pileup_dump(self.ctx.h, self.h, target, _ptr(sel), _ptr(sup), _ptr(tot), cap, C.byref(n)),
                       "pileup_dump")
        return sel[:cap], sup[:cap], tot[:cap]

    def evolve(self):
        """Returns (SeqSet of the corrected reads, rows of CORRECT_ROW_DTYPE); the pile-up is spent afterwards."""
        rows = np.zeros(max(self.t_hi - self.t_lo, 1), CORRECT_ROW_DTYPE)
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pba_pileup_evolve(self.ctx.h, self.h, C.byref(h), _ptr(rows)), "pileup_evolve")
        return SeqSet(self.ctx, h), rows[:self.t_hi - self.t_lo]

    def evolve_qual(self, qmax: int = PBA_QUAL_QMAX):
        """evolve() with the evidence of every character (pba_pileup_evolve_qual).  Returns (SeqSet, rows of CORRECT_ROW_DTYPE,
        Qual); the pile-up is spent afterwards.  A qmax outside [0, 60] is refused and leaves the pile-up usable."""
        rows = np.zeros(max(self.t_hi - self.t_lo, 1), CORRECT_ROW_DTYPE)
        h, qh = C.c_void_p(), C.c_void_p()
        self.ctx.check(self.ctx.lib.pba_pileup_evolve_qual(self.ctx.h, self.h, qmax, C.byref(h), _ptr(rows), C.byref(qh)), "pileup_evolve_qual")
        return SeqSet(self.ctx, h), rows[:self.t_hi - self.t_lo], Qual(self.ctx, qh)


class Layout:
    """The layout of a read set from its overlap rows (pba_layout): containments, the best dovetail at every read end,
    chains of mutual best edges as contigs.  rows(): the per-read table; contigs(): head read, reads and bases per contig;
    stitch(reads): the contigs as a new SeqSet, written on the device."""

    def __init__(self, ctx: "Context", reads: "SeqSet", rows: np.ndarray, hang: int = 64, min_reads: int = 2):
        self.ctx, self.n = ctx, reads.count
        rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
        self.h = C.c_void_p()
        st = _lib.PbaLayoutStats()
        ctx.check(ctx.lib.pba_layout_create(ctx.h, reads.h, _ptr(rows), rows.size, hang, min_reads, C.byref(self.h), C.byref(st)),
                  "layout_create")

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_layout_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stats(self) -> dict:
        st = _lib.PbaLayoutStats()
        self.ctx.check(self.ctx.lib.pba_layout_last_stats(self.h, C.byref(st)), "layout_last_stats")
        return {n: getattr(st, n) for n, _ in _lib.PbaLayoutStats._fields_}

    def rows(self) -> np.ndarray:
        """One LAYOUT_ROW_DTYPE record per read."""
        out = np.zeros(max(self.n, 1), LAYOUT_ROW_DTYPE)
        self.ctx.check(self.ctx.lib.pba_layout_rows(self.ctx.h, self.h, _ptr(out), self.n), "layout_rows")
        return out[:self.n]

    def contigs(self) -> np.ndarray:
        """One LAYOUT_CONTIG_DTYPE record per contig, by ascending head read."""
        nc = int(self.ctx.lib.pba_layout_contigs(self.h))
        head, cnt, length = (np.zeros(max(nc, 1), np.int32) for _ in range(3))
        self.ctx.check(self.ctx.lib.pba_layout_contig_info(self.h, _ptr(head), _ptr(cnt), _ptr(length), nc), "layout_contig_info")
        out = np.zeros(nc, LAYOUT_CONTIG_DTYPE)
        out["head_read"], out["n_reads"], out["length"] = head[:nc], cnt[:nc], length[:nc]
        return out

    def stitch(self, reads: "SeqSet") -> "SeqSet":
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pba_layout_stitch(self.ctx.h, self.h, reads.h, C.byref(h)), "layout_stitch")
        return SeqSet(self.ctx, h)

    def place(self, reads: "SeqSet", rows: np.ndarray) -> np.ndarray:
        """One PLACE_ROW_DTYPE record per read: where overlap_strands `rows` (any rows over `reads`, dir included) anchor it
        on this layout's contigs (pba_layout_place).  The counters of the call are kept in place_stats."""
        rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
        out = np.zeros(max(self.n, 1), PLACE_ROW_DTYPE)
        st = _lib.PbaPlaceStats()
        self.ctx.check(self.ctx.lib.pba_layout_place(self.ctx.h, self.h, reads.h, _ptr(rows), rows.size, _ptr(out), self.n, C.byref(st)),
                       "layout_place")
        self.place_stats = {n: getattr(st, n) for n, _ in _lib.PbaPlaceStats._fields_}
        return out[:self.n]


def _layout(self, reads, rows, hang=64, min_reads=2) -> "Layout":
    """Lay `reads` out into contigs from overlap_strands rows (pba_layout_create)."""
    return Layout(self, reads, rows, hang, min_reads)


def _layout_reads(self, reads, mask, R, max_trial=32, overlap_min=64, hang=64, min_reads=2, strands=3, targets_per_call=10000,
                  kernel=PBA_KERNEL_AUTO, reads_rc=None):
    """overlap_strands_sharded -> layout -> stitch.  Returns (SeqSet of the contigs, the Layout, the overlap rows, [stats of
    the +1 pass, of the -1 pass])."""
    rows, st2 = self.overlap_strands_sharded(reads, mask, R, max_trial, overlap_min, targets_per_call, kernel, strands=strands,
                                             reads_rc=reads_rc)
    lay = self.layout(reads, rows, hang, min_reads)
    return lay.stitch(reads), lay, rows, st2


def _layout_consensus(self, lay, reads, rows, R, overlap_min=64, weight=1, max_boxes=0, reads_rc=None):
    """The consensus of a layout's contigs from the reads its overlap rows place on them (pba_layout_consensus): stitch ->
    place -> vote -> evolve, one round.  max_boxes: a ceiling on the bases of one internal range of contigs (0 = sized from the
    free device memory).  Returns (SeqSet of the contigs, rows of POLISH_ROW_DTYPE per contig, stats: the place counters,
    n_voted, n_chunks, n_contigs, bases in and out and the stage times)."""
    rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
    nc = int(self.lib.pba_layout_contigs(lay.h))
    rows_out = np.zeros(max(nc, 1), POLISH_ROW_DTYPE)
    st = _lib.PbaLayoutConsStats()
    h = C.c_void_p()
    rc_h = reads_rc.h if reads_rc is not None else None
    self.check(self.lib.pba_layout_consensus(self.h, lay.h, reads.h, rc_h, _ptr(rows), rows.size, R, overlap_min, weight, max_boxes,
                                             C.byref(h), _ptr(rows_out), C.byref(st)), "layout_consensus")
    stats = {n: getattr(st.place, n) for n, _ in _lib.PbaPlaceStats._fields_}
    stats.update({n: getattr(st, n) for n, _ in _lib.PbaLayoutConsStats._fields_ if n != "place"})
    return SeqSet(self, h), rows_out[:nc], stats


def _layout_consensus_qual(self, lay, reads, rows, R, overlap_min=64, weight=1, max_boxes=0, reads_rc=None, qmax=PBA_QUAL_QMAX):
    """layout_consensus with the evidence of the contigs it returns (pba_layout_consensus_qual): its returns with the Qual
    appended."""
    rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
    nc = int(self.lib.pba_layout_contigs(lay.h))
    rows_out = np.zeros(max(nc, 1), POLISH_ROW_DTYPE)
    st = _lib.PbaLayoutConsStats()
    h, qh = C.c_void_p(), C.c_void_p()
    rc_h = reads_rc.h if reads_rc is not None else None
    self.check(self.lib.pba_layout_consensus_qual(self.h, lay.h, reads.h, rc_h, _ptr(rows), rows.size, R, overlap_min, weight, max_boxes,
                                                  C.byref(h), _ptr(rows_out), C.byref(st), qmax, C.byref(qh)), "layout_consensus_qual")
    stats = {n: getattr(st.place, n) for n, _ in _lib.PbaPlaceStats._fields_}
    stats.update({n: getattr(st, n) for n, _ in _lib.PbaLayoutConsStats._fields_ if n != "place"})
    return SeqSet(self, h), rows_out[:nc], stats, Qual(self, qh)


def _polish_contigs_qual(self, target, reads, mask, R, trials=50, min_len=500, maxn=0, maxm=0, kernel=PBA_KERNEL_AUTO, strands=3,
                         overlap_min=64, weight=1, rounds=1, reads_rc=None, max_boxes=0, qmax=PBA_QUAL_QMAX):
    """polish_contigs with the evidence of the LAST round (pba_polish_contigs_qual; src addresses the contigs that entered
    that round): its returns with the Qual appended."""
    rows = np.zeros(max(target.count, 1), POLISH_ROW_DTYPE)
    log = np.zeros(max(rounds, 1), POLISH_LOG_DTYPE)
    h, qh = C.c_void_p(), C.c_void_p()
    rc_h = reads_rc.h if reads_rc is not None else None
    st = self.lib.pba_polish_contigs_qual(self.h, target.h, reads.h, rc_h, mask, R, trials, min_len, maxn, maxm, kernel, strands,
                                          overlap_min, weight, rounds, max_boxes, C.byref(h), _ptr(rows), _ptr(log), log.size, qmax,
                                          C.byref(qh))
    self.check(st, "polish_contigs_qual")
    return SeqSet(self, h), rows[:target.count], log[:max(rounds, 0)], Qual(self, qh)


def _correct_reads_qual(self, reads, mask, R, max_trial=32, overlap_min=64, strands=3, weight=1, t_lo=0, t_hi=None,
                        kernel=PBA_KERNEL_AUTO, reads_rc=None, max_boxes=0, qmax=PBA_QUAL_QMAX):
    """correct_reads with the evidence of the corrected reads (pba_correct_reads_qual), whatever the chunk cut: its returns
    with the Qual appended."""
    t_hi = reads.count if t_hi is None else t_hi
    rows = np.zeros(max(t_hi - t_lo, 1), CORRECT_ROW_DTYPE)
    st2 = (_lib.PbaOverlapStats * 2)()
    h, qh = C.c_void_p(), C.c_void_p()
    rc_h = reads_rc.h if reads_rc is not None else None
    st = self.lib.pba_correct_reads_qual(self.h, reads.h, rc_h, t_lo, t_hi, mask, R, max_trial, overlap_min, kernel, strands, weight,
                                         max_boxes, C.byref(h), _ptr(rows), C.byref(st2), qmax, C.byref(qh))
    self.check(st, "correct_reads_qual")
    return SeqSet(self, h), rows[:max(t_hi - t_lo, 0)], _stats_pair(st2), Qual(self, qh)


Context.layout = _layout
Context.layout_reads = _layout_reads
Context.layout_consensus = _layout_consensus
Context.layout_consensus_qual = _layout_consensus_qual
Context.polish_contigs_qual = _polish_contigs_qual
Context.correct_reads_qual = _correct_reads_qual


class Clip:
    """The clip table of a read set from its overlap rows (pba_clip): per-base coverage by the row intervals that span a base
    with `margin` on both sides, the longest run of bases with coverage >= min_cov, extended by the margin.  rows(): the
    per-read table; apply(reads): the clipped reads as a new SeqSet, written on the device.  The rows the table was made
    from are stale for the clipped set: run the overlapper again."""

    def __init__(self, ctx: "Context", reads: "SeqSet", rows: np.ndarray, margin: int = 100, min_cov: int = 2, min_len: int = 0,
                 roles: int = 3, keep_unseen: bool = False, max_bases: int = 0):
        self.ctx, self.n = ctx, reads.count
        rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
        self.h = C.c_void_p()
        st = _lib.PbaClipStats()
        flags = int(roles) | (PBA_CLIP_KEEP_UNSEEN if keep_unseen else 0)
        ctx.check(ctx.lib.pba_clip_create(ctx.h, reads.h, _ptr(rows), rows.size, margin, min_cov, min_len, flags, max_bases,
                                          C.byref(self.h), C.byref(st)), "clip_create")

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_clip_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stats(self) -> dict:
        st = _lib.PbaClipStats()
        self.ctx.check(self.ctx.lib.pba_clip_last_stats(self.h, C.byref(st)), "clip_last_stats")
        return {n: getattr(st, n) for n, _ in _lib.PbaClipStats._fields_}

    def rows(self) -> np.ndarray:
        """One CLIP_ROW_DTYPE record per read."""
        out = np.zeros(max(self.n, 1), CLIP_ROW_DTYPE)
        self.ctx.check(self.ctx.lib.pba_clip_rows(self.ctx.h, self.h, _ptr(out), self.n), "clip_rows")
        return out[:self.n]

    def apply(self, reads: "SeqSet") -> "SeqSet":
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.pba_clip_apply(self.ctx.h, self.h, reads.h, C.byref(h)), "clip_apply")
        return SeqSet(self.ctx, h)


def _clip(self, reads, rows, margin=100, min_cov=2, min_len=0, roles=3, keep_unseen=False, max_bases=0) -> "Clip":
    """The clip table of `reads` from overlap_strands rows (pba_clip_create).  roles: 1 = the rows' target intervals, 2 = their
    query intervals, 3 = both."""
    return Clip(self, reads, rows, margin, min_cov, min_len, roles, keep_unseen, max_bases)


def _clip_coverage(self, reads, rows, read, margin=100, roles=3) -> np.ndarray:
    """cov[0 .. L) of one read: how many counted intervals span each base with `margin` on both sides (pba_clip_coverage)."""
    rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
    n = C.c_uint32()
    self.check(self.lib.pba_clip_coverage(self.h, reads.h, _ptr(rows), rows.size, margin, roles, read, None, 0, C.byref(n)), "clip_coverage")
    out = np.zeros(max(n.value, 1), np.int32)
    self.check(self.lib.pba_clip_coverage(self.h, reads.h, _ptr(rows), rows.size, margin, roles, read, _ptr(out), n.value, C.byref(n)),
               "clip_coverage")
    return out[:n.value]


def _clip_reads(self, reads, mask, R, max_trial=32, overlap_min=64, margin=100, min_cov=2, min_len=0, roles=3, keep_unseen=False,
                max_bases=0, strands=3, targets_per_call=10000, kernel=PBA_KERNEL_AUTO, reads_rc=None):
    """overlap_strands_sharded -> clip -> apply.  Returns (SeqSet of the clipped reads, the clip table as CLIP_ROW_DTYPE records,
    the overlap rows, the Clip's stats).  The rows belong to the UNCLIPPED set: overlap the clipped set again before a layout."""
    rows, _ = self.overlap_strands_sharded(reads, mask, R, max_trial, overlap_min, targets_per_call, kernel, strands=strands,
                                           reads_rc=reads_rc)
    clip = self.clip(reads, rows, margin, min_cov, min_len, roles, keep_unseen, max_bases)
    clipped, table = clip.apply(reads), clip.rows()
    stats = clip.stats
    clip.close()
    return clipped, table, rows, stats


Context.clip = _clip
Context.clip_coverage = _clip_coverage
Context.clip_reads = _clip_reads


# ---- per-window alignment counts and rows trimmed where they break (pba_windows.hip)
def windows_bound(a_pos: int, a_len: int, b_len: int, R: float, W: int, a_backward: bool = False) -> int:
    """Windows the clipped len_a of a pair touches: the bound on n_win (pba_windows_bound; host arithmetic)."""
    return int(_lib.load().pba_windows_bound(a_pos, a_len, b_len, R, W, int(bool(a_backward))))


def windows_from_script(ops, a_elems: bytes, b_elems: bytes, a_pos: int, a_backward: bool, W: int, flags: int = 0) -> np.ndarray:
    """The windows (ALN_COUNTS_DTYPE) of a script and the elements of its two accessors in element order
    (pba_windows_from_script): the host twin of the device sink."""
    ops = np.ascontiguousarray(ops, np.uint8)
    cap = max(windows_bound(a_pos, len(a_elems), len(a_elems), 0.5, W, a_backward), 1) + 1
    win = np.zeros(cap, ALN_COUNTS_DTYPE)
    n = _lib.load().pba_windows_from_script(_ptr(ops), ops.size, a_elems, b_elems, a_pos, int(bool(a_backward)), W, flags, _ptr(win), cap)
    if n < 0 or n > cap:
        raise PbaError(_lib.PBA_E_INVALID, "windows_from_script")
    return win[:n]


def trim_rows_apply(rows: np.ndarray, trims: np.ndarray) -> np.ndarray:
    """The rows that are not DROPPED with their four interval ends replaced by the trimmed ones (pba_trim_rows_apply).  INTERVAL
    ROWS: good for clip, which reads only target, query, strand and the four ends; not for anything that re-runs the alignment."""
    rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
    trims = np.ascontiguousarray(trims, TRIM_ROW_DTYPE)
    if rows.size != trims.size:
        raise PbaError(_lib.PBA_E_INVALID, "trim_rows_apply: one trim per row")
    out = np.zeros(max(rows.size, 1), STRAND_OVERLAP_DTYPE)
    n = _lib.load().pba_trim_rows_apply(_ptr(rows), _ptr(trims), rows.size, _ptr(out))
    if n < 0:
        raise PbaError(_lib.PBA_E_INVALID, "trim_rows_apply")
    return out[:n]


def _align_batch_windows(self, A, B, pairs, R, W, maxn=0, maxm=0, flags=0):
    """The alignments of a batch as per-window counts on a's own grid of W bases (pba_align_batch_windows), made on the device
    from the traceback walk.  Returns (results, list of window arrays of ALN_COUNTS_DTYPE -- views into one array --, counts)."""
    pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
    n = pairs.size
    out = np.zeros(n, RESULT_DTYPE)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([windows_bound(int(p["a_pos"]), int(p["a_len"]), int(p["b_len"]), R, W, int(p["flags"]) & 1)     # PBA_A_BACKWARD
                         for p in pairs], dtype=np.uint64) if n else 0
    win = np.zeros(int(off[-1]) + 1, ALN_COUNTS_DTYPE)
    nwin = np.zeros(max(n, 1), np.int32)
    counts = np.zeros(max(n, 1), ALN_COUNTS_DTYPE)
    self.check(self.lib.pba_align_batch_windows(self.h, A.h, B.h, _ptr(pairs), n, R, maxn, maxm, W, flags, _ptr(out), _ptr(win), _ptr(off),
                                                _ptr(nwin), _ptr(counts)), "align_batch_windows")
    return out, [win[int(off[q]):int(off[q]) + int(nwin[q])] for q in range(n)], counts[:n]


def _rows_windows(self, fn, what, head, rows, dtype, R, W, cap, max_slots):
    rows = np.ascontiguousarray(rows, dtype)
    n = rows.size
    off = np.zeros(n + 1, np.uint64)
    counts = np.zeros(max(n, 1), ALN_COUNTS_DTYPE)
    res = np.zeros(max(n, 1), RESULT_DTYPE)
    total = C.c_uint64()
    if cap is None:                                  # one call to learn the total, one to fetch: the windows are not kept between
        self.check(fn(self.h, *head, _ptr(rows), n, R, W, None, 0, _ptr(off), C.byref(total), None, None, max_slots), what)
        cap = total.value
    win = np.zeros(max(int(cap), 1), ALN_COUNTS_DTYPE)
    self.check(fn(self.h, *head, _ptr(rows), n, R, W, _ptr(win), int(cap), _ptr(off), C.byref(total), _ptr(counts), _ptr(res), max_slots), what)
    wins, pos_ok = [], True
    for k in range(n):
        pos_ok = pos_ok and int(off[k + 1]) <= int(cap)
        wins.append(win[int(off[k]):int(off[k + 1])] if pos_ok else None)
    return wins, counts[:n], off, res[:n], total.value


def _map_windows(self, target, reads, rows, R, W, reads_rc=None, cap=None, max_slots=0):
    """Per-window counts of map_reads rows on the read's own grid (pba_map_rows_windows_budget).  Returns (windows per row --
    views into one array, None for a row beyond cap --, counts, offsets, results, total windows)."""
    head = (target.h, reads.h, reads_rc.h if reads_rc is not None else None)
    return _rows_windows(self, self.lib.pba_map_rows_windows_budget, "map_windows", head, rows, MAP_ROW_DTYPE, R, W, cap, max_slots)


def _overlap_windows(self, reads, rows, R, W, reads_rc=None, cap=None, max_slots=0):
    """Per-window counts of overlap_strands rows on the TARGET's own grid, in the target's forward order, I / D named with the
    query read as the query (pba_overlap_rows_windows_budget).  Returns what map_windows returns."""
    head = (reads.h, reads_rc.h if reads_rc is not None else None)
    return _rows_windows(self, self.lib.pba_overlap_rows_windows_budget, "overlap_windows", head, rows, STRAND_OVERLAP_DTYPE, R, W, cap,
                         max_slots)


def _windows_trim(self, wins, W, max_err, min_span):
    """The trim rule on windows the caller supplies (pba_windows_trim): wins is a list of ALN_COUNTS_DTYPE arrays, one per item,
    I / D named as under the default flags.  Returns TRIM_SPAN_DTYPE records."""
    n = len(wins)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(w) for w in wins], dtype=np.uint64) if n else 0
    flat = np.zeros(int(off[-1]) + 1, ALN_COUNTS_DTYPE)
    for k, w in enumerate(wins):
        flat[int(off[k]):int(off[k + 1])] = w
    spans = np.zeros(max(n, 1), TRIM_SPAN_DTYPE)
    self.check(self.lib.pba_windows_trim(self.h, _ptr(flat), _ptr(off), n, W, max_err, min_span, _ptr(spans)), "windows_trim")
    return spans[:n]


def _overlap_trim(self, reads, rows, R, W=100, max_err=0.25, min_span=64, reads_rc=None, max_slots=0):
    """overlap_strands rows trimmed to their longest run of good target windows (pba_overlap_rows_trim_budget): windows and the
    trim rule on the device.  Returns (TRIM_ROW_DTYPE records, one per row; stats dict)."""
    rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
    out = np.zeros(max(rows.size, 1), TRIM_ROW_DTYPE)
    st = _lib.PbaTrimStats()
    self.check(self.lib.pba_overlap_rows_trim_budget(self.h, reads.h, reads_rc.h if reads_rc is not None else None, _ptr(rows), rows.size, R,
                                                     W, max_err, min_span, _ptr(out), C.byref(st), max_slots), "overlap_trim")
    return out[:rows.size], {n: getattr(st, n) for n, _ in _lib.PbaTrimStats._fields_}


def _clip_reads_trimmed(self, reads, mask, R, W=100, max_err=0.25, min_span=64, max_trial=32, overlap_min=64, margin=100, min_cov=2,
                        min_len=0, roles=3, keep_unseen=False, max_bases=0, strands=3, targets_per_call=10000, kernel=PBA_KERNEL_AUTO,
                        reads_rc=None):
    """overlap_strands_sharded -> overlap_trim -> trim_rows_apply -> clip -> apply: clip_reads with every row first narrowed to
    its longest run of good W-base target windows, so that a row an alignment carried across a junction stops there.  Returns
    (SeqSet of the clipped reads, the clip table, the UNTRIMMED overlap rows, the Clip's stats, the trim records, the trim stats).
    A strand -1 row needs the reverse complements: reads_rc is built when it is not given."""
    rc_own = None
    if reads_rc is None and strands != 1:
        reads_rc = rc_own = self.seqs_revcomp(reads)
    try:
        rows, _ = self.overlap_strands_sharded(reads, mask, R, max_trial, overlap_min, targets_per_call, kernel, strands=strands,
                                               reads_rc=reads_rc)
        trims, tstats = self.overlap_trim(reads, rows, R, W, max_err, min_span, reads_rc=reads_rc)
    finally:
        if rc_own is not None:
            rc_own.close()
    clip = self.clip(reads, trim_rows_apply(rows, trims), margin, min_cov, min_len, roles, keep_unseen, max_bases)
    clipped, table = clip.apply(reads), clip.rows()
    stats = clip.stats
    clip.close()
    return clipped, table, rows, stats, trims, tstats


class Sites:
    """The variant sites of a target range, resident on the device (pba_sites): records of SITE_DTYPE sorted by (target, pos,
    kind).  Independent of the pile-up it was scanned from."""

    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_sites_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def count(self) -> int:
        return int(self.ctx.lib.pba_sites_count(self.h))

    @property
    def count_sel(self) -> int:
        return int(self.ctx.lib.pba_sites_count_sel(self.h))

    def target_range(self, target: int):
        """(lo, hi): records [lo, hi) are the target's."""
        lo, hi = C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx.lib.pba_sites_target_range(self.h, target, C.byref(lo), C.byref(hi)), "sites_target_range")
        return int(lo.value), int(hi.value)

    def get(self, lo: int = 0, hi: Optional[int] = None) -> np.ndarray:
        hi = self.count if hi is None else hi
        out = np.zeros(max(hi - lo, 1), SITE_DTYPE)
        self.ctx.check(self.ctx.lib.pba_sites_get(self.ctx.h, self.h, lo, hi, _ptr(out)), "sites_get")
        return out[:max(hi - lo, 0)]


def _pileup_sites(self, min_depth: int, min_alt: int, min_permille: int) -> "Sites":
    """The sites of the boxes as they stand, before evolve (pba_pileup_sites); the pile-up is only read."""
    h = C.c_void_p()
    self.ctx.check(self.ctx.lib.pba_pileup_sites(self.ctx.h, self.h, self.reads.h, min_depth, min_alt, min_permille, C.byref(h)), "pileup_sites")
    return Sites(self.ctx, h)


Pileup.sites = _pileup_sites


def _sites_create(self, seqs, recs, t_lo: int = 0, t_hi: Optional[int] = None) -> "Sites":
    """A Sites from a list of SITE_DTYPE records for the sequences [t_lo, t_hi) of seqs (pba_sites_create)."""
    recs = np.ascontiguousarray(recs, SITE_DTYPE)
    h = C.c_void_p()
    self.check(self.lib.pba_sites_create(self.h, seqs.h, t_lo, seqs.count if t_hi is None else t_hi, _ptr(recs) if recs.size else None,
                                         recs.size, C.byref(h)), "sites_create")
    return Sites(self, h)


def _rows_alleles(self, fn, what, head, rows, dtype, mid, sites, cap, max_slots):
    rows = np.ascontiguousarray(rows, dtype)
    n = rows.size
    off = np.zeros(n + 1, np.uint64)
    sums = np.zeros(max(n, 1), ALLELE_COUNTS_DTYPE)
    res = np.zeros(max(n, 1), RESULT_DTYPE)
    total = C.c_uint64()
    if cap is None:                                  # one call to learn the total, one to fetch
        self.check(fn(self.h, *head, _ptr(rows), n, *mid, sites.h, None, 0, _ptr(off), C.byref(total), None, None, max_slots), what)
        cap = total.value
    out = np.zeros(max(int(cap), 1), ALLELE_DTYPE)
    self.check(fn(self.h, *head, _ptr(rows), n, *mid, sites.h, _ptr(out), int(cap), _ptr(off), C.byref(total), _ptr(sums), _ptr(res), max_slots),
               what)
    whole = int(off[np.searchsorted(off, cap, side="right") - 1]) if n else 0      # the rows that fit cap, whole
    return out[:whole], off, sums[:n], res[:n]


def _overlap_alleles(self, reads, rows, R, sites, reads_rc=None, cap=None, max_slots=0):
    """Every overlap_strands row's allele at the SEL sites of its target (pba_overlap_rows_alleles_budget).  Returns (records of
    ALLELE_DTYPE for the rows that fit cap, offsets -- n + 1, always complete --, per-row totals, results)."""
    head = (reads.h, reads_rc.h if reads_rc is not None else None)
    return _rows_alleles(self, self.lib.pba_overlap_rows_alleles_budget, "overlap_alleles", head, rows, STRAND_OVERLAP_DTYPE, (R,), sites, cap,
                         max_slots)


def _map_alleles(self, target, reads, rows, R, sites, overlap_min=64, reads_rc=None, cap=None, max_slots=0):
    """Every map_reads row's allele at the SEL sites of its contig, in the row's voting roles under vote_mapped's gate
    (pba_map_rows_alleles_budget).  Returns what overlap_alleles returns."""
    head = (target.h, reads.h, reads_rc.h if reads_rc is not None else None)
    return _rows_alleles(self, self.lib.pba_map_rows_alleles_budget, "map_alleles", head, rows, MAP_ROW_DTYPE, (R, overlap_min), sites, cap,
                         max_slots)


def sites_tsv_lines(sites, names=None):
    """One line per record (a Sites, or records of SITE_DTYPE): target, 1-based position, kind, own / major / minor as letters
    (`-` for DEL), n, n_major, n_minor."""
    letters = "ACGT-"
    for r in (sites.get() if isinstance(sites, Sites) else sites):
        t = int(r["target"])
        yield "\t".join([str(names[t]) if names is not None else str(t), str(int(r["pos"]) + 1), "SEL" if int(r["kind"]) == PBA_SITE_SEL else "SUP",
                          letters[int(r["own"])], letters[int(r["major"])], letters[int(r["minor"])], str(int(r["n"])), str(int(r["n_major"])),
                          str(int(r["n_minor"]))])


def _phase_params(n_iter, min_margin, self_weight) -> np.ndarray:
    p = np.zeros(1, PHASE_PARAMS_DTYPE)
    p["n_iter"], p["min_margin"], p["self_weight"] = n_iter, min_margin, self_weight
    return p


def _stats_dict(st: np.ndarray) -> dict:
    return {n: (float(st[0][n]) if n.endswith("_ms") else int(st[0][n])) for n in st.dtype.names}


def _alleles_phase(self, sites, rows_records, n_iter=2, min_margin=2, self_weight=1, want_sites=True):
    """The phase rule on allele records the caller supplies (pba_alleles_phase): rows_records is a list of ALLELE_DTYPE arrays (or
    of lists of (site, allele)), one per row.  Returns (PHASE_ROW_DTYPE records, PHASE_SITE_DTYPE records -- one per SEL site
    of `sites`, None without want_sites --, stats dict)."""
    n = len(rows_records)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in rows_records], dtype=np.uint64) if n else 0
    flat = np.zeros(int(off[-1]) + 1, ALLELE_DTYPE)
    for k, r in enumerate(rows_records):
        if len(r):
            flat[int(off[k]):int(off[k + 1])] = r if isinstance(r, np.ndarray) else np.array([tuple(x) for x in r], ALLELE_DTYPE)
    out = np.zeros(max(n, 1), PHASE_ROW_DTYPE)
    so = np.zeros(max(sites.count_sel, 1), PHASE_SITE_DTYPE) if want_sites else None
    st = np.zeros(1, PHASE_STATS_DTYPE)
    p = _phase_params(n_iter, min_margin, self_weight)
    self.check(self.lib.pba_alleles_phase(self.h, sites.h, _ptr(flat), _ptr(off), n, _ptr(p), _ptr(out), _ptr(so) if want_sites else None,
                                          _ptr(st)), "alleles_phase")
    return out[:n], (so[:sites.count_sel] if want_sites else None), _stats_dict(st)


def _overlap_phase(self, reads, rows, R, sites, n_iter=2, min_margin=2, self_weight=1, reads_rc=None, max_slots=0, want_sites=True):
    """overlap_strands rows phased by their alleles at the SEL sites of their targets (pba_overlap_rows_phase_budget): the allele
    walk and the phase rule on the device.  Returns (PHASE_ROW_DTYPE records, one per row; PHASE_SITE_DTYPE records; stats
    dict; results)."""
    rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
    n = rows.size
    out = np.zeros(max(n, 1), PHASE_ROW_DTYPE)
    so = np.zeros(max(sites.count_sel, 1), PHASE_SITE_DTYPE) if want_sites else None
    st = np.zeros(1, PHASE_STATS_DTYPE)
    res = np.zeros(max(n, 1), RESULT_DTYPE)
    p = _phase_params(n_iter, min_margin, self_weight)
    self.check(self.lib.pba_overlap_rows_phase_budget(self.h, reads.h, reads_rc.h if reads_rc is not None else None, _ptr(rows), n, R, sites.h,
                                                      _ptr(p), _ptr(out), _ptr(so) if want_sites else None, _ptr(st), _ptr(res), max_slots),
               "overlap_phase")
    return out[:n], (so[:sites.count_sel] if want_sites else None), _stats_dict(st), res[:n]


def phase_rows_apply(rows: np.ndarray, phase: np.ndarray, keep_unphased: bool = True) -> np.ndarray:
    """The rows the phase rule puts on the target's own copy (label > 0), with the undecided ones (label == 0) under
    keep_unphased, in order and unchanged (pba_phase_rows_apply): good for every call that takes overlap rows."""
    rows = np.ascontiguousarray(rows, STRAND_OVERLAP_DTYPE)
    phase = np.ascontiguousarray(phase, PHASE_ROW_DTYPE)
    if rows.size != phase.size:
        raise PbaError(_lib.PBA_E_INVALID, "phase_rows_apply: one phase record per row")
    out = np.zeros(max(rows.size, 1), STRAND_OVERLAP_DTYPE)
    n = _lib.load().pba_phase_rows_apply(_ptr(rows), _ptr(phase), rows.size, int(bool(keep_unphased)), _ptr(out))
    if n < 0:
        raise PbaError(_lib.PBA_E_INVALID, "phase_rows_apply")
    return out[:n]


def _correct_reads_phased(self, reads, mask, R, thresholds=(8, 3, 250), n_iter=2, min_margin=2, self_weight=1, keep_unphased=True,
                          max_trial=32, overlap_min=64, strands=3, weight=1, t_lo=0, t_hi=None, kernel=PBA_KERNEL_AUTO, reads_rc=None,
                          max_boxes=0):
    """correct_reads with every target voted only by the rows the phase rule does not put on the other copy
    (pba_correct_reads_phased_budget): thresholds = (min_depth, min_alt, min_permille) of the site scan.  Returns (SeqSet of the
    corrected reads, rows of CORRECT_ROW_DTYPE -- n_rows counts the rows kept --, phase stats dict summed over the chunks, [stats
    of the +1 pass, of the -1 pass])."""
    t_hi = reads.count if t_hi is None else t_hi
    rows = np.zeros(max(t_hi - t_lo, 1), CORRECT_ROW_DTYPE)
    st2 = (_lib.PbaOverlapStats * 2)()
    pst = np.zeros(1, PHASE_STATS_DTYPE)
    p = _phase_params(n_iter, min_margin, self_weight)
    h = C.c_void_p()
    self.check(self.lib.pba_correct_reads_phased_budget(self.h, reads.h, reads_rc.h if reads_rc is not None else None, t_lo, t_hi, mask, R,
                                                        max_trial, overlap_min, kernel, strands, weight, max_boxes, *thresholds, _ptr(p),
                                                        int(bool(keep_unphased)), C.byref(h), _ptr(rows), _ptr(pst), C.byref(st2)),
               "correct_reads_phased")
    return SeqSet(self, h), rows[:max(t_hi - t_lo, 0)], _stats_dict(pst), _stats_pair(st2)


Context.alleles_phase = _alleles_phase
Context.overlap_phase = _overlap_phase
Context.correct_reads_phased = _correct_reads_phased
Context.sites_create = _sites_create
Context.overlap_alleles = _overlap_alleles
Context.map_alleles = _map_alleles
Context.align_batch_windows = _align_batch_windows
Context.map_windows = _map_windows
Context.overlap_windows = _overlap_windows
Context.windows_trim = _windows_trim
Context.overlap_trim = _overlap_trim
Context.clip_reads_trimmed = _clip_reads_trimmed


class Hpc:
    """The run starts of one homopolymer compression, resident on the device (pba_hpc): S[k] = the original position of head k of
    every sequence, S[H] = L.  lengths(): (L, H) of every sequence; run_starts(i): S of one; lift_overlaps / lift_map_rows: rows
    found on the compressed set into rows on the original one.  A lifted row keeps the cost of the compressed alignment."""

    def __init__(self, ctx: "Context", h):
        self.ctx, self.h = ctx, h
        self.n = int(ctx.lib.pba_hpc_count(h))

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_hpc_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stats(self) -> dict:
        st = _lib.PbaHpcStats()
        self.ctx.check(self.ctx.lib.pba_hpc_last_stats(self.h, C.byref(st)), "hpc_last_stats")
        return {n: getattr(st, n) for n, _ in _lib.PbaHpcStats._fields_}

    def lengths(self):
        """(original lengths, compressed lengths), one u32 each per sequence."""
        a, b = np.zeros(max(self.n, 1), np.uint32), np.zeros(max(self.n, 1), np.uint32)
        self.ctx.check(self.ctx.lib.pba_hpc_lengths(self.h, _ptr(a), _ptr(b), self.n), "hpc_lengths")
        return a[:self.n], b[:self.n]

    def run_starts(self, i: int) -> np.ndarray:
        """S[0 .. H] of sequence i (H + 1 entries, the last one its original length)."""
        n = C.c_uint32()
        self.ctx.check(self.ctx.lib.pba_hpc_run_starts(self.ctx.h, self.h, i, None, 0, C.byref(n)), "hpc_run_starts")
        out = np.zeros(n.value, np.uint32)
        self.ctx.check(self.ctx.lib.pba_hpc_run_starts(self.ctx.h, self.h, i, _ptr(out), n.value, C.byref(n)), "hpc_run_starts")
        return out

    def lift_overlaps(self, rows: np.ndarray) -> np.ndarray:
        """overlap_strands rows of the compressed set as rows of the original set (pba_hpc_lift_overlaps); a new array."""
        out = np.array(rows, STRAND_OVERLAP_DTYPE, order="C")
        self.ctx.check(self.ctx.lib.pba_hpc_lift_overlaps(self.ctx.h, self.h, _ptr(out), out.size, _ptr(out)), "hpc_lift_overlaps")
        return out

    def lift_map_rows(self, rows: np.ndarray, target_hpc: "Hpc") -> np.ndarray:
        """map_reads rows of the compressed reads (this map) against the compressed contigs (target_hpc) as rows of the original
        sets (pba_hpc_lift_map_rows); a new array."""
        out = np.array(rows, MAP_ROW_DTYPE, order="C")
        self.ctx.check(self.ctx.lib.pba_hpc_lift_map_rows(self.ctx.h, self.h, target_hpc.h, _ptr(out), out.size, _ptr(out)),
                       "hpc_lift_map_rows")
        return out


def _seqs_hpc(self, S, max_bases=0):
    """(SeqSet, Hpc): S with every homopolymer run collapsed to one base, written on the device in seqs_from_text's layout
    whatever layout S has, and the map that lifts rows found on it back (pba_seqs_hpc).  max_bases: input bases per internal
    chunk (0 = the default); the result does not depend on it."""
    h, mh = C.c_void_p(), C.c_void_p()
    self.check(self.lib.pba_seqs_hpc(self.h, S.h, max_bases, C.byref(h), C.byref(mh), None), "seqs_hpc")
    return SeqSet(self, h), Hpc(self, mh)


def _overlap_hpc(self, reads, mask, R, max_trial=32, overlap_min=64, strands=3, targets_per_call=10000, kernel=PBA_KERNEL_AUTO):
    """seqs_hpc -> overlap_strands_sharded on the compressed reads -> lift_overlaps.  Returns (rows in the coordinates of `reads`,
    [stats of the +1 pass, of the -1 pass], the Hpc).  overlap_min and R apply to the compressed texts; a row's cost is that of
    the compressed alignment: clip / layout / layout_consensus take the rows, pileup_vote and overlap_rows_cigar refuse them."""
    comp, hpc = self.seqs_hpc(reads)
    rows, st2 = self.overlap_strands_sharded(comp, mask, R, max_trial, overlap_min, targets_per_call, kernel, strands=strands)
    comp.close()
    return hpc.lift_overlaps(rows), st2, hpc


Context.seqs_hpc = _seqs_hpc
Context.overlap_hpc = _overlap_hpc


_INDEX_MODES = {"all": PBA_INDEX_ALL, "head_tail": PBA_INDEX_HEAD_TAIL}


def census_cutoff(hist: np.ndarray, fraction: float, floor: int = 1) -> int:
    """pba_census_cutoff (host arithmetic): the smallest occurrence count c >= max(floor, 1) that leaves at most
    int(fraction * n_distinct) distinct keys above it; PbaError(PBA_E_TOOLONG) when the histogram is too short to tell."""
    hist = np.ascontiguousarray(hist, np.uint64)
    out = C.c_uint32()
    st = _lib.load().pba_census_cutoff(_ptr(hist), hist.size, fraction, floor, C.byref(out))
    if st != _lib.PBA_OK:
        raise PbaError(st, "census_cutoff")
    return int(out.value)


class Census:
    """How often every masked seed key occurs among the positions the seed index visits (pba_census): one u32 counter per
    value of the mask's care bits, resident on the device."""

    def __init__(self, ctx: "Context", seqs: "SeqSet", mask: int, mode="head_tail", lo: int = 0, hi: Optional[int] = None):
        self.ctx, self.mask = ctx, mask
        self.mode = _INDEX_MODES.get(mode, mode)
        self.h = C.c_void_p()
        ctx.check(ctx.lib.pba_census_create(ctx.h, seqs.h, lo, seqs.count if hi is None else hi, mask, self.mode, C.byref(self.h)),
                  "census_create")

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_census_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, seqs: "SeqSet", lo: int = 0, hi: Optional[int] = None):
        """further sequences -- of this or of another set -- into the same counters"""
        self.ctx.check(self.ctx.lib.pba_census_add(self.ctx.h, self.h, seqs.h, lo, seqs.count if hi is None else hi), "census_add")
        return self

    @property
    def stats(self) -> dict:
        st = _lib.PbaCensusStats()
        self.ctx.check(self.ctx.lib.pba_census_last_stats(self.h, C.byref(st)), "census_last_stats")
        return {n: getattr(st, n) for n, _ in _lib.PbaCensusStats._fields_}

    def lookup(self, keys) -> np.ndarray:
        keys = np.ascontiguousarray(keys, np.uint32)
        out = np.zeros(keys.size, np.uint32)
        self.ctx.check(self.ctx.lib.pba_census_lookup(self.ctx.h, self.h, _ptr(keys), keys.size, _ptr(out)), "census_lookup")
        return out

    def histogram(self, cap: int = 65536):
        """(hist u64[cap], n_distinct, max_count): hist[0] = counters never counted, hist[cap - 1] = keys with count >= cap - 1"""
        hist = np.zeros(max(cap, 0), np.uint64)
        nd, mx = C.c_uint64(), C.c_uint32()
        self.ctx.check(self.ctx.lib.pba_census_histogram(self.ctx.h, self.h, _ptr(hist), cap, C.byref(nd), C.byref(mx)), "census_histogram")
        return hist, int(nd.value), int(mx.value)

    def cutoff(self, fraction: float, floor: int = 1, cap: int = 65536) -> int:
        return census_cutoff(self.histogram(cap)[0], fraction, floor)

    def read_repeats(self, seqs: "SeqSet", max_occ: int):
        """(n_over, n_visited) per sequence of seqs: visited positions whose key occurs more than max_occ times, visited positions"""
        n = seqs.count
        over, vis = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self.ctx.check(self.ctx.lib.pba_census_read_repeats(self.ctx.h, self.h, seqs.h, max_occ, _ptr(over), _ptr(vis), n), "census_read_repeats")
        return over, vis

    def mask_probes(self, d_entries_ptr: int, n_slots: int, max_occ: int, mask: Optional[int] = None) -> int:
        """in place on a device buffer of probe entries: those of keys with count > max_occ become all-ones; returns how many"""
        n = C.c_uint64()
        self.ctx.check(self.ctx.lib.pba_census_mask_probes(self.ctx.h, self.h, C.c_void_p(d_entries_ptr), n_slots,
                                                           self.mask if mask is None else mask, max_occ, C.byref(n)), "census_mask_probes")
        return int(n.value)


def _census(self, seqs, mask, mode="head_tail", lo=0, hi=None) -> "Census":
    return Census(self, seqs, mask, mode, lo, hi)


def _overlap_strands_masked(self, reads, mask, R, census, max_occ, max_trial=32, overlap_min=64, strands=3, t_lo=0, t_hi=None,
                            kernel=PBA_KERNEL_AUTO, cap=None, reads_rc=None):
    """overlap_strands with the probes of keys that occur more than max_occ times (census: a head_tail census of the forward
    reads under `mask`) left out of both probe tables.  Returns (rows, [stats of the +1 pass, of the -1 pass], [probe entries
    masked on +1, on -1])."""
    t_hi = reads.count if t_hi is None else t_hi
    cap = cap if cap is not None else max(1, 2 * (t_hi - t_lo) * max(reads.count - 1, 1))
    out = np.empty(cap, STRAND_OVERLAP_DTYPE)
    n = C.c_uint64()
    st2 = (_lib.PbaOverlapStats * 2)()
    nm = (C.c_uint64 * 2)()
    self.check(self.lib.pba_overlap_strands_masked(self.h, reads.h, reads_rc.h if reads_rc is not None else None, t_lo, t_hi, mask, R,
                                                   max_trial, overlap_min, kernel, strands, census.h if census is not None else None,
                                                   max_occ, _ptr(out), cap, C.byref(n), C.byref(st2), C.byref(nm)),
               "overlap_strands_masked")
    return out[:min(int(n.value), cap)], _stats_pair(st2), [int(nm[0]), int(nm[1])]


Context.census = _census
Context.overlap_strands_masked = _overlap_strands_masked


def script_vals(ops: np.ndarray, seg: bytes, fwd: bool = True) -> bytes:
    """edits[k].val of an edit script (seq_aligner.h:218,224): the b element a MATCH / INSERT consumes, 0 for a DELETE.
    seg: the accessor's elements in memory order (a backward accessor starts at its last byte)."""
    elems = np.frombuffer(seg if fwd else seg[::-1], np.uint8)
    ops = np.asarray(ops, np.uint8)
    takes = ops != 3
    idx = np.cumsum(takes) - 1
    out = np.where(takes, elems[np.minimum(idx, max(elems.size - 1, 0))] if elems.size else 0, 0).astype(np.uint8)
    return out.tobytes()


class SeedIndex:
    def __init__(self, ctx: Context, h):
        self.ctx, self.h = ctx, h

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.lib.pba_index_destroy(self.h)
        self.h = None

    __del__ = close

    @property
    def entries(self) -> int:
        return self.ctx.lib.pba_index_entries(self.h)

    @property
    def visited(self) -> int:
        return self.ctx.lib.pba_index_visited(self.h)

    @property
    def seqs(self) -> int:
        """Sequences the index covers (pba_index_seqs): 1 unless it was made by Context.index_build_set."""
        return self.ctx.lib.pba_index_seqs(self.h)

    def dump(self):
        n = self.entries
        keys = np.zeros(max(n, 1), np.uint32)
        pos = np.zeros(max(n, 1), np.int32)
        got = C.c_uint64()
        self.ctx.check(self.ctx.lib.pba_index_dump(self.ctx.h, self.h, _ptr(keys), _ptr(pos), n, C.byref(got)),
                       "index_dump")
        return keys[:n], pos[:n]

    def find(self, keys: np.ndarray):
        keys = np.ascontiguousarray(keys, np.uint32)
        off = np.zeros(keys.size + 1, np.uint64)
        lib, c = self.ctx.lib, self.ctx
        c.check(lib.pba_index_find(c.h, self.h, _ptr(keys), keys.size, _ptr(off), None, 0), "index_find")
        total = int(off[-1])
        pos = np.zeros(max(total, 1), np.int32)
        c.check(lib.pba_index_find(c.h, self.h, _ptr(keys), keys.size, _ptr(off), _ptr(pos), total), "index_find")
        return off, pos[:total]
