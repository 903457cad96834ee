"""The reads that sit on every edge of a sequence set's layout, and the host-side restatements they are held against: shared by
tests/test_gpu_map_stream.py (a stream's slots), tests/test_gpu_seqs_edges.py (the resident makers) and
tests/test_seq_layout_cpu.py (csrc/seq_layout.h alone).  host_packed keeps its own arithmetic on purpose: it is the
restatement that does not go through seq_layout.h."""
import numpy as np

from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PAIR_DTYPE

# every residue class of the layout (64 bases per 16 packed bytes, 32 per plane word and per thread, 16 per dword, 4 per byte,
# 2 048 per work item) and the empty read; rotated so that reads shorter than 32 bases come first and last in a batch
EDGE_LENGTHS = [0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4097]
ROTATIONS = [(0, "the empty read first"), (1, "a 1-base read first, the empty read last"), (4, "5 first, 4 last"),
             (10, "33 first, 32 last"), (14, "2 047 first, 65 last"), (17, "4 097 first, 2 049 last"), (8, "31 first, 17 last")]


def host_packed(texts, offs):
    """The arena of pba_seqs_from_text's layout through the host codec alone: pba_text2bin's payload of every text at its
    16-byte aligned offset, zeros between."""
    total = int(offs[-1]) + (((len(texts[-1]) + 3) // 4 + 15) & ~15) if texts else 0
    out = np.zeros(total, np.uint8)
    for t, o in zip(texts, offs):
        rec = eng.text2bin(t)
        assert int.from_bytes(rec[:4], "little") == len(t) and len(rec) == 4 + (len(t) + 3) // 4
        out[int(o):int(o) + len(rec) - 4] = np.frombuffer(rec[4:], np.uint8)
    return out


def np_revcomp(t: bytes) -> bytes:
    a = np.frombuffer(t, np.uint8)[::-1]
    lut = np.zeros(256, np.uint8)
    lut[list(b"ACGT")] = list(b"TGCA")
    return lut[a].tobytes()


def self_pairs(texts):
    """every read that has a base against itself (the empty read has no alignment to cost anything)"""
    return np.array([(i, 0, len(t), i, 0, len(t), 0) for i, t in enumerate(texts) if len(t) > 0], PAIR_DTYPE)
