"""tests/map_ref.py -- the plain restatement tests/test_gpu_map.py holds pba_map_reads to -- pinned without a GPU: to
Oracle.locator on one contig, to the interval arithmetic include/pba.h states for pba_map_row, and the new entry points
exported by libpba.so."""
import ctypes as C

import numpy as np

from conftest import MASK_PAT
from map_ref import intervals, map_reads_ref, rc, rand_text
from pacbioassembly_amd import engine as eng

R = 0.30


def test_restatement_equals_oracle_locator_on_one_contig(oracle):
    """300 reads of 300 - 700 bases of a 20 kb genome (15 % error; some below min_len, 20 unrelated): rows, n_pairs and
    the stats of the restatement on a one-contig target are Oracle.locator's."""
    mask = oracle.mask_from_pattern(MASK_PAT)
    g = eng.synth_genome(701, 20000)
    text, offs, _ = eng.synth_reads(702, g, 280, 700)
    rng = np.random.default_rng(703)
    reads = [text[int(offs[i]):int(offs[i + 1])].tobytes()[:int(rng.integers(300, 701))] for i in range(280)]
    reads += [rand_text(rng, 650) for _ in range(20)]
    rtext, roffs = eng.concat(reads)
    want, wst = oracle.locator(g, mask, R, rtext, roffs, 50, 500, nthreads=4)
    got, gst, _ = map_reads_ref(oracle, [g.tobytes()], reads, mask, R, 50, 500, strands=1)
    assert 100 < wst["n_located"] < wst["n_reads_kept"] < len(reads) and wst["n_pairs"] > wst["n_located"]
    for c in ("read", "nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs"):
        assert (got[c] == want[c]).all(), c
    assert (got["contig"] == np.where(want["found"] == 1, 0, -1)).all() and (got["strand"] == want["found"]).all()
    assert gst[0] == wst and gst[1] == dict.fromkeys(wst, 0)
    # ... and strands == 2 is the same walk over the reverse complements
    got2, gst2, _ = map_reads_ref(oracle, [g.tobytes()], [rc(x) for x in reads[:60]], mask, R, 50, 500, strands=2)
    for c in ("found", "j", "pos", "cost", "matlen_a", "matlen_b", "n_pairs"):
        assert (got2[c] == want[c][:60]).all(), c
    assert (got2["strand"] == -want["found"][:60]).all() and gst2[0]["n_pairs"] == 0


def test_intervals_of_all_four_cases():
    """(strand, found): walked read [j, j + matlen_a), contig [pos, pos + matlen_b); strand -1 gives the read interval on the
    read's forward strand, [len - j - matlen_a, len - j); nothing found: zeros."""
    assert intervals(1, 1, 3, 100, 40, 42, 50) == (3, 43, 100, 142)
    assert intervals(-1, 1, 3, 100, 40, 42, 50) == (7, 47, 100, 142)
    assert intervals(0, 0, -1, -1, 0, 0, 50) == (0, 0, 0, 0)
    assert intervals(-1, 0, -1, -1, 0, 0, 50) == (0, 0, 0, 0)
    # a - interval is the + interval of the same bases seen from the other end: rc(read)[j : j + ma] == rc(read[b : e])
    x = b"ACGTTGCAAGGCTTAACCGGATCGATTACA"
    b, e, _, _ = intervals(-1, 1, 4, 0, 9, 9, len(x))
    assert rc(x)[4:13] == rc(x[b:e])


def test_new_entry_points_are_exported_and_refuse_a_null_ctx(lib):
    """pba_index_build_set, pba_index_seqs and pba_map_reads are in the library and in the ctypes table; without a ctx the two
    that take one answer PBA_E_INVALID before anything else is looked at."""
    from pacbioassembly_amd import _lib
    for name in ("pba_index_build_set", "pba_index_seqs", "pba_map_reads"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    out = C.c_void_p()
    assert lib.pba_index_build_set(None, None, 0xFFFFFFFF, C.byref(out)) == _lib.PBA_E_INVALID and not out.value
    assert lib.pba_map_reads(None, None, None, None, None, 0.3, 50, 500, 0, 0, 0, 3, None, None) == _lib.PBA_E_INVALID
    assert lib.pba_index_seqs(None) == 0
    assert C.sizeof(_lib.PbaMapRow) == 17 * 4 == eng.MAP_ROW_DTYPE.itemsize
