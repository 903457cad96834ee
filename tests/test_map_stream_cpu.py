"""Streamed mapping (pba_map_stream), the part that needs no GPU: the C ABI is declared, exported and bound, every entry point
refuses a NULL stream, examples/map_stream_gpu.cpp is plain C++ over include/pba.h that refuses to run without a device, and
the world tests/test_gpu_map_stream.py maps holds what it is for -- judged from tests/map_ref.py alone."""
import ctypes
import os
import subprocess

import numpy as np

from conftest import MASK_PAT, ROOT
from map_ref import map_reads_ref
from map_stream_inputs import BATCH_SIZES, CONTIG_LENS, MIN_LEN, N_READS, R, TRIALS, batches_of, composition, rows_tsv, world

MAP_STREAM_SYMBOLS = ["pba_map_stream_create", "pba_map_stream_buffer", "pba_map_stream_submit", "pba_map_stream_collect",
                      "pba_map_stream_pending", "pba_map_stream_last_profile", "pba_map_stream_destroy"]


def test_map_stream_symbols_declared_exported_and_bound(lib):
    from pacbioassembly_amd import MapStream, _lib
    from pacbioassembly_amd.engine import Context, LocStream
    from test_abi_symbols import declared_functions
    names = declared_functions()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in MAP_STREAM_SYMBOLS:
        assert n in names, n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    assert "typedef struct pba_map_stream pba_map_stream;" in open(os.path.join(ROOT, "include", "pba.h")).read()
    for m in ("submit_reads", "buffer", "submit", "collect", "pending", "profile", "close"):
        assert callable(getattr(MapStream, m)), m
    assert MapStream.collect is not LocStream.collect and MapStream.pending is not LocStream.pending
    assert callable(Context.map_stream)


def test_null_map_stream_is_refused_without_touching_a_device(lib):
    assert lib.pba_map_stream_buffer(None, None, None) == -1
    assert lib.pba_map_stream_submit(None, 0) == -1
    assert lib.pba_map_stream_collect(None, None, 0, None, None) == -1
    assert lib.pba_map_stream_pending(None, None, None) == -1
    assert lib.pba_map_stream_last_profile(None, None) == -1
    assert lib.pba_map_stream_create(None, None, None, 0.3, 50, 500, 0, 0, 0, 3, 1024, 4, 0, None) == -1
    lib.pba_map_stream_destroy(None)


def test_map_stream_example_builds_against_the_c_abi_and_refuses_to_run_without_a_gpu(lib, tmp_path):
    import torch
    libdir = os.path.join(ROOT, "pacbioassembly_amd", "lib")
    exe = str(tmp_path / "map_stream_gpu")
    subprocess.run(["g++", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "examples", "map_stream_gpu.cpp"), "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}"], check=True)
    if torch.cuda.is_available():
        return
    (tmp_path / "c.txt").write_text("ACGT" * 100 + "\n\n" + "ACGT" * 50 + "\n")
    r = subprocess.run([exe, str(tmp_path / "c.txt"), MASK_PAT, "0.30", "64"], input=b"ACGT\n", capture_output=True)
    assert r.returncode != 0 and r.stdout == b"" and b"device" in r.stderr.lower()


def test_gpu_world_holds_what_it_is_for(lib, oracle):
    """With the committed seed the restatement finds at least 30 reads on +, 30 on -, leaves at least 10 of full length
    unfound and at least 5 below min_len, finds a read on each non-trivial contig and walks some reads a second time: the
    conditions the GPU test asserts on the engine's rows are conditions the reference itself meets."""
    from pacbioassembly_amd import engine as eng
    contigs, reads, flipped = world()
    assert [len(c) for c in contigs] == CONTIG_LENS == [5000, 3000, 12, 0] and len(reads) == N_READS == 150
    assert sum(BATCH_SIZES) == N_READS and [len(b) for b in batches_of(reads)] == BATCH_SIZES
    lens = np.array([len(x) for x in reads])
    full = lens >= MIN_LEN
    assert lens[full].max() <= 1400 and 100 <= lens[~full].min() and lens[~full].max() <= 400 and (~full).sum() == 10
    assert 50 < int(flipped.sum()) < 100
    rows, stats, _ = map_reads_ref(oracle, contigs, reads, eng.mask_from_pattern(MASK_PAT), R, TRIALS, MIN_LEN, strands=3)
    n_second_walk = stats[1]["n_reads_kept"]
    verdict = composition(rows, n_second_walk, reads)
    print(verdict, stats)
    assert all(verdict.values()), verdict
    assert n_second_walk == int(((rows["found"] == 0) | (rows["strand"] == -1))[full].sum())
    tsv = rows_tsv(np.zeros(2, eng.MAP_ROW_DTYPE))
    assert tsv == (b"\t".join([b"0"] * 17) + b"\n") * 2
