"""Streamed locate (pba_loc_stream), the part that needs no GPU: the C ABI is declared, exported and bound, and
examples/locator_stream_gpu.cpp is plain C++ over include/pba.h that refuses to run without a device."""
import ctypes
import os
import subprocess

from conftest import ROOT

STREAM_SYMBOLS = ["pba_loc_stream_create", "pba_loc_stream_buffer", "pba_loc_stream_submit", "pba_loc_stream_collect",
                  "pba_loc_stream_pending", "pba_loc_stream_last_profile", "pba_loc_stream_destroy"]


def test_stream_symbols_declared_exported_and_bound(lib):
    from pacbioassembly_amd import _lib
    from test_abi_symbols import declared_functions
    names = declared_functions()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in STREAM_SYMBOLS:
        assert n in names, n
        assert hasattr(raw, n), n
        assert n in _lib.SYMBOLS, n
    hdr = open(os.path.join(ROOT, "include", "pba.h")).read()
    assert "PBA_STREAM_TEXT = 0" in hdr and "PBA_STREAM_RECORDS = 1" in hdr and "pba_stream_profile" in hdr
    assert (_lib.PBA_STREAM_TEXT, _lib.PBA_STREAM_RECORDS) == (0, 1)
    # the profile struct as the header lays it out: four floats, a u32, padding to 8, a u64
    assert ctypes.sizeof(_lib.PbaStreamProfile) == 32 and _lib.PbaStreamProfile.n_bytes.offset == 24


def test_null_stream_is_refused_without_touching_a_device(lib):
    assert lib.pba_loc_stream_submit(None, 0) == -1
    assert lib.pba_loc_stream_collect(None, None, 0, None, None) == -1
    assert lib.pba_loc_stream_pending(None, None) == -1
    assert lib.pba_loc_stream_last_profile(None, None) == -1
    assert lib.pba_loc_stream_create(None, None, None, 0, 0.3, 50, 500, 0, 0, 0, 1024, 4, 0, None) == -1
    lib.pba_loc_stream_destroy(None)


def test_stream_example_builds_against_the_c_abi_and_refuses_to_run_without_a_gpu(lib, tmp_path):
    import torch
    libdir = os.path.join(ROOT, "pacbioassembly_amd", "lib")
    exe = str(tmp_path / "locator_stream_gpu")
    subprocess.run(["g++", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                    os.path.join(ROOT, "examples", "locator_stream_gpu.cpp"), "-L", libdir, "-lpba", f"-Wl,-rpath,{libdir}"], check=True)
    if torch.cuda.is_available():
        return
    (tmp_path / "c.txt").write_text("ACGT" * 100 + "\n")
    r = subprocess.run([exe, str(tmp_path / "c.txt"), "111*11*11*1*1111", "0.15", "64"], input=b"ACGT\n", capture_output=True)
    assert r.returncode != 0 and r.stdout == b"" and b"device" in r.stderr.lower()
