"""csrc/aln_rows.h alone -- the walker over an edit script that pba_cigar_from_script and pba_windows_from_script are written
on, and the row layout shared by the row-level CIGAR and window entry points -- as a stand-alone host program
(tests/cpp/aln_rows_main.cpp, under ASan + UBSan where the compiler has the runtimes).  The program checks itself against
hand-written scripts (the empty one, a leading INSERT, gap-only scripts, a byte that is no op, every flag combination) and
hand-written rows (a cap that cuts at the first row, at a middle row, at the last row and at none) on exact-size heap arrays.
No GPU."""
import os
import subprocess

from conftest import HERE, ROOT

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"]


def test_walker_and_layout(tmp_path):
    exe = str(tmp_path / "aln_rows_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pacbioassembly_amd", "csrc"),
           "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "aln_rows_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    p = subprocess.run([exe], capture_output=True, timeout=60)
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stderr.decode(errors="replace")[-4000:])
    assert p.stdout.decode().startswith("ok ") and int(p.stdout.split()[1]) >= 40
