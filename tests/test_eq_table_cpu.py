"""csrc/eq_table.h alone -- where the score-only sweep's match-mask table, its ring of row offsets and the fin words live in
a wavefront's LDS -- as a stand-alone host program (tests/cpp/eq_table_main.cpp, under ASan + UBSan where the compiler has
the runtimes) against a step-by-step model of the sweep that knows nothing of the layout: at every step every lane with an
open window reads, for every block, the row its own superblock's planes gave for exactly the letter of column t - s; no
address, of an open lane or a closed one, leaves the table; no fin word lands on a row that a lane with an open window
still reads, and the fin superblock word survives the sweep.  Rings 1 and 2, the narrow first window and the reference
band, over the sweep geometries of the text-ring model (test_text_ring_cpu.py).  No GPU."""
import os
import subprocess

import pytest

import align_rings as ar
from conftest import HERE, ROOT
from test_text_ring_cpu import SAN, model_reads, sweeps

CSRC = os.path.join(ROOT, "pacbioassembly_amd", "csrc")
TABLE_RINGS = (1, 2)


def table_sweeps():
    return [s for s in sweeps() if s[4] in TABLE_RINGS]


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("eq_table") / "eq_table_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "cpp", "eq_table_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    sw = table_sweeps()
    p = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % s for s in sw).encode(), capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stderr.decode(errors="replace")[-4000:])
    rows = [tuple(int(v) for v in ln.split()) for ln in p.stdout.decode().splitlines()]
    assert len(rows) == len(sw)
    return sw, rows


def test_grid_covers_both_rings_and_a_second_superblock():
    sw = table_sweeps()
    assert {s[4] for s in sw} == set(TABLE_RINGS) <= set(ar.RINGS)
    for NB in TABLE_RINGS:
        RB = 32 * NB
        assert any(s[4] == NB and s[1] > 64 * RB for s in sw)                          # a lane fills its rows a second time
        assert any(s[4] == NB and s[1] > s[0] and (s[0] - 1) // RB < (s[1] - 1) // RB for s in sw)   # fin words from more than one lane
        assert any(s[4] == NB and s[1] == s[0] for s in sw)                            # and from the last superblock alone
        assert any(s[4] == NB and s[2] + s[3] > ar.bv_max_span(NB) - 40 for s in sw)   # a full ring


def test_every_open_lane_reads_its_own_rows_for_its_column(played):
    sw, rows = played
    for s, (t_end, reads, fills, fins) in zip(sw, rows):
        assert (t_end, reads) == model_reads(*s), s


def test_rows_are_filled_once_per_superblock_and_fin_once_per_goal_superblock(played):
    """a lane fills its rows when it takes a superblock and at no other time; every superblock from row m's down puts its
    words aside exactly once, on its own lane's rows, after that lane's last read (the program's exit codes 7 and 8)"""
    sw, rows = played
    for (m, nr, wleft, w, NB), (t_end, reads, fills, fins) in zip(sw, rows):
        RB = 32 * NB
        S, s_m = (nr + RB - 1) // RB, (m - 1) // RB
        closes = sum(1 for s in range(S) if min(m, s * RB + RB + w) + s + 1 <= t_end and s + 64 < S)
        assert fills == min(S, 64) + closes and fins == S - s_m and S - s_m < 64, (m, nr, wleft, w, NB)


def test_layout_fits_the_locate_kernel_at_full_occupancy():
    """the header's own figures: ring 2 takes 2 944 bytes per wavefront, which with the locate walk's 1 792 stays under the
    5 120 a wavefront may have when 32 of them share a CU's 160 KB"""
    src = open(os.path.join(CSRC, "eq_table.h")).read()
    assert "#define PBA_EQT_LETTERS 4" in src and "#define PBA_EQT_LANES 64" in src
    words = {NB: 4 * NB * 64 + (128 + 32) + 64 for NB in TABLE_RINGS}
    assert words[2] * 4 == 2944 and words[1] * 4 == 1920
    assert words[2] * 4 + 1792 <= 160 * 1024 // 32
