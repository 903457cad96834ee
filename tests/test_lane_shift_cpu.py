"""csrc/lane_shift.h alone -- which lane holds which superblock in the shifted form of the score-only sweep, and what the
lanes hand to each other -- as a stand-alone host program (tests/cpp/lane_shift_main.cpp, under ASan + UBSan where the
compiler has the runtimes).  The program plays the ring of lanes with its `live` mask, exactly as bitvec_pass derives it,
and the shifted form side by side over the same schedule, and for every step and every superblock whose window is open
both must take the same thing: the hout of superblock s - 1 from the step before where that superblock's window reaches
the column, else the border.  Lane, superblock and column stay bijections across every close, every table and ring address
stays inside its region, the 64 lanes hit 64 banks, and no column receives fin words while a lane still reads its rows.
Rings 1 and 2 over the geometries of the table model (test_eq_table_cpu.py) and sweeps of 1, 2, 63, 64, 65, 128 and 129
superblocks.  No GPU."""
import os
import subprocess

import pytest

import align_rings as ar
from conftest import HERE, ROOT
from test_eq_table_cpu import TABLE_RINGS, table_sweeps
from test_text_ring_cpu import SAN, model_reads

CSRC = os.path.join(ROOT, "pacbioassembly_amd", "csrc")
SB_COUNTS = (1, 2, 63, 64, 65, 128, 129)


def sb_sweeps():
    """(m, nr, wleft, w, NB) with exactly S superblocks of rows, S in SB_COUNTS: the narrow window and the reference band of
    a pair whose longer side ends a few rows into its last superblock, at two divergences; and, per ring, the widest window
    the ring holds (wleft + w == bv_max_span), where superblock s + 64 opens at the very step superblock s closes"""
    out = []
    for NB in TABLE_RINGS:
        RB = 32 * NB
        for S in SB_COUNTS:
            for R in (0.05, 0.30):
                nr = (S - 1) * RB + 5 if S > 1 else 12
                for m in sorted({max(11, nr - 3), max(11, nr - RB - 2), max(11, nr - 3 * RB)}):
                    md = ar.max_dst_of(m, m + 1, R)
                    for w, wl in ((ar.bv_pass1_w(md, NB), ar.bv_pass1_wl(md, NB)), (md, ar.bv_full_wl(md))):
                        if wl + w > ar.bv_max_span(NB) or nr > m + w or nr < m:
                            continue
                        out.append((m, nr, w, wl, NB))
        span = ar.bv_max_span(NB)
        wl = span // 3
        out.append((129 * RB, 129 * RB + 40, span - wl, wl, NB))
    return sorted(set(out))


def all_sweeps():
    return sorted(set(table_sweeps()) | set(sb_sweeps()))


def t_open(s, m, wleft, RB):
    return max(1, s * RB + 1 - wleft) + s


def t_close(s, m, w, RB):
    return min(m, s * RB + RB + w) + s + 1


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lane_shift") / "lane_shift_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(HERE, "cpp", "lane_shift_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    sw = all_sweeps()
    p = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % s for s in sw).encode(), capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stderr.decode(errors="replace")[-4000:])
    rows = [tuple(int(v) for v in ln.split()) for ln in p.stdout.decode().splitlines()]
    assert len(rows) == len(sw)
    return sw, rows


def test_grid_has_every_superblock_count_and_the_edges_of_the_schedule():
    sw = all_sweeps()
    for NB in TABLE_RINGS:
        RB = 32 * NB
        mine = [s for s in sw if s[4] == NB]
        assert {(s[1] + RB - 1) // RB for s in mine} >= set(SB_COUNTS)
        # open(s + 64) == close(s): the last lane's next superblock opens in the step behind the close that handed it over
        assert any(t_open(s + 64, m, wleft, RB) == t_close(s, m, w, RB)
                   for (m, nr, wleft, w, _) in mine for s in range(max(0, (nr + RB - 1) // RB - 64)))
        # one close per step at the end of a sweep: the windows that end with the last column
        def run_of_closes(m, nr, wleft, w, _):
            S = (nr + RB - 1) // RB
            cl = [t_close(s, m, w, RB) for s in range(S) if t_close(s, m, w, RB) <= m + S - 1]
            return sum(1 for a, b in zip(cl, cl[1:]) if b == a + 1)
        assert max(run_of_closes(*s) for s in mine) >= 3
        assert any(s[1] == s[0] for s in mine) and any(s[1] > 64 * RB for s in mine) and any(s[1] > 128 * RB for s in mine)


def test_both_hand_offs_take_the_cell_above_or_the_border(played):
    """the program's exit codes 3 and 4, and its count of checked hand-offs: one per open superblock and step"""
    sw, rows = played
    for s, (t_end, checked, closes, fins) in zip(sw, rows):
        assert (t_end, checked) == model_reads(*s), s


def test_closes_and_fin_words(played):
    """every superblock whose window ends before the sweep does closes once, with the lanes moving up; every superblock from
    row m's down puts its column aside exactly once, into column s & 63 (exit codes 6, 7 and 8)"""
    sw, rows = played
    for (m, nr, wleft, w, NB), (t_end, checked, closes, fins) in zip(sw, rows):
        RB = 32 * NB
        S, s_m = (nr + RB - 1) // RB, (m - 1) // RB
        assert closes == sum(1 for s in range(S) if t_close(s, m, w, RB) <= t_end), (m, nr, wleft, w, NB)
        assert fins == S - s_m and S - s_m < 64, (m, nr, wleft, w, NB)


def test_the_border_one_step_early_is_caught(tmp_path):
    """the model has teeth: a close that moves the carries down with the lanes (and so hands lane 0 the border already in
    the step behind the close, one column before the window above has ended) is exit code 4"""
    src = open(os.path.join(HERE, "cpp", "lane_shift_main.cpp")).read()
    a, b = "lsh_hin_plus_closed(hpmS)", "lsh_hin_minus_closed(hnmS)"
    assert src.count(a) == 1 and src.count(b) == 1
    bad = tmp_path / "early_border.cpp"
    bad.write_text(src.replace(a, "lsh_hin_plus(hpmS >> 1)").replace(b, "lsh_hin_minus(hnmS >> 1)"))
    exe = str(tmp_path / "early_border")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", CSRC, str(bad), "-o", exe], check=True)
    p = subprocess.run([exe], input=b"15000 15900 2700 1351 2\n", capture_output=True, timeout=60)
    assert p.returncode == 4, p.returncode


def test_header_is_plain_cpp_and_the_kernel_uses_it():
    hdr = open(os.path.join(CSRC, "lane_shift.h")).read()
    assert "hip" not in hdr.lower().replace("without hip", "") and "#define PBA_LSH_LANES 64" in hdr
    src = open(os.path.join(CSRC, "align_bitvec.h")).read()
    for fn in ("lsh_col(", "lsh_sb(", "lsh_lane(", "lsh_ring_addr("):
        assert fn in src, fn
    assert "constexpr bool SHIFT = EQT && PBA_BV_SHIFT;" in src
