"""csrc/text_ring.h alone -- the arithmetic of the bit-vector sweep's text ring -- as a stand-alone host program
(tests/cpp/text_ring_main.cpp, under ASan + UBSan where the compiler has the runtimes) against a step-by-step model of the
sweep that knows nothing of the ring: at every step every lane with an open window finds exactly element t - 1 - s at its
address, no write replaces an element an open window still has to read, no address leaves the ring, and the superblock the
kernel derives for a lane is the one the lane holds.  The grid is every (m, rows, window, NB) the inputs of
test_gpu_text_ring.py run at, in the narrow first window and at the reference band.  No GPU."""
import os
import subprocess

import pytest

import align_rings as ar
from conftest import HERE, ROOT

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"]
RS = (0.05, 0.15, 0.30, 0.45)
COLS, CHUNK = 128, 32


def ring_ms(NB):
    RB = 32 * NB
    return sorted({11, 31, 32, 33, 63, 64, 65, COLS - 1, COLS, COLS + 1, 2 * COLS + 1, RB - 1, RB, RB + 1, 2 * RB + 1,
                   64 * RB - 24, 64 * RB + 1, 2100, 4200, 15000})


def sweeps():
    """(m, nr, wleft, w, NB) as bitvec_pass takes them: the narrow window and the reference band of every pair shape, in
    every ring that holds the window"""
    out = []
    for NB in ar.RINGS:
        for R in RS:
            for m in ring_ms(NB):
                md = ar.max_dst_of(m, m + 1, R)
                for w, wl in ((ar.bv_pass1_w(md, NB), ar.bv_pass1_wl(md, NB)), (md, ar.bv_full_wl(md))):
                    if wl + w > ar.bv_max_span(NB):
                        continue
                    for n in sorted({m, m + 1, m + md - 1, m + md}):
                        out.append((m, min(n, m + w), w, wl, NB))
    return sorted(set(out))


def model_reads(m, nr, wleft, w, NB):
    RB = 32 * NB
    S = (nr + RB - 1) // RB
    return m + S - 1, sum(max(0, min(m, s * RB + RB + w) - max(1, s * RB + 1 - wleft) + 1) for s in range(S))


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("text_ring") / "text_ring_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pacbioassembly_amd", "csrc"),
           os.path.join(HERE, "cpp", "text_ring_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    sw = sweeps()
    p = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % s for s in sw).encode(), capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stderr == b"", (p.returncode, p.stderr.decode(errors="replace")[-4000:])
    rows = [tuple(int(v) for v in ln.split()) for ln in p.stdout.decode().splitlines()]
    assert len(rows) == len(sw)
    return sw, rows


def test_grid_covers_the_gpu_shapes():
    sw = sweeps()
    assert {s[4] for s in sw} == set(ar.RINGS)
    for m in (31, 32, 33, 63, 64, 65, COLS - 1, COLS, COLS + 1, 2 * COLS + 1):
        assert any(s[0] == m and s[4] == 1 for s in sw) and any(s[0] == m and s[4] == 2 for s in sw)
    assert any(s[4] == 1 and s[1] > 2048 for s in sw) and any(s[4] == 2 and s[1] > 4096 for s in sw)     # a lane's second superblock
    assert any(s[2] + s[3] == ar.bv_max_span(s[4]) or s[2] + s[3] > ar.bv_max_span(s[4]) - 40 for s in sw)  # a full ring


def test_every_open_lane_reads_its_column(played):
    sw, rows = played
    for s, (t_end, reads, span) in zip(sw, rows):
        assert (t_end, reads) == model_reads(*s), s


def test_live_window_fits_the_ring(played):
    """the program's own measure of it: oldest element still to be read .. frontier, at every write.  64 lanes, one closing
    step and the 32 elements of the chunk: 97 at the most, under the 128 the ring holds"""
    sw, rows = played
    spans = [r[2] for r in rows]
    assert max(spans) <= 64 + 1 + CHUNK < COLS and max(spans) >= 64 + CHUNK - 1, max(spans)


def test_header_constants():
    src = open(os.path.join(ROOT, "pacbioassembly_amd", "csrc", "text_ring.h")).read()
    assert "#define PBA_TXR_COLS %d " % COLS in src and "#define PBA_TXR_CHUNK %d " % CHUNK in src
