"""csrc/seq_layout.h alone -- the one place where the layout of a sequence set is computed -- as a stand-alone host
program (tests/cpp/seq_layout_main.cpp, under ASan + UBSan where the compiler has the runtimes) against a numpy restatement:
the prefixes and totals of every edge length in every rotation, of every single length up to 4 200, of seeded random
batches and of the batches that round up the most, and the condition that protects a stream's slot -- no batch that fits slot_bytes and slot_reads lays out past what
slot_caps reserved, the batch that fills the slot exactly included.  No GPU, nothing loaded into python."""
import os
import subprocess

import numpy as np
import pytest

from conftest import HERE, ROOT
from seqs_edge_inputs import EDGE_LENGTHS

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"]


def batches():
    out = [EDGE_LENGTHS[r:] + EDGE_LENGTHS[:r] for r in range(len(EDGE_LENGTHS))]
    out += [[L] for L in range(4201)]
    rs = np.random.RandomState(20261)
    out += [rs.randint(0, 3001, rs.randint(0, 65)).tolist() for _ in range(200)]
    # the batches that round up the most per byte given: 1 base past a 16-byte unit of the arena (64 bases) and past a plane word
    # (32), up to 64 reads of them -- random lengths leave half of the 16 bytes per read that pk_cap adds unused
    out += [[L] * n for L in (1, 33, 65) for n in (1, 2, 15, 16, 17, 63, 64)]
    return [np.array(b, np.int64) for b in out]


def slot_bytes_of(lens):
    """the batch's own byte count as ASCII and as a binary read file (a u32 length, then four bases per byte)"""
    return int(lens.sum()), int((4 + (lens + 3) // 4).sum())


def caps_ref(text_form, slot_bytes, slot_reads):
    if text_form:
        pk = ((slot_bytes + 3) // 4 + 16 * slot_reads + 15) & ~15
        return pk, pk, slot_bytes // 32 + slot_reads + 1
    return (slot_bytes + 15) & ~15, (slot_bytes + 16 * slot_reads + 15) & ~15, slot_bytes // 8 + slot_reads + 1


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """every batch through the program, once: a list of {tag: [ints]} per batch, and the constants line"""
    exe = str(tmp_path_factory.mktemp("seq_layout") / "seq_layout_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pacbioassembly_amd", "csrc"),
           os.path.join(HERE, "cpp", "seq_layout_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    bs = batches()
    stdin = "".join("%d %d %d %s\n" % (len(b), *slot_bytes_of(b), " ".join(map(str, b))) for b in bs)
    p = subprocess.run([exe], input=stdin.encode(), capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode(errors="replace")[-4000:]
    lines = [ln.split() for ln in p.stdout.decode().splitlines()]
    assert lines[0][0] == "consts" and len(lines) == 1 + 6 * len(bs)
    per = [{ln[0]: [int(x) for x in ln[1:]] for ln in lines[1 + 6 * k:7 + 6 * k]} for k in range(len(bs))]
    return bs, per, [int(x) for x in lines[0][1:]]


def test_constants_and_arena_kinds(answers):
    # kMaxSeqLen, kSlack, kPlaneSlack, kRecordSlack, PBA_PP_BASES; 65 bases: 17 payload bytes -> 32, 3 plane words; the three arenas
    assert answers[2] == [65000, 1024, 64, 65536, 2048, 32, 3, 1024 + 100 + 1024, 1024 + 100 + 65536, 1024 + 100 + 1024]


def test_prefixes_and_totals_equal_the_restatement(answers):
    bs, per, _ = answers
    assert len(bs) == 18 + 4201 + 200 + 21 and any(len(b) == 0 for b in bs) and any(len(b) == 64 for b in bs)
    for lens, got in zip(bs, per):
        pk, w, it = ((lens + 3) // 4 + 15) & ~15, (lens + 31) // 32, (lens + 2047) // 2048
        for tag, each in (("off", pk), ("poff", w), ("item", it)):
            assert got[tag] == np.concatenate([[0], np.cumsum(each)]).tolist(), (tag, lens)
        totals = [int(pk.sum()), int(w.sum()), int(it.sum()), int(lens.max()) if len(lens) else 0]
        assert got["totals"] == totals + totals, lens
    one = {int(b[0]): g for b, g in zip(bs[18:18 + 4201], per[18:]) if len(b) == 1}      # the single lengths: every residue of 4, 16, 32, 64, 2 048
    assert sorted(one) == list(range(4201)) and one[0]["totals"][:3] == [0, 0, 0]
    assert [one[L]["totals"][:3] for L in (1, 64, 65, 2048, 2049)] == [[16, 1, 1], [16, 2, 1], [32, 3, 1], [512, 64, 1], [528, 65, 2]]


def test_no_batch_that_fits_the_slot_lays_out_past_its_capacities(answers):
    bs, per, _ = answers
    for lens, got in zip(bs, per):
        n, (sb_text, sb_rec) = len(lens), slot_bytes_of(lens)
        pk_total, words = got["totals"][0], got["totals"][1]
        for tag, text_form, sb in (("caps_text", True, sb_text), ("caps_records", False, sb_rec)):
            pk_cap, rc_cap, plane_cap = got[tag][:3]
            assert (pk_cap, rc_cap, plane_cap) == caps_ref(text_form, sb, n), (tag, lens)
            assert got[tag][3:] == [pk_cap, 0, plane_cap]                    # a slot without rc reserves no rc arena
            # the forward arena of the records form is the file itself; its rc arena, and both of the text form, the text layout
            assert (pk_total if text_form else sb) <= pk_cap and pk_total <= rc_cap and words <= plane_cap, (tag, lens)
            assert pk_cap % 16 == 0 and rc_cap % 16 == 0
