"""csrc/locate_walk.h alone -- the slot arithmetic of k_locate's lane-parallel candidate walk -- as a stand-alone host program
(tests/cpp/locate_walk_main.cpp, under ASan + UBSan where the compiler has the runtimes) against a brute-force enumeration: the
exclusive offsets of 64 hit counts, the (probe, hit) of a list slot, the hit probes up to a probe; counts of 0, 1, 63, 64, 65,
one probe with 2^32 - 1 hits, lists longer than 2^32.  And the proof, from the genome texts and the oracle, of what every
input of test_gpu_locate_walk.py is (locate_walk_inputs.py).  No GPU, nothing loaded into python but the oracle."""
import os
import subprocess

import numpy as np
import pytest

import locate_walk_inputs as lw
import map_ref
from conftest import HERE, ROOT

SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-fno-omit-frame-pointer", "-g"]
BIG = 2 ** 32 - 1
ENUMERATE_UP_TO = 20000


def blocks():
    out = [[0] * 64, [1] * 64, [BIG] * 64, [64] * 64]
    for p in (0, 1, 31, 32, 62, 63):
        for c in (1, 63, 64, 65, BIG):
            out.append([c if q == p else 0 for q in range(64)])
    edge = [0, 1, 63, 64, 65]
    out += [[edge[(q + r) % 5] for q in range(64)] for r in range(5)]
    out += [[edge[(q * 7 + r) % 5] if q % 3 else 0 for q in range(64)] for r in range(5)]
    out.append([BIG if q in (5, 40) else (q % 4) for q in range(64)])         # lists longer than 2^32 with short runs between
    out.append([BIG if q % 2 else 0 for q in range(64)])
    rs = np.random.RandomState(20262)
    out += [(rs.randint(0, 130, 64) * (rs.rand(64) < 0.4)).tolist() for _ in range(60)]
    out += [rs.randint(0, 2 ** 32, 64, dtype=np.uint64).tolist() for _ in range(10)]
    return [[int(c) for c in b] for b in out]


def brute(cnt):
    """offsets (65 of them) by a running sum, and the slots to ask about with their (probe, hit): every slot of a list that
    can be written down, else the first, middle and last slot of every run"""
    off = [0]
    for c in cnt:
        off.append(off[-1] + c)
    if off[-1] <= ENUMERATE_UP_TO:
        ans = [(p, h) for p in range(64) for h in range(cnt[p])]
        return off, list(range(off[-1])), ans
    qs, ans = [], []
    for p in range(64):
        for h in sorted({0, 1, cnt[p] // 2, cnt[p] - 2, cnt[p] - 1}):
            if 0 <= h < cnt[p]:
                qs.append(off[p] + h)
                ans.append((p, h))
    return off, qs, ans


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("locate_walk") / "locate_walk_main")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pacbioassembly_amd", "csrc"),
           os.path.join(HERE, "cpp", "locate_walk_main.cpp"), "-o", exe]
    if subprocess.run(cmd + SAN, capture_output=True).returncode != 0:       # a compiler without the sanitizer runtimes
        subprocess.run(cmd, check=True)
    bs = blocks()
    want = [brute(b) for b in bs]
    stdin = "".join("%s %d %s\n" % (" ".join(map(str, b)), len(w[1]), " ".join(map(str, w[1]))) for b, w in zip(bs, want))
    p = subprocess.run([exe], input=stdin.encode(), capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stderr == b"", p.stderr.decode(errors="replace")[-4000:]
    lines = [ln.split() for ln in p.stdout.decode().splitlines()]
    assert len(lines) == 4 * len(bs) and all(ln[0] == t for k, ln in enumerate(lines) for t in [("off", "off1", "slots", "upto")[k % 4]])
    return bs, want, [lines[4 * k:4 * k + 4] for k in range(len(bs))]


def test_blocks_cover_the_edges():
    bs = blocks()
    assert any(sum(b) == 0 for b in bs) and any(sum(b) > 2 ** 32 for b in bs) and any(sum(b) == 64 * BIG for b in bs)
    assert any(b.count(BIG) == 1 and sum(b) == BIG for b in bs)
    for c in (1, 63, 64, 65):
        assert any(sum(b) == c and c in b for b in bs)


def test_offsets_equal_the_running_sum(answers):
    for cnt, (off, _, _), got in zip(*answers):
        assert [int(v) for v in got[0][1:]] == off, cnt                       # lw_offsets: 64 offsets and the length
        assert [int(v) for v in got[1][1:]] == off, cnt                       # lw_offset(l), l = 0 .. 64


def test_slots_resolve_to_their_probe_and_hit(answers):
    n_enumerated = 0
    for cnt, (off, qs, ans), got in zip(*answers):
        res = [tuple(int(v) for v in t.split(":")) for t in got[2][1:]]
        assert res == ans, cnt
        assert all(cnt[p] > 0 for p, _ in res)                                # never a probe without hits
        n_enumerated += off[-1] <= ENUMERATE_UP_TO and off[-1] > 64
    assert n_enumerated >= 40


def test_hit_probes_up_to_a_probe(answers):
    for cnt, _, got in zip(*answers):
        assert [int(v) for v in got[3][1:]] == [sum(c > 0 for c in cnt[:p + 1]) for p in range(64)], cnt


# ----------------------------------------------------------------------------- what the GPU inputs are
def test_every_case_is_what_it_claims(oracle):
    cs = lw.cases()
    assert len({c["name"] for c in cs}) == len(cs)
    for c in cs:
        f = lw.facts(oracle, c)
        for k, v in c["claims"].items():
            assert f[k] == v, (c["name"], k, v, f)
        assert f["other_fails"] == 0, (c["name"], f)                          # every hit in front of a success fails in rows 11 .. 64
        if c["group"] in ("run", "rowsweep") and "surv" not in c["name"]:
            assert f["array_fails"] == 0 and f["pre_fails"] == f["success"][1], (c["name"], f)     # ... in the prefilter's rows
        w, st = lw.expected(oracle, c)
        ok = f["success"] is not None
        assert w["found"][0] == ok and st["n_located"] == ok
        if ok:                                                                # the oracle stops where facts() says
            assert w["j"][0] == f["success"][2] and st["n_probe_hits"] == sum(j <= f["success"][2] for j in f["hit_probes"])
            assert st["n_pairs"] == sum(f["lists"][:-1]) + f["success"][1] + 1
        else:                                                                 # every probe tried, every pair counted
            assert st["n_pairs"] == sum(f["lists"]) and st["n_probe_hits"] == len(f["hit_probes"])
    by = {c["name"]: lw.facts(oracle, c) for c in cs if c["group"] in ("seam", "zero", "trials")}
    assert {by[n]["success"][1] for n in by if n.startswith("seam_probes")} == {63, 64, 65}
    assert {by[n]["success"][1] for n in by if n.startswith("seam_run")} == {63, 64, 65}
    assert all(by[n]["behind"] >= 48 for n in by if n.startswith("seam"))     # hitting probes behind the success: uncounted
    z = by["zero_keys"]
    assert min(z["hit_probes"]) < min(z["zero"]) and any(j > max(z["zero"]) for j in z["hit_probes"] if j <= z["success_j"])
    assert by["trials130_j65"]["lists"][0] == 64                              # the first block's list ends exactly at slot 64
    assert sorted({c["trials"] for c in cs}) == [1, 50, 64, 65, 130]


def test_short_reads_case(oracle):
    c = lw.short_case()
    assert [len(x) for x in c["reads"]] == [45, 40, 40, 15] and c["min_len"] == 20
    rows = [lw.expected(oracle, c, r)[0] for r in range(4)]
    assert [int(w["found"][0]) for w in rows] == [1, 1, 1, 0] and [int(w["j"][0]) for w in rows] == [0, 12, 30, -1]
    assert rows[3]["nseq"][0] == -1                                           # below min_len: not walked
    assert 40 - 30 < 16                                                       # read 2's success is a probe of a padded window
    f = lw.facts(oracle, c, 1)                                                # read 1: 28 bases left, the prefilter does not apply
    assert f["success"] == (0, 3, 12) and f["pre_fails"] == 0


def test_set_case(oracle):
    contigs, reads = lw.set_case()
    mask = oracle.mask_from_pattern(lw.MASK_PAT)
    six = map_ref.SetIndex(oracle, contigs, mask)
    hits = six.hits(oracle.encode(lw.window(reads[0], 0)) & mask)
    assert [sum(c == k for c, _ in hits) for k in range(3)] == [30, 40, 4] and hits == sorted(hits)
    w = map_ref.walk_one(oracle, six, contigs, reads[0], mask, 0.30, 50)
    assert (w["found"], w["contig"], w["j"], w["rank"], w["n_pairs"]) == (1, 2, 0, 73, 74)
    rows1, _, _ = map_ref.map_reads_ref(oracle, contigs, reads, mask, 0.30, 50, 500, strands=1)
    rows3, st3, _ = map_ref.map_reads_ref(oracle, contigs, reads, mask, 0.30, 50, 500, strands=3)
    assert rows1["found"].tolist() == [1, 0] and rows3["found"].tolist() == [1, 1] and rows3["strand"].tolist() == [1, -1]
    assert rows3["contig"].tolist() == [2, 1] and st3[1]["n_pairs"] == 6


def test_redo_case(oracle):
    g, x, j = lw.redo_case(oracle)
    mask = oracle.mask_from_pattern(lw.MASK_PAT)
    w, st = oracle.locator(np.frombuffer(g, np.uint8), mask, 0.30, np.frombuffer(x, np.uint8), np.array([0, len(x)], np.uint64), 50, 500)
    assert w["found"][0] and w["j"][0] == j and w["cost"][0] > 1384 and st["n_pairs"] >= 71     # dearer than the one-block ring's window
    hits = lw.pi.key_hits(g, lw.window(x, j), lw.MASK_PAT)
    assert len(hits) == 71 and hits[-1] == w["pos"][0]
