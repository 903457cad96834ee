"""The inputs of tests/test_gpu_locate_parked.py are what they are named for, from the genome text and the oracle's aligner
alone: where the success sits in its lane block's list, and which slots in front of it are survivors -- hits that pass the
prefilter's 32 rows and that the wavefront's sweep refuses in rows 33 .. 64, so that the walk goes on behind a sweep.  No GPU."""
import pytest

import align_rings as ar
import locate_parked_inputs as lp

CASES = lp.cases()


def late_before(blk, upto):
    return [s for s, (_, k) in enumerate(blk[:upto]) if k == "late"]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_survivors_stand_where_they_are_named(oracle, c):
    blocks = lp.slots(oracle, c)
    cl = c["claims"]
    true_at = [(b, s, j) for b, blk in enumerate(blocks) for s, (j, k) in enumerate(blk) if k == "true"]
    for blk in blocks:
        assert all(k != "other" for _, k in blk), c["name"]                   # every refusal is the prefilter's or an early sweep's
    if "success" in cl and cl["success"] is not None:
        assert true_at[0] == cl["success"], (c["name"], true_at[:2])
        assert late_before(blocks[-1], cl["success"][1]) == cl["late"], c["name"]
        # the survivors in front of the success within its own 64-slot group: what the walk resumes behind (seam64: the
        # success opens its group, the survivor at slot 63 ends the one before)
        g0 = cl["success"][1] // 64 * 64
        assert sum(s >= g0 for s in cl["late"]) >= 1 or (cl["success"][1] == g0 and g0 - 1 in cl["late"]), c["name"]
    elif "success" in cl:
        assert not true_at and len(blocks) == 1
        assert len(late_before(blocks[0], len(blocks[0]))) >= cl["min_late"], c["name"]
        assert sum(k == "pre" for _, k in blocks[0]) >= 5, c["name"]
    else:
        b, s, j = true_at[0]
        assert b == cl["success_block"] and j == cl["success_j"] and len(blocks) == 2, (c["name"], true_at[0])
        assert len(late_before(blocks[0], len(blocks[0]))) >= 3                # failed survivors in the first lane block ...
        assert len(late_before(blocks[1], s)) >= 1                              # ... and in the second, in front of the success
        assert sum(k == "pre" for _, k in blocks[0]) >= 5
        assert {jj for jj, _ in blocks[0]} >= {0, 5, 30, 40, 63}               # probes of the first block that found their key


def test_the_cases_cover_what_the_walk_resumes():
    by = {c["name"]: c["claims"] for c in CASES}
    assert [len(by[n]["late"]) for n in ("behind1", "behind2", "behind3")] == [1, 2, 3]       # one, two and three sweeps
    assert by["seam63"]["success"][1] == 63 and by["seam64"]["success"][1] == 64 and by["chunk3"]["success"][1] // 64 == 2
    assert 62 in by["seam63"]["late"] and 63 in by["seam64"]["late"]
    assert {s // 64 for s in by["chunk3"]["late"]} == {0, 1, 2}
    lens = sorted(len(c["reads"][0]) for c in CASES)
    assert lens[0] == 600 and lens[-1] == 2200                                   # ring 1 on their own:
    assert all(ar.nb1(ar.max_dst_of(n, n + 10000, lp.R)) == 1 for n in lens)
    md = ar.max_dst_of(len(lp.pilot_read()), 1 << 20, lp.R)                      # ... ring 2 behind the pilot read
    assert ar.nb1(md) == 2


def test_redo_read_sits_behind_survivors(oracle):
    c, j = lp.redo_case(oracle)
    x, g = c["reads"][0], c["g"]
    blk = lp.slots(oracle, c)[0]
    mine = [(s, k) for s, (jj, k) in enumerate(blk) if jj == j]
    kinds = [k for _, k in mine]
    assert kinds.count("late") == 2 and kinds[0] == "late" and kinds.count("pre") >= 73 and kinds[-1] == "true"
    assert mine[-1][0] >= 64                                                    # the re-run is asked for from the second chunk
    assert ar.nb1(ar.max_dst_of(len(x), len(g), lp.R)) == 1
