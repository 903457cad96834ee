"""pba_map_row_pair (host arithmetic, no GPU): the pair a mapped row votes with, against hand arithmetic on both strands, and
the exactness of its clip -- the oracle aligns the whole contig remainder and the clipped accessor to the same result."""
import numpy as np
import pytest

from map_ref import mutate, rand_text, rc
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import MAP_ROW_DTYPE, PbaError
from polish_helpers import clip_len

R = 0.30
READ_LEN, J = 900, 7
B_LEN = READ_LEN - J


def a_row(strand=1, contig=2, read=5, j=J, pos=100, found=1):
    r = np.zeros(1, MAP_ROW_DTYPE)[0]
    r["found"], r["strand"], r["contig"], r["read"], r["j"], r["pos"] = found, strand, contig, read, j, pos
    return r


# contig remainder longer than, equal to, shorter than the read remainder
CASES = {"longer": 5000, "equal": B_LEN, "shorter": 300}


@pytest.mark.parametrize("strand", [1, -1])
@pytest.mark.parametrize("case", list(CASES))
def test_pair_vs_hand_arithmetic_and_clip_is_exact(lib, oracle, case, strand):
    rem, pos = CASES[case], 100
    rng = np.random.default_rng(11 + rem)
    contig = rand_text(rng, pos + rem)
    seg = mutate(rng, contig[pos:pos + min(rem, 1100)], 0.12, keep=20)[:B_LEN]
    seg += rand_text(rng, B_LEN - len(seg))                    # (past the contig's end: overhang)
    walked = rand_text(rng, J) + seg                           # the text the mapper walked: rc(read) on strand -1
    assert len(walked) == READ_LEN
    pr = eng.map_row_pair(a_row(strand, pos=pos), len(contig), READ_LEN, R)
    md = 1 + int(B_LEN * R)
    want_a_len = {"longer": B_LEN + md, "equal": B_LEN, "shorter": 300}[case]
    assert clip_len(rem, B_LEN, R) == want_a_len
    assert (int(pr["a_seq"]), int(pr["a_pos"]), int(pr["a_len"])) == (2, pos, want_a_len)
    assert (int(pr["b_seq"]), int(pr["b_pos"]), int(pr["b_len"]), int(pr["flags"])) == (5, J, B_LEN, 0)
    whole = oracle.align(contig[pos:], walked[J:], R, want_ops=True)
    clipped = oracle.align(contig[pos:pos + want_a_len], walked[J:], R, want_ops=True)
    for k in ("rc", "cost", "matlen_a", "matlen_b", "len_a", "len_b", "max_dst"):
        assert whole[k] == clipped[k], (k, whole[k], clipped[k])
    assert (whole["ops"] == clipped["ops"]).all()
    assert whole["rc"] >= 0 and whole["len_a"] == want_a_len


def test_refusals(lib):
    def status(row, contig_len=6000, read_len=READ_LEN, r=R):
        with pytest.raises(PbaError) as e:
            eng.map_row_pair(row, contig_len, read_len, r)
        return e.value.status

    assert status(a_row(found=0)) == -1
    assert status(a_row(strand=0)) == -1
    assert status(a_row(j=READ_LEN)) == -1
    assert status(a_row(pos=6000)) == -1
    assert status(a_row(), r=0.0) == -1
    assert status(a_row(), r=1.0) == -1
    # b_len 59 993 -> a clipped to b_len + max_dst = 77 991 elements: beyond the accessor limit of 65 000
    assert status(a_row(), contig_len=200000, read_len=60000) == -4
    assert int(eng.map_row_pair(a_row(), 200000, 40000, R)["a_len"]) == clip_len(199900, 39993, R) <= 65000
    assert lib.pba_map_row_pair(None, 10, 10, R, None) == -1
