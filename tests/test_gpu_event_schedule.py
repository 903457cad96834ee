"""The event schedule of the bit-vector sweep (align_bitvec.h: bitvec_pass) against the oracle, exactly: paths along the far
edge of every window, where a lane's first block takes the hand-off of a lane that has just closed (the one-step skew of
`valid`), and lengths at which segment end, close, open and diagonal entry fall on one step -- through every entry point that
shares the sweep, in rings 1 and 2.  tests/event_schedule_inputs.py builds the inputs, tests/test_event_schedule_cpu.py proves
them from the oracle.  Every case asserts its ring and what the narrow pass certified by itself through last_profile(): a
re-run at the reference band would hide a wrong narrow sweep.  Needs a real MI355X (-m gpu)."""
import pytest

import align_rings as ar
import event_schedule_inputs as ev
import test_gpu_align_rings as rings
from pacbioassembly_amd.engine import PBA_KERNEL_BITVEC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("form", ["checkpoint", "stream"])
@pytest.mark.parametrize("NB", [1, 2])
def test_edge_hugging_paths(ctx, oracle, NB, form, monkeypatch):
    """k_trace_pairs<NB> in both forms, results and edit scripts: gaps of w - RB - 1 .. w bases towards the free end and of
    wl - 1 bases on the other side are certified by the narrow sweep itself -- nothing is re-run."""
    ok, _ = ev.hug_pairs(NB)
    if form == "stream":
        monkeypatch.setenv("PBA_TRACE_STREAM", "1")
    prof = rings.check_batch(ctx, oracle, ok, ev.HUG_R, PBA_KERNEL_BITVEC, scripts=True)
    assert prof["nb_first"] == NB and prof["n_first"] == len(ok.pairs) and prof["n_redo"] == 0


@pytest.mark.parametrize("NB", [1, 2])
def test_edge_hugging_align_pairs(ctx, oracle, NB):
    """k_align_pairs<NB> also reports D(m,m), the end of the diagonal, and re-runs a pair whose window cannot vouch for that
    cell: behind a gap that is the cheapest way to the free end it costs more than w (test_event_schedule_cpu.py), so the
    deletions are re-run -- all of them and nothing else of the certified batch -- and the 2 wl > w insertion of the other."""
    ok, redo = ev.hug_pairs(NB)
    prof = rings.check_batch(ctx, oracle, ok, ev.HUG_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == NB and prof["n_first"] == len(ok.pairs)
    assert prof["n_redo"] == sum(x["kind"] == "del" for x in ok.meta) == 5
    prof = rings.check_batch(ctx, oracle, redo, ev.HUG_R, PBA_KERNEL_BITVEC)
    assert prof["nb_first"] == NB and prof["n_redo"] == len(redo.pairs) == 1


@pytest.mark.parametrize("NB", [1, 2])
def test_coinciding_events(ctx, oracle, NB):
    """Short pairs in their whole band and pairs failing at rows 11, 32, 33, 64, 65 and right after the ring wrap: nothing is
    re-run, the scripts of the same batch agree too."""
    B = ev.forced(NB, ev.coin_pairs(NB))
    for scripts in (False, True):
        prof = rings.check_batch(ctx, oracle, B, ev.COIN_R, PBA_KERNEL_BITVEC, scripts=scripts)
        assert prof["nb_first"] == NB and prof["n_first"] == len(B.pairs) and prof["n_redo"] == 0, scripts


def test_coinciding_events_streamed(ctx, oracle, monkeypatch):
    """the streamed trace form on the ring-1 batch (the scratch of a wavefront is sized for the longest pair of the call)"""
    B = ev.coin_pairs(1)
    monkeypatch.setenv("PBA_TRACE_STREAM", "1")
    prof = rings.check_batch(ctx, oracle, B, ev.COIN_R, PBA_KERNEL_BITVEC, scripts=True)
    assert prof["nb_first"] == 1 and prof["n_redo"] == 0


@pytest.mark.parametrize("row", [(1, 2), (2, 2)])
def test_drivers_in_rings_1_and_2(ctx, oracle, row):
    """k_locate<NB> and k_spaced_round<NB>: forty reads of 1 - 1.5 kb against a 60 kb genome behind a filler read that sizes
    the plan -- first-success order, n_pairs and every column against the oracle (the comparison of the ring suite, which
    runs it in rings 3 and 6)."""
    rings.test_drivers_in_forced_rings(ctx, oracle, row)
