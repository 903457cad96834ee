"""The all-vs-all walk (overlap.h: k_ovl_walk<NB>, k_ovl_walk_rc<NB>) in every ring, stage and parked-run edge, held to the plain
model (overlap_ref.walk_composition) on the inputs of walk_ring_inputs.py; test_walk_rings_cpu.py proves what each input is.
Every comparison is exact: rows, n_overlaps, n_pairs, n_candidates, n_probe_entries, n_prefiltered and n_listed as
test_gpu_overlap_edges.check holds them, and with them the rings that ran -- the ctx profile of the walk (nb_first, n_first,
nb_redo, n_redo) and the call's n_redo and wide_first -- against what walk_ring_inputs.stages derives on the CPU.

  A  the lane-held one-hot of align_bitvec<NB, BAIL> (LANE_HOT: dmw, re-armed in segment_done and at the diagonal's entry):
     the first failing row at the first, second, 31st and last row of every block, rings 1, 2, 3 and 6, as the last row of the
     pair and with clean rows behind it; the row sweep on rings 1 and 3 cross-checks the inputs
  B  every plan row: its first launch, the middle ring and the reference band, plainly, started wider (PBA_OVL_WIDE) and
     through the sampled decision (PBA_OVL_SAMPLE_MIN); rows (2, 4) and (4, 8) through k_ovl_walk_rc as well
  C  the parked candidate at slot 0, 63 and 64 of its target's list, past its item's end, in front of a candidate that would
     succeed in the narrow ring, two in one item; forward and on the other strand

What this cannot show: a sweep that is never given up ends uncertified and is parked all the same -- no counter separates the
two -- and the ring of a launch in the middle of a call (only the first launch and the last resumed one are in the profile).
Needs a real MI355X (-m gpu)."""
import pytest

import walk_ring_inputs as wi
from pacbioassembly_amd.engine import PBA_KERNEL_BITVEC, PBA_KERNEL_ROWSWEEP
from test_gpu_overlap_edges import check

pytestmark = pytest.mark.gpu

HOOKS = ("PBA_OVL_ROOM", "PBA_OVL_CAPFILL_PCT", "PBA_OVL_SAMPLE_MIN", "PBA_OVL_MAX_CANDIDATES", "PBA_OVL_WIDE")
ENVS = {None: {}, "wide": {"PBA_OVL_WIDE": "1"}, "sample": {"PBA_OVL_SAMPLE_MIN": "1"}}


def run(ctx, monkeypatch, W, view="forward", env=None, kernel=PBA_KERNEL_BITVEC):
    """one call on the set of W (view "rc": the reverse-complement pass alone, over the set with its queries flipped): rows and
    counters against the model, the rings and stages against wi.stages"""
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    what = f"{W['name']} {view} {env}"
    S = ctx.seqs_from_list(W["texts"], strict_acgt=True)
    args = (S, W["mask"], W["R"], W["max_trial"], W["overlap_min"])
    if view == "forward":
        got, st = ctx.overlap_all(*args, t_lo=W["t_lo"], t_hi=W["t_hi"], kernel=kernel)
    else:
        got, sts = ctx.overlap_strands(*args, strands=2, t_lo=W["t_lo"], t_hi=W["t_hi"], kernel=kernel)
        assert (got["strand"] == -1).all()
        st = sts[1]
    prof = ctx.last_profile()
    print(what, {k: prof[k] for k in ("nb_first", "n_first", "nb_redo", "n_redo")}, st["n_redo"], st["wide_first"])
    check(got, st, W, kernel, what)
    if kernel == PBA_KERNEL_ROWSWEEP:
        assert (prof["nb_first"], prof["nb_redo"], prof["n_redo"], st["n_redo"]) == (0, 0, 0, 0), what
        return None
    want = wi.stages(W, env)
    print(what, want["launches"])
    assert {k: prof[k] for k in ("nb_first", "n_first", "nb_redo", "n_redo")} == {k: want[k] for k in ("nb_first", "n_first", "nb_redo", "n_redo")}, what
    assert (st["n_redo"], st["wide_first"]) == (want["parked"], want["wide_first"]), what
    return want


@pytest.mark.parametrize("case", wi.COLLECT_CASES, ids=lambda c: f"ring{c[0]}.{c[1]}")
def test_lane_held_one_hot_at_every_block_edge(ctx, oracle, monkeypatch, case):
    """k_ovl_walk<NB>, NB = 1, 2, 3, 6: every planted failure is found at its row (a missed one would pass and be a row, an
    early one would lose a true pair), in the ring the set was built for, nothing parked."""
    NB, _ = case
    W = wi.model(oracle, wi.collect_set(*case))
    assert len(W["rows"]) > 0
    want = run(ctx, monkeypatch, W)
    assert want["launches"] == [(NB, "first", len(wi.items_of(W)))] and want["parked"] == 0
    if case in ((1, 0), (3, 0)):
        run(ctx, monkeypatch, W, kernel=PBA_KERNEL_ROWSWEEP)


@pytest.mark.parametrize("env", list(ENVS), ids=lambda e: e or "plain")
@pytest.mark.parametrize("row", list(wi.STAGE_ROWS), ids=str)
def test_every_plan_row_in_every_stage(ctx, oracle, monkeypatch, row, env):
    """the first launch, the middle ring and the reference band of every plan row, with the runs each stage takes"""
    W = wi.model(oracle, wi.stage_set(row))
    want = run(ctx, monkeypatch, W, env=env)
    if env is None:
        mid = wi.nb_mid_of(*row)
        assert want["nb_first"] == row[0] and want["nb_redo"] in ((row[1], mid, 0) if want["parked"] else (0,))
    if env == "wide":
        assert want["nb_first"] == (wi.nb_mid_of(*row) or row[1]) and want["wide_first"] == 1


@pytest.mark.parametrize("row", wi.RC_ROWS, ids=str)
def test_plan_rows_on_the_other_strand(ctx, oracle, monkeypatch, row):
    """k_ovl_walk_rc through a middle ring (3 and 6) and at the band of rings 4 and 8"""
    V = wi.model(oracle, wi.stage_set(row), "rc")
    want = run(ctx, monkeypatch, V, view="rc")
    assert [(nb, form) for nb, form, _ in want["launches"]] == [(row[0], "first"), (wi.nb_mid_of(*row), "redo"), (row[1], "redo_band")]


@pytest.mark.parametrize("view", ["forward", "rc"])
@pytest.mark.parametrize("name", wi.PARK_CASES)
def test_parked_candidate_wherever_it_sits(ctx, oracle, monkeypatch, name, view):
    """the parked candidate's slot, what follows it in its run and in its item: resumed at the band of ring 2, never tried
    twice, and nothing behind it tried before the resume"""
    C = wi.parked_set(name)
    W = wi.model(oracle, C, view)
    want = run(ctx, monkeypatch, W, view=view)
    assert want["launches"][0][:2] == (1, "first") and want["launches"][1:] == [(2, "redo_band", len(C["parked"]))]
