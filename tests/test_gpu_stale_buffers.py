"""Every entry point that takes a buffer the context keeps between calls, held to its existing reference whatever an earlier
call left there (the cases, their decoys and their checkers: tests/stale_cases.py).

Each case runs in five states: straight after Context.trim() (fresh allocations), and after its decoy -- a larger call of the
same entry points -- followed by Context.scribble(0x00), scribble(0xFF), scribble(0x5A) or nothing.  0x00 hides a missing
zero-fill and 0xFF a missing sentinel-fill (PBA_LAY_NONE, FX_NO_LINE and the cost cells are all-ones); 0x5A hides neither;
the decoy's own leftovers are structured and look valid.  In every state the case's checker holds the result to the
reference, never to another state's run.  So that no state passes vacuously, every slot a case claims must be allocated
after the decoy and keep its capacity through the case: the case ran inside the scribbled memory.  If a slot grew, the test
names it and the decoy is to be enlarged.  Needs a real MI355X (-m gpu)."""
import pytest

import stale_cases as sc

pytestmark = pytest.mark.gpu


def test_every_kept_buffer_is_claimed_by_a_case():
    """pool slots in the enum's order, the scratch, the three idle index arrays, the queue counters, the staging buffer"""
    claimed = {s for c in sc.CASES for s in c.slots}
    assert claimed <= set(sc.ALL_SLOTS), sorted(claimed - set(sc.ALL_SLOTS))
    assert not set(sc.ALL_SLOTS) - claimed, sorted(set(sc.ALL_SLOTS) - claimed)


def test_kept_bytes_and_scribble(ctx):
    """kept_bytes names every slot once; trim empties all but the queue counters; scribble changes no capacity"""
    ctx.trim()
    kb = ctx.kept_bytes()
    assert tuple(kb) == sc.ALL_SLOTS and kb["queue"] == 64 and not any(v for k, v in kb.items() if k != "queue")
    ctx.scribble(0x5A)
    assert ctx.kept_bytes() == kb


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_stale_buffers(ctx, oracle, case):
    for state in sc.STATES:
        ctx.trim()
        if state == "fresh":
            case.run(ctx, oracle)
            continue
        case.decoy(ctx, oracle)
        if state in sc.SCRIBBLE:
            ctx.scribble(sc.SCRIBBLE[state])
        before = ctx.kept_bytes()
        empty = [s for s in case.slots if before[s] == 0]
        assert not empty, (case.name, state, "not allocated by the decoy", empty)
        try:
            case.run(ctx, oracle)
        except AssertionError as e:
            raise AssertionError(f"{case.name} in state {state}: {e}") from e
        after = ctx.kept_bytes()
        grew = {s: (before[s], after[s]) for s in case.slots if after[s] != before[s]}
        assert not grew, (case.name, state, "the case did not run in the decoy's buffer: enlarge the decoy", grew)
    ctx.trim()
