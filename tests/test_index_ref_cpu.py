"""Pin tests/index_ref.py (the numpy restatement the GPU index tests compare with) to Oracle.index, which
test_oracle_vs_ref.py pins to the reference's own code.  CPU only."""
import numpy as np
import pytest

from conftest import GOLD
from index_ref import np_index, runs

SEED_MASKS = [l.strip() for l in open(f"{GOLD}/seeds.txt") if l.strip()]
LENGTHS = [0, 1, 5, 15, 16, 17, 18, 33, 100, 2049, 20015, 20016, 20017, 20036, 40015, 40016, 40017, 40040, 50000, 100000]


KINDS = ["random", "repeat", "mixed", "poly_t", "poly_a", "random_then_t"]


def make_text(kind: str, n: int) -> bytes:
    if kind in ("random", "random_then_t"):
        t = np.frombuffer(b"ACGT", np.uint8)[np.random.RandomState(n + 1).randint(0, 4, n)].tobytes()
        # random_then_t: not periodic, ending in a T run -- code-3-padded tail windows collide with real all-T windows
        return t if kind == "random" else t[:n - n // 3] + b"T" * (n // 3)
    unit = {"repeat": b"ACGGT", "mixed": b"ACGTNacgt", "poly_t": b"T", "poly_a": b"A"}[kind]
    return (unit * (n // len(unit) + 1))[:n]


def masks(oracle):
    return [0, 0xFFFFFFFF, 0x000000FF, 0xC0000003, 0x00000300] + [oracle.mask_from_pattern(p) for p in SEED_MASKS]


def test_seed_masks_file():
    assert len(SEED_MASKS) == 8 and all(len(p) == 16 and set(p) <= set("1*") for p in SEED_MASKS)


def first_difference(k, p, ok, op):
    """First differing entry: its key, the key's run length in the oracle, and what np_index gave there."""
    m = min(k.size, ok.size)
    bad = np.flatnonzero((k[:m] != ok[:m]) | (p[:m] != op[:m]))
    i = int(bad[0]) if bad.size else m
    key = int(ok[i]) if i < ok.size else int(k[i])
    return (f"entry {i}: key {key:#010x} has {int((ok == key).sum())} entries in the oracle at {op[ok == key][:8].tolist()}, "
            f"np_index has {int((k == key).sum())} at {p[k == key][:8].tolist()}; sizes {k.size} / {ok.size}")


@pytest.mark.parametrize("mode", ["all", "head_tail"])
@pytest.mark.parametrize("kind", KINDS)
def test_np_index_equals_oracle_index(oracle, kind, mode):
    failures = []                                          # every failing (n, mask) is reported, not the first alone
    for n in LENGTHS:
        text = make_text(kind, n)
        for mask in masks(oracle):
            ok, op, orv, onk = oracle.index(text, mask, mode)
            k, p, rv = np_index(text, mask, mode)
            tag = f"{kind} {mode} n={n} mask={mask:#010x}"
            assert k.dtype == np.uint32 and p.dtype == np.int32, tag
            if not (np.array_equal(k, ok) and np.array_equal(p, op)):
                failures.append(f"{tag}: {first_difference(k, p, ok, op)}")
                continue
            if runs(k)[0].size != onk:
                failures.append(f"{tag}: {runs(k)[0].size} distinct keys, the oracle has {onk}")
            if mode == "head_tail":
                if rv != orv:                              # (orc_index_all returns the entry count, not get_seedmap's value)
                    failures.append(f"{tag}: visited {rv}, the oracle returns {orv}")
            elif rv != n or orv != k.size:
                failures.append(f"{tag}: visited {rv} / oracle entry count {orv} for {k.size} entries")
            if mask == 0 and k.size:
                failures.append(f"{tag}: {k.size} entries under mask 0")
    assert not failures, f"{len(failures)} cases differ:\n" + "\n".join(failures)


def test_random_then_t_tail_windows_collide_with_real_t_windows():
    n = 100
    k, p, _ = np_index(make_text("random_then_t", n), 0xFFFFFFFF, "all")
    at = p[k == 0xFFFFFFFF]
    assert (at <= n - 16).sum() >= 10 and (at > n - 16).sum() == 15     # real all-T windows and padded ones under one key


def test_np_index_head_positions_precede_tail_positions(oracle):
    """A 16-mer planted in head and tail: the list holds the head position first, then the tail ones descending."""
    n = 60000
    t = bytearray(make_text("random", n))
    w = b"GATTACAGATTACAGG"
    for at in (100, 19000, n - 16 - 5, n - 16 - 700):
        t[at:at + 16] = w
    text = bytes(t)
    k, p, _ = np_index(text, 0xFFFFFFFF, "head_tail")
    ok, op, _, _ = oracle.index(text, 0xFFFFFFFF, "head_tail")
    assert np.array_equal(k, ok) and np.array_equal(p, op)
    key = oracle.encode(w)
    assert p[k == key].tolist() == [100, 19000, n - 16 - 5, n - 16 - 700]
