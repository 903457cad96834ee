"""tests/stale_cases.py judged without a GPU: the slot names are the enum's, every kept buffer has a row in the audit table of
DESIGN §3.2 and a case that claims it, every case's checker and inputs import, and every decoy is strictly larger than its case
in the quantity that sizes each claimed slot -- so the condition "no claimed slot grew" of tests/test_gpu_stale_buffers.py is
expected to hold before anyone reaches a GPU."""
import importlib
import os
import re

import pytest

import stale_cases as sc
from conftest import ROOT
from pacbioassembly_amd import _lib

CSRC = os.path.join(ROOT, "pacbioassembly_amd", "csrc")


def enum_slots():
    src = open(os.path.join(CSRC, "pba_host.h")).read()
    body = re.search(r"enum\s*\{\s*(POOL_[A-Z_]+\s*=\s*0\s*,.*?)\}", src, re.S).group(1)
    names = [n.split("=")[0].strip() for n in body.split(",") if n.strip()]
    assert names[-1] == "POOL_COUNT"
    return names[:-1]


def audit_table():
    """{first cell without its backquotes: row} of the table of DESIGN §3.2"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    part = text.split("### 3.2", 1)[1].split("\n## ", 1)[0]
    rows = {}
    for line in part.splitlines():
        if line.startswith("| `"):
            rows[line.split("|")[1].strip().strip("`")] = line
    return rows


def test_pool_slots_are_the_enum():
    names = enum_slots()
    assert list(_lib.POOL_SLOTS) == names and len(names) <= 32 and len(set(names)) == len(names)
    assert _lib.PbaKeptBytes.pool.size == 32 * 8 and tuple(_lib.IX_CACHE_SLOTS) == ("ix_ent", "ix_off", "ix_ent2")
    # every slot of the enum is taken somewhere in the sources: a slot nobody reserves could not be exercised by any case
    srcs = "".join(open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    for n in names:
        assert len(re.findall(r"\b%s\b" % n, srcs)) >= 2, n


def test_every_kept_buffer_has_an_audit_row():
    rows = audit_table()
    missing = [s for s in sc.ALL_SLOTS if s not in rows]
    assert not missing, missing
    for s in sc.ALL_SLOTS:
        cells = [c.strip() for c in rows[s].split("|")[1:-1]]
        assert len(cells) == 3 and all(len(c) > 10 for c in cells[1:]), s     # who takes it as what; what defines it before it is read


def test_every_kept_buffer_is_claimed_by_a_case():
    claimed = {s for c in sc.CASES for s in c.slots}
    assert claimed == set(sc.ALL_SLOTS), (sorted(set(sc.ALL_SLOTS) - claimed), sorted(claimed - set(sc.ALL_SLOTS)))
    assert len({c.name for c in sc.CASES}) == len(sc.CASES) and sc.STATES[0] == "fresh" and set(sc.SCRIBBLE.values()) == {0x00, 0xFF, 0x5A}


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_checker_imports_and_decoy_is_larger(case):
    module, name = case.checker.split(":")
    assert callable(getattr(importlib.import_module(module), name)), case.checker
    assert callable(case.decoy) and callable(case.run)
    sizes = case.sizes()                                          # builds the inputs of the decoy and of the case
    for slot in case.slots:
        if slot in sc.FIXED_SLOTS:
            assert slot not in sizes
            continue
        assert slot in sizes, (case.name, slot, "claimed, and no quantity given")
        decoy, small = sizes[slot]
        assert decoy > small > 0, (case.name, slot, decoy, small)
    assert set(sizes) <= set(case.slots), (case.name, sorted(set(sizes) - set(case.slots)))
