"""Deterministic inputs for the lane-parallel candidate walk of k_locate (pba_drivers.hip, csrc/locate_walk.h): a read's
probes are keyed and looked up 64 at a time, their hits form one list (probe ascending, inside a probe the index's run order)
that is prefiltered 64 slots at a time, and the walk stops at the first success.  Every case plants, for chosen probes of one
read, places in a small genome: copies of the probe's window that the reference's aligner refuses within rows 11 .. 32 (the
prefilter's), refuses in rows 33 .. 64 (a survivor of the prefilter), or accepts (the read's own text: it ends the walk).
No GPU in here.  facts() measures from the genome text and the oracle what a case is -- the list of every lane block, where
the first success sits in it, what the hits in front of it are; test_locate_walk_cpu.py holds that against the case's claims,
test_gpu_locate_walk.py runs the kernels on the same cases against Oracle.locator / map_ref.

How a place stays the place of ONE probe.  Probe j of read x looks for the window x[j : j + 16] at the mask's care positions.
A refused place keeps the window (another base at some of the mask's wildcards) and the read's next bases up to row `keep`, and
from there on holds, row by row, a base the read does not have there.  The last position of every shifted window is a care
position that lies in that stretch (keep = 16), so no later probe hits inside the place; the 15 bases in front of a place differ
one by one from x[j - 15 : j], so probe j - s does not hit s bases earlier (its first position is a care position).  A survivor
(keep = 30) and an accepted place are hit by the probes behind j as well: those hits sit behind j's in the list."""
import numpy as np

import align_rings as ar
import map_ref
import prefilter_inputs as pi
from conftest import MASK_PAT
from pacbioassembly_amd import engine as eng

ACGT = b"ACGT"
WILD = (4, 7, 10, 12)                  # rows of a forward MASK_PAT pair at which the sides may differ inside the window
PROBES = 64                            # probes of a lane block (PBA_LW_PROBES), slots of a chunk (PBA_WAVE)
LOC_COLS = ("nseq", "found", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "n_pairs")
STAT_KEYS = ("n_reads_kept", "n_probe_hits", "n_pairs", "n_located", "n_cells")


def window(x: bytes, j: int) -> bytes:
    """the 16 bases probe j keys: past the read's end they read as code 3 (locator.cpp:62-63 sees NUL there)"""
    return x[j:j + 16].ljust(16, b"T")


def another(rng, b: int) -> int:
    return ACGT[(ACGT.index(b) + 1 + rng.randint(3)) % 4]


def refused(rng, x: bytes, j: int, diff=WILD, keep: int = 16, n: int = 48) -> bytes:
    """n bases that probe j of x hits: the window with another base at the wildcard rows `diff`, x up to row `keep`, and from
    row keep + 1 on a base x does not have at that row (random where x has ended)"""
    y = bytearray(window(x, j))
    for r in diff:
        y[r - 1] = another(rng, y[r - 1])
    for i in range(16, n):
        src = x[j + i] if j + i < len(x) else None
        y.append(src if src is not None and i < keep else (another(rng, src) if src is not None else ACGT[rng.randint(4)]))
    return bytes(y)


class Genome:
    """places in the order they are planted, random spacers of 20 .. 40 bases between them"""

    def __init__(self, rng, lead: int = 120):
        self.rng, self.parts, self.n = rng, [ar.rand_seq(rng, lead)], lead

    def plant(self, y: bytes, not_before=b"") -> int:
        """not_before: the read's bases in front of the probe; base by base the spacer's end differs from them"""
        sp = bytearray(ar.rand_seq(self.rng, int(self.rng.randint(20, 41))))
        for k in range(1, min(15, len(not_before)) + 1):
            if sp[-k] == not_before[-k]:
                sp[-k] = another(self.rng, sp[-k])
        self.parts += [bytes(sp), y]
        pos = self.n + len(sp)
        self.n = pos + len(y)
        return pos

    def text(self, tail: int = 150) -> bytes:
        return b"".join(self.parts) + ar.rand_seq(self.rng, tail)


# kinds of a planted place: ("fail", diff rows) refused within the prefilter's rows; ("surv",) refused in rows 33 .. 64;
# ("true",) the read's own text from the probe on
FAILS = [("fail", WILD), ("fail", (4, 7, 10))]        # (R = 0.30: the first failing row is 12, and 19 or a few rows later)


def fails(k: int, rot: int = 0):
    return [FAILS[(rot + i) % len(FAILS)] for i in range(k)]


def plant_all(rng, gen: Genome, x: bytes, layout):
    """layout: [(probe j, kind), ...] in genome order"""
    for j, kind in layout:
        before = x[:j]
        if kind[0] == "true":
            gen.plant(x[j:], before)
        elif kind[0] == "surv":
            gen.plant(refused(rng, x, j, (4, 7, 10), keep=30, n=72), before)
        else:
            gen.plant(refused(rng, x, j, kind[1]), before)


def case(name, seed, layout, trials=50, read_len=520, R=0.30, min_len=500, claims=None, read=None, **more):
    rng = np.random.RandomState(seed)
    x = ar.rand_seq(rng, read_len) if read is None else read(rng)
    gen = Genome(rng)
    plant_all(rng, gen, x, layout)
    return dict(name=name, g=gen.text(), reads=[x], trials=trials, R=R, min_len=min_len, pat=MASK_PAT, claims=claims or {}, **more)


def one_key(n: int, k: int, probe: int = 0, surv=()):
    """probe `probe` has n hits, the k-th (from 0) is the read itself; `surv`: hits in front of it that survive 32 rows"""
    return [(probe, ("surv",) if i in surv else (("true",) if i == k else FAILS[i % len(FAILS)])) for i in range(n)]


def spread(probes, each: int):
    """`each` refused places for every probe of `probes`, probe after probe"""
    return [(j, kind) for j in probes for kind in fails(each, j)]


def zero_key_read(rng):
    """probes 5 .. 9 key sixteen A: key 0, never inserted (locator.cpp:64)"""
    x = bytearray(ar.rand_seq(rng, 520))
    x[5:25] = b"A" * 20
    x[4:5] = x[25:26] = b"C"                                          # (probes 4 and 10 key a care position that is not A)
    return bytes(x)


def cases():
    """every one-contig case of test_gpu_locate_walk.py; claims: what facts() must say about it"""
    out = []
    # -- run length: one key with n hits, the read's own place the k-th; the probes behind 0 hit inside that place, uncounted
    for n, k in ((1, 0), (63, 62), (64, 0), (64, 63), (65, 63), (65, 64), (128, 64), (128, 127), (129, 65), (129, 128), (129, 63)):
        out.append(case(f"run{n}_{k}", 100 + 7 * n + k, one_key(n, k), group="run",
                        claims=dict(per_probe0=n, success=(0, k, 0), behind=49, array_fails=0)))
    out.append(case("run65_64_surv", 171, one_key(65, 64, surv=(10, 63)), group="run",
                    claims=dict(per_probe0=65, success=(0, 64, 0), array_fails=2)))
    out.append(case("run65_64_R15", 172, one_key(65, 64), R=0.15, group="run",
                    claims=dict(lists=[65 + 49], success=(0, 64, 0), array_fails=0)))
    # -- chunk seam: the list crosses slots 63 | 64 between two probes (probe 0 fills slots 0 .. 63) ...
    for c1 in (0, 1):
        out.append(case(f"seam_probes_{64 + c1}", 200 + c1, spread([0], 64) + one_key(c1 + 1, c1, probe=1), group="seam",
                        claims=dict(per_probe0=64, success=(0, 64 + c1, 1), behind=48)))
    out.append(case("seam_probes_63", 202, one_key(64, 63), group="seam", claims=dict(per_probe0=64, success=(0, 63, 0), behind=49)))
    # ... and inside probe 1's run (probe 0 has ten hits)
    for c1 in (53, 54, 55):
        out.append(case(f"seam_run_{10 + c1}", 210 + c1, spread([0], 10) + one_key(c1 + 1, c1, probe=1), group="seam",
                        claims=dict(per_probe0=10, success=(0, 10 + c1, 1), behind=48)))
    # -- position of the success: j = 0, 1, trials - 1, and none at all
    out.append(case("pos_j0", 300, one_key(3, 2), group="pos", claims=dict(success=(0, 2, 0), behind=49)))
    out.append(case("pos_j1", 301, spread([0], 2) + one_key(2, 1, probe=1), group="pos", claims=dict(success=(0, 3, 1), behind=48)))
    out.append(case("pos_j49", 302, spread([3, 20], 3) + one_key(1, 0, probe=49), group="pos", claims=dict(success=(0, 6, 49), behind=0)))
    out.append(case("pos_none", 303, spread([0, 7, 31, 49], 5) + spread([50], 2), group="pos", claims=dict(lists=[20], success=None)))
    out.append(case("pos_none_long", 304, spread([0, 49], 40), group="pos", claims=dict(lists=[80], success=None)))
    # -- probe count
    out.append(case("trials1", 400, one_key(2, 1), trials=1, group="trials", claims=dict(lists=[2], success=(0, 1, 0), behind=0)))
    out.append(case("trials64", 401, spread([0, 62], 2) + one_key(1, 0, probe=63), trials=64, group="trials",
                    claims=dict(lists=[5], success=(0, 4, 63), behind=0)))
    out.append(case("trials65_j64", 402, spread([0, 63], 2) + one_key(2, 1, probe=64), trials=65, group="trials",
                    claims=dict(lists=[4, 2], success=(1, 1, 64), behind=0)))
    out.append(case("trials130_j65", 403, spread(range(0, 64, 8), 8) + spread([64], 3) + one_key(1, 0, probe=65), trials=130, group="trials",
                    claims=dict(lists=[64, 3 + 1 + 62], success=(1, 3, 65), behind=62)))     # (block 1: probes 64 .. 127)
    out.append(case("trials130_none", 404, spread([1, 63, 64, 127, 129], 3) + spread([130], 2), trials=130, group="trials",
                    claims=dict(lists=[6, 6, 3], success=None)))
    # -- zero keys between hitting probes
    out.append(case("zero_keys", 500, spread([2, 12], 3) + one_key(1, 0, probe=14), read=zero_key_read, group="zero",
                    claims=dict(zero=[5, 6, 7, 8, 9], success_j=14)))
    # -- the same walk under the row sweep (k_locate<0>: nothing is prefiltered, every listed hit goes to the aligner)
    out.append(dict(case("rowsweep_run65_63", 100 + 7 * 65 + 63, one_key(65, 63), group="rowsweep",
                         claims=dict(per_probe0=65, success=(0, 63, 0))), kernel="rowsweep"))
    return out


def short_case():
    """min_len = 20: reads of 45 and 40 bases -- lanes past the read's end idle, the last 15 probes key windows padded with
    code 3 -- and one of 15 bases, below min_len.  The read of 45 lies in the genome whole; of the first read of 40 only bases
    12 .. 39, followed by T: its probes from 12 on hit there (28 bases and fewer: the prefilter does not apply), and three
    refused places of probe 12 lie in front; of the second only bases 30 .. 39: the first probe that hits keys a padded window."""
    rng = np.random.RandomState(600)
    a, b, d, c = ar.rand_seq(rng, 45), ar.rand_seq(rng, 40), ar.rand_seq(rng, 40), ar.rand_seq(rng, 15)
    gen = Genome(rng)
    plant_all(rng, gen, b, spread([12], 3))
    gen.plant(b[12:] + b"T" * 24, b[:12])
    gen.plant(d[30:] + b"T" * 24, d[:30])
    plant_all(rng, gen, a, spread([0], 2) + [(0, ("true",))])
    return dict(name="short", g=gen.text(), reads=[a, b, d, c], trials=50, R=0.30, min_len=20, pat=MASK_PAT, group="short",
                claims=dict(padded=True))


def set_case():
    """(contigs, reads): probe 0 of read 0 has 30 refused places in contig 0, 40 in contig 1 -- the 64-slot seam inside them --
    and in contig 2 three more and the read itself; read 1 is the reverse complement of a text that lies in contig 1 behind
    five refused places in contig 0 (found by the - walk of strands = 3 only)."""
    rng = np.random.RandomState(700)
    x = ar.rand_seq(rng, 520)
    z = ar.rand_seq(rng, 540)
    gens = [Genome(rng) for _ in range(3)]
    plant_all(rng, gens[0], x, spread([0], 30))
    plant_all(rng, gens[0], z, spread([0], 5))
    plant_all(rng, gens[1], x, spread([0], 40))
    plant_all(rng, gens[1], z, [(0, ("true",))])
    plant_all(rng, gens[2], x, spread([0], 3) + [(0, ("true",))])
    return [g.text() for g in gens], [x, map_ref.rc(z)]


_REDO = []                             # (the search for the read, once per session)


def redo_case(oracle):
    """One read on the recipe of test_bitvec_uncertified_pairs_rerun_at_reference_band (7.3 kb at 21 % error: dearer than the
    one-block ring's window of 1 384), its stretch of the genome, and in front of it 70 refused places of the probe that finds
    it.  Returns (genome, read, j of the success)."""
    if _REDO:
        return _REDO[0]
    g = eng.synth_genome(55, 60000)
    L = 7300
    reads, offs, starts = eng.synth_reads(56, g, 64, L, 0.07, 0.07, 0.07)
    mask = eng.mask_from_pattern(MASK_PAT)
    for r in range(64):
        x = reads[int(offs[r]):int(offs[r + 1])].tobytes()
        s = int(starts[r])
        piece = g[max(0, s - 300):s + L + 2600]
        want, _ = oracle.locator(piece, mask, 0.30, np.frombuffer(x, np.uint8), np.array([0, L], np.uint64), 50, 500)
        if want["found"][0] and want["cost"][0] > 1384:
            rng = np.random.RandomState(800)
            j = int(want["j"][0])
            gen = Genome(rng)
            plant_all(rng, gen, x, spread([j], 70))
            _REDO.append((gen.text(60) + piece.tobytes(), x, j))
            return _REDO[0]
    raise RuntimeError("no read of the recipe costs more than the narrow window")


# ----------------------------------------------------------------------------- what a case is, measured
def facts(oracle, c, read=0):
    """From the genome text and the oracle's aligner: lists = slots per lane block (up to and including the block of the
    success), per_probe0 = hits of the first hitting probe, zero = probes whose key is 0, success = (block, slot in the block's
    list, j) or None, behind = hitting probes of that block behind the success's, array_fails = hits in front of the success
    that fail in rows 33 .. 64, pre_fails = those that fail in rows 11 .. 32 with both sides >= 32 elements, hit_probes = the
    probes that found their key, up to the end of the success's block."""
    g, x, R, pat = c["g"], c["reads"][read], c["R"], c["pat"]
    mask = oracle.mask_from_pattern(pat)
    nprobe = min(c["trials"], len(x))
    f = dict(lists=[], per_probe0=None, zero=[], success=None, success_j=None, behind=0, array_fails=0, pre_fails=0, other_fails=0,
             hit_probes=[])
    for j0 in range(0, nprobe, PROBES):
        slot, hit_probes = 0, []
        for j in range(j0, min(j0 + PROBES, nprobe)):
            if oracle.encode(window(x, j)) & mask == 0:
                f["zero"].append(j)
                continue
            hits = pi.key_hits(g + b"T" * 15, window(x, j), pat)
            if not hits:
                continue
            hit_probes.append(j)
            f["hit_probes"].append(j)
            if f["per_probe0"] is None:
                f["per_probe0"] = len(hits)
            for p in hits:
                if f["success"] is None:
                    res = oracle.align(x[j:], g[p:], R)
                    if res["rc"] > 0:
                        f["success"], f["success_j"] = (j0 // PROBES, slot, j), j
                    elif res["fail_row"] and res["fail_row"] <= 32 and min(res["len_a"], res["len_b"]) >= 32:
                        f["pre_fails"] += 1
                    elif 33 <= res["fail_row"] <= 64:
                        f["array_fails"] += 1
                    else:
                        f["other_fails"] += 1
                slot += 1
        f["lists"].append(slot)
        if f["success"] is not None:
            f["behind"] = sum(j > f["success"][2] for j in hit_probes)
            break
    return f


_EXPECTED = {}


def expected(oracle, c, read=0):
    """Oracle.locator's row and stats of one read of a one-contig case, once per session"""
    key = (c["name"], read)
    if key not in _EXPECTED:
        x = c["reads"][read]
        _EXPECTED[key] = oracle.locator(np.frombuffer(c["g"], np.uint8), oracle.mask_from_pattern(c["pat"]), c["R"],
                                        np.frombuffer(x, np.uint8), np.array([0, len(x)], np.uint64), c["trials"], c["min_len"])
    return _EXPECTED[key]
