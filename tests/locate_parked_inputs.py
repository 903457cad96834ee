"""Deterministic inputs for k_locate's walk where it goes on BEHIND a sweep (pba_drivers.hip).  Across align_dispatch the walk
keeps its wave-uniform state -- the survivors and failures of the 64-slot group, the hit mask and length of the lane block's
list, where the count of failed hits has got to, chunk, lane block, the counters -- in scalar registers that the compiler
moves in and out of vector lanes and scratch memory around the sweep (a form that parked them in LDS
was built against these inputs, measured and dropped).  What can go wrong there shows only behind a sweep that FAILED: so
every case plants survivors, hits that pass the prefilter's 32 rows and are refused by the wavefront's sweep in rows 33 .. 64,
in front of the place that ends the walk, on the recipe of locate_walk_inputs.py (same genome builder, same kinds of places).

  behind1 / 2 / 3   the success behind one, two and three survivors of its own 64-slot group, prefilter failures between them
  seam63 / seam64   one key's list across slots 63 | 64: the success at slot 63 behind a survivor at slot 62, and at slot 64
                    (the second chunk's first) behind a survivor at slot 63
  chunk3            the success at slot 131, in the third chunk, survivors in every chunk and at slots 128 and 130
  block2            trials = 130: the success at probe 72, in the second lane block, survivors at probes of the first block
                    and one in the second; probes that found their key are counted across the break
  none_late         never located: five survivors and as many prefilter failures, every sweep fails late
  redo_case         a read the narrow pass cannot certify, behind two survivors and the 70 prefilter failures of
                    locate_walk_inputs.redo_case: handed to the re-run with its counters held

No GPU in here.  slots() measures from the genome text and the oracle what every list slot of a case is;
test_locate_parked_inputs_cpu.py holds that against the claims below, test_gpu_locate_parked.py runs the kernels."""
import numpy as np

import align_rings as ar
import locate_walk_inputs as lw
import prefilter_inputs as pi

R = 0.30
MIN_LEN = 500
SURV = ("surv",)


def with_surv(j, n, k, surv):
    """probe j has n places, the k-th (from 0) the read itself, those of `surv` survivors, the others prefilter failures"""
    return [(j, SURV if i in surv else (("true",) if i == k else lw.FAILS[i % len(lw.FAILS)])) for i in range(n)]


def cases():
    """claims: late = slots of the success's lane block, in front of the success, that fail in rows 33 .. 64 (exactly these);
    success = (lane block, slot, j) or None"""
    out = [
        lw.case("behind1", 9501, with_surv(0, 12, 11, (3,)), read_len=600, claims=dict(success=(0, 11, 0), late=[3])),
        lw.case("behind2", 9502, with_surv(0, 12, 11, (0, 7)), read_len=1100, claims=dict(success=(0, 11, 0), late=[0, 7])),
        lw.case("behind3", 9503, with_surv(0, 14, 13, (2, 3, 12)), read_len=2200, claims=dict(success=(0, 13, 0), late=[2, 3, 12])),
        lw.case("seam63", 9504, with_surv(0, 70, 63, (5, 62)), read_len=700, claims=dict(success=(0, 63, 0), late=[5, 62])),
        lw.case("seam64", 9505, with_surv(0, 70, 64, (5, 63)), read_len=700, claims=dict(success=(0, 64, 0), late=[5, 63])),
        lw.case("chunk3", 9506, with_surv(0, 140, 131, (10, 64, 100, 128, 130)), read_len=900,
                claims=dict(success=(0, 131, 0), late=[10, 64, 100, 128, 130])),
        lw.case("block2", 9507, lw.spread([0], 3) + [(5, SURV)] + lw.spread([30], 2) + [(40, SURV), (63, SURV)] + lw.spread([64], 2) +
                [(70, SURV)] + with_surv(72, 2, 1, ()), trials=130, read_len=800, claims=dict(success_block=1, success_j=72, min_late=4)),
        lw.case("none_late", 9508, [(0, SURV), (0, SURV)] + lw.spread([3], 2) + [(3, SURV), (20, SURV)] + lw.spread([20], 3) + [(49, SURV)],
                read_len=1500, claims=dict(success=None, min_late=5)),
    ]
    for c in out:
        c["R"], c["min_len"] = R, MIN_LEN
    return out


_REDO = []


def redo_case(oracle):
    """locate_walk_inputs.redo_case with two survivors and three prefilter failures of the same probe planted in front: (case, j)"""
    if not _REDO:
        g, x, j = lw.redo_case(oracle)
        rng = np.random.RandomState(9509)
        gen = lw.Genome(rng)
        lw.plant_all(rng, gen, x, [(j, SURV)] + lw.spread([j], 3) + [(j, SURV)])
        c = dict(name="redo", g=gen.text(60) + g, reads=[x], trials=50, R=R, min_len=MIN_LEN, pat=lw.MASK_PAT, claims={})
        _REDO.append((c, j))
    return _REDO[0]


def pilot_read():
    """an unrelated read long enough for the plan to start in ring 2"""
    return ar.pilot(ar.row_of(2, 2)[0], R, seed=7)[0]


def slots(oracle, c, read=0):
    """[per lane block: [(j, kind)] per list slot], kind = "true" (the aligner accepts), "pre" (refused within rows 11 .. 32, both
    sides >= 32 elements: the prefilter's), "late" (refused in rows 33 .. 64: a survivor the wavefront's sweep fails), "other".
    Blocks up to and including the one of the first success; every slot of that block is classified."""
    g, x, pat = c["g"], c["reads"][read], c["pat"]
    mask = oracle.mask_from_pattern(pat)
    nprobe = min(c["trials"], len(x))
    out = []
    for j0 in range(0, nprobe, lw.PROBES):
        blk = []
        for j in range(j0, min(j0 + lw.PROBES, nprobe)):
            if oracle.encode(lw.window(x, j)) & mask == 0:
                continue
            for p in pi.key_hits(g + b"T" * 15, lw.window(x, j), pat):
                res = oracle.align(x[j:], g[p:], c["R"])
                if res["rc"] > 0:
                    kind = "true"
                elif res["fail_row"] and res["fail_row"] <= 32 and min(res["len_a"], res["len_b"]) >= 32:
                    kind = "pre"
                elif 33 <= res["fail_row"] <= 64:
                    kind = "late"
                else:
                    kind = "other"
                blk.append((j, kind))
        out.append(blk)
        if any(k == "true" for _, k in blk):
            break
    return out


_EXPECTED = {}


def expected(oracle, c, pilot: bool):
    """Oracle.locator's rows and stats of the case's read, alone or with the pilot read behind it in the same call"""
    key = (c["name"], pilot)
    if key not in _EXPECTED:
        texts = c["reads"] + ([pilot_read()] if pilot else [])
        reads = np.frombuffer(b"".join(texts), np.uint8)
        offs = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.uint64)
        _EXPECTED[key] = oracle.locator(np.frombuffer(c["g"], np.uint8), oracle.mask_from_pattern(c["pat"]), c["R"], reads, offs,
                                        c["trials"], c["min_len"])
    return _EXPECTED[key]
