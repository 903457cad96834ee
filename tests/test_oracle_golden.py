"""Pin oracle/pba_oracle.c (the CPU restatement) to the golden vectors produced by the reference
itself (tests/golden/make_golden.py) and to the reference's own test KATs.  CPU only."""
import hashlib

import numpy as np
import pytest

from conftest import GOLD, gold_json, gold_npz
from pacbioassembly_amd import engine as eng

RES_KEYS = ("rc", "cost", "matlen_a", "matlen_b", "len_a", "len_b", "max_dst", "nedit")


def test_codec(oracle):
    g = gold_json("codec.json")
    for w, code in g["encode"]:
        assert oracle.encode(w.encode()) == code
    for c, v in g["c2i"]:
        assert oracle.lib.orc_c2i(c) == v
    rec = oracle.text2bin(g["seed_at_text"].encode())
    for pos, want in g["seed_at"]:
        assert oracle.seed_at(rec, pos) == want
    for pat, m in g["masks"]:
        assert oracle.mask_from_pattern(pat) == m
    for s, hexrec, back in g["text2bin"]:
        assert oracle.text2bin(s.encode()).hex() == hexrec
        assert oracle.bin2text(bytes.fromhex(hexrec)).decode() == back


def check_align_case(got, exp, tag):
    assert got["rc"] == exp["rc"], tag
    for k in ("len_a", "len_b", "max_dst"):
        assert got[k] == exp[k], (tag, k)
    if exp["rc"] >= 0:
        for k in ("cost", "matlen_a", "matlen_b"):
            assert got[k] == exp[k], (tag, k)


def test_align_kats(oracle):
    cases = gold_json("align_kat.json")
    assert len(cases) > 300
    for c in cases:
        got = oracle.align(c["a"].encode("latin1"), c["b"].encode("latin1"), c["R"], c["a_fwd"], c["b_fwd"],
                           want_ops=True)
        check_align_case(got, c["exp"], c["tag"])
        if c["exp"]["rc"] >= 0:
            assert got["nedit"] == c["exp"]["nedit"], c["tag"]
            assert (int(got["ops"][0]) if got["nedit"] else 0) == c["exp"]["first_op"], c["tag"]
            assert hashlib.sha256(bytes(got["ops"])).hexdigest()[:24] == c["exp"]["ops_sha"], c["tag"]   # whole edit script


def test_aligner_test_expectations(oracle):
    """test/aligner_test.cpp:44-117, the assertions as the reference states them."""
    ref, s1, s2, s3 = b"ACGTAACCGGTT", b"CGTAAGC", b"GTAACGGGTTAA", b"TCGTAAC"
    r = oracle.align(s1[:6], ref[:7], 0.3); assert 6 <= r["rc"] <= 7 and r["cost"] == 2
    r = oracle.align(s1[:7], ref[:8], 0.3); assert r["rc"] == 7 and r["cost"] == 2
    r = oracle.align(s3[:7], ref[:8], 0.3); assert r["rc"] == 7 and r["cost"] == 1
    r = oracle.align(s1[:7], ref[1:8], 0.3, False, False); assert r["rc"] == 7 and r["cost"] == 1
    r = oracle.align(s2, ref[2:12], 0.3); assert r["rc"] == 10 and r["cost"] == 1
    r = oracle.align(ref[1:10], ref[:10], 0.3, want_ops=True)
    assert r["rc"] == 10 and r["nedit"] == 10 and r["ops"][0] == 2 and r["cost"] == 1      # INSERT
    r = oracle.align(ref[:10], ref[1:10], 0.3, want_ops=True)
    assert r["rc"] == 9 and r["nedit"] == 10 and r["ops"][0] == 3 and r["cost"] == 1       # DELETE
    lines = open(f"{GOLD}/real_align.txt").read().split()
    assert oracle.align(lines[1].encode(), lines[0].encode(), 0.3, False, False)["rc"] > 0
    assert oracle.align(lines[3].encode(), lines[2].encode(), 0.3)["rc"] == -1


def index_inputs(case):
    if "seed" in case:
        return eng.synth_genome(case["seed"], case["len"]).tobytes()
    return (case["text_unit"].encode() * (case["len"] // len(case["text_unit"]) + 1))[:case["len"]]


def index_digest(k, p):
    return hashlib.sha256(k.astype("<u4").tobytes() + p.astype("<i4").tobytes()).hexdigest()


def test_index(oracle):
    g = gold_json("index.json")
    arrays = gold_npz("index.npz")
    b = g["ref_test_basic"]                         # test/ref_test.cpp:119-128
    k, p, rv, nk = oracle.index(b["text"].encode(), b["mask"], "head_tail")
    assert k.tolist() == b["keys"] and p.tolist() == b["pos"] and rv == b["rv"] and nk == b["nkeys"]
    sz = len(b["text"])
    assert nk == sz - 15 - 1 and sorted(p.tolist()) == list(range(sz - 16))
    for c in g["cases"]:
        k, p, rv, nk = oracle.index(index_inputs(c), c["mask"], "all" if c["mode"] == "all" else "head_tail")
        assert k.size == c["n"], c["name"]
        assert index_digest(k, p) == c["sha256"], c["name"]
        if c["mode"] == "head_tail":
            assert rv == c["rv"] and nk == c["nkeys"], c["name"]
        if c["name"] + "_keys" in arrays:
            assert (k == arrays[c["name"] + "_keys"]).all() and (p == arrays[c["name"] + "_pos"]).all()


def locator_inputs(m):
    g = eng.synth_genome(m["genome_seed"], m["genome_len"])
    reads, offs, _ = eng.synth_reads(m["reads_seed"], g, m["n_reads"], m["read_len"], *m["err"])
    if m["name"] == "short_mix":
        n, rl = m["n_reads"], m["read_len"]
        cut = [(int(offs[i]), int(offs[i]) + (300 if i % 3 == 0 else rl)) for i in range(n)]
        reads = np.concatenate([reads[a:b] for a, b in cut])
        offs = np.concatenate([[0], np.cumsum([b - a for a, b in cut])]).astype(np.uint64)
    return g, reads, offs


def check_locator_rows(rows, want, cols, name):
    for ci, col in enumerate(cols):
        if col in ("cost", "matlen_a", "matlen_b", "seglen", "pos", "j"):
            sel = want[:, cols.index("found")] == 1
            assert (rows[col][sel] == want[sel, ci]).all(), (name, col)
        else:
            assert (rows[col] == want[:, ci]).all(), (name, col)


@pytest.mark.parametrize("name", ["cfg1_R30", "cfg1_R15", "cfg1_pacbio", "short_mix", "r15k_R30", "r15k_R15"])
def test_locator(oracle, name):
    meta = {m["name"]: m for m in gold_json("locator.json")}[name]
    want = gold_npz("locator.npz")[name]
    g, reads, offs = locator_inputs(meta)
    rows, st = oracle.locator(g, meta["mask"], meta["R"], reads, offs, meta["trials"], meta["min_len"], nthreads=8)
    check_locator_rows(rows, want, meta["columns"], name)
    for k, v in meta["stats"].items():
        assert st[k] == v, (name, k)


def spaced_inputs(m, text2bin):
    g = eng.synth_genome(m["genome_seed"], m["genome_len"])
    reads, offs, _ = eng.synth_reads(m["reads_seed"], g, m["n_reads"], m["read_len"])
    rl = m["read_len"]
    file = b"".join(text2bin(reads[int(offs[i]):int(offs[i + 1])].tobytes()) for i in range(m["n_reads"]))
    rec_offs = np.array([i * (4 + (rl + 3) // 4) for i in range(m["n_reads"])], np.uint64)
    return g, file, rec_offs


@pytest.mark.parametrize("name", ["ss_30k", "ss_50k", "ss_12k"])
def test_spaced_round(oracle, name):
    meta = {m["name"]: m for m in gold_json("spaced.json")}[name]
    want = gold_npz("spaced.npz")[name]
    g, file, rec_offs = spaced_inputs(meta, oracle.text2bin)
    rows = oracle.spaced_round(g.tobytes(), meta["mask"], meta["R"], file, rec_offs, meta["max_trial"],
                               meta["overlap_min"], buggy=True, nthreads=8)
    cols = meta["columns"]
    for ci, col in enumerate(cols):
        if col in ("dir", "ref_pos", "cost", "matlen_a", "matlen_b"):
            sel = want[:, cols.index("found")] == 1
            assert (rows[col][sel] == want[sel, ci]).all(), (name, col)
        else:
            assert (rows[col] == want[:, ci]).all(), (name, col)
    assert int(rows["found"].sum()) == meta["found"]


# ----------------------------------------------------------------------------- consensus (ref_seq, unlocked)
def test_consensus_golden(oracle):
    """ref_seq::try_align (elect, append, prepend) and evolve, two rounds per scenario: the oracle's restatement
    reproduces what the reference itself produced (tests/golden/consensus.json) -- every try's outcome, the vote
    boxes before and after evolve, the evolved text."""
    from cons_scenarios import SCENARIOS, run_scenario, scenario_inputs
    gold = {g["name"]: g for g in gold_json("consensus.json")}
    for sc in SCENARIOS:
        text, weight, reads = scenario_inputs(sc)
        got = run_scenario(oracle.consensus(text, weight), reads)
        want = gold[sc[0]]
        for k, (a, b) in enumerate(zip(got["rounds"], want["rounds"])):
            assert a["tries"] == b["tries"], (sc[0], k)
            assert a["before_evolve"] == b["before_evolve"], (sc[0], k)
            assert a["after_evolve"] == b["after_evolve"], (sc[0], k)
        assert sum(t[4] for r in want["rounds"] for t in r["tries"]) >= 12


def test_votebox_golden(oracle):
    """The hand-built vote-box states (tests/votebox_inputs.py) as the reference itself elected and evolved them, twice in a
    row (tests/golden/votebox.json: every state the reference is defined on): extent, vote boxes and text of the oracle at
    every stage."""
    import votebox_inputs as vb
    gold = gold_json("votebox.json")["states"]
    assert set(gold) == {st.name for st in vb.all_states() if st.ref_safe}
    assert {st.name for st in vb.evolve_states()} <= set(gold)
    for st in vb.all_states():
        if st.name not in gold:
            continue
        c = vb.build(oracle.consensus, st)
        vb.elect_loop(c, st)
        assert vb.record(vb.stages(c, st)) == gold[st.name], st.name


def test_spaced_multi_golden(oracle):
    """spaced_seed's main loop for a locked reference (seed rotation, pool erasure, stop rule; spaced_seed.cpp:409-452):
    the oracle's locked rounds chained by the same loop reproduce the reference's chain."""
    from cons_scenarios import MULTI, multi_inputs, multi_rounds
    gold = gold_json("spaced_multi.json")
    text, file, rec_offs = multi_inputs()
    fn = lambda mask, pool: oracle.spaced_round(text, mask, MULTI["R"], file, rec_offs[pool], MULTI["max_trial"],
                                                MULTI["overlap_min"], buggy=True, nthreads=4)
    found_round, log, final = multi_rounds(fn, gold["masks"], rec_offs.size)
    assert log == gold["log"] and found_round == gold["found_round"]
    for r, (a, b) in enumerate(zip(final, gold["final"])):
        assert a[0] == b[0] and (not a[0] or a == b), r
    assert sum(1 for x in found_round if x) > 100 and len({x for x in found_round}) >= 5


def test_assemble_golden(oracle):
    """spaced_seed's main loop WITHOUT -l (unlocked rounds: votes and growth inside a round, evolve after it, seed
    rotation, pool erasure) recorded from the reference's own ref_seq (tests/golden/assemble.json): the oracle's
    orc_cons_round / evolve chain reproduces every round -- reads found and their rows, probe and pair counts, extent,
    vote boxes, evolved text -- and the final assembly."""
    from cons_scenarios import assemble_inputs, run_assembly
    gold = gold_json("assemble.json")
    text, weight, file, rec_offs, texts = assemble_inputs()
    got = run_assembly(oracle.consensus(text, weight), gold["masks"], file, rec_offs, len(texts))
    assert len(got["rounds"]) == len(gold["rounds"])
    for a, b in zip(got["rounds"], gold["rounds"]):
        assert a == b, a["round"]
    assert got["final_text"] == gold["final_text"]
    assert len(gold["final_text"]) > 4 * len(text) and sum(len(r["found"]) for r in gold["rounds"]) > 150
    assert any(r["extent"][0] < 0 for r in gold["rounds"]) and any(r["extent"][1] > r["extent"][2] for r in gold["rounds"])


def test_spaced_seed_cli_golden(oracle):
    """The reference's own `spaced_seed` main, unmodified (tests/golden/spaced_seed_cli.json: -f ref_file, a one-line
    seed file, its t_aligner and OVERLAP_MIN, no -l): the consensus it prints after every round and the `found` lines
    of its log are what the oracle's unlocked rounds produce."""
    import hashlib
    from cons_scenarios import ASSEMBLE, SPACED_SEED_CLI, assemble_inputs, run_assembly
    gold = gold_json("spaced_seed_cli.json")["runs"]
    text, _, file, rec_offs, texts = assemble_inputs()
    mask = oracle.mask_from_pattern(SPACED_SEED_CLI["pattern"])
    for name, R, mt, mr in (("unlocked", 0.3, 32, 5), ("unlocked_r20", 0.2, 20, 3)):
        cfg = dict(ASSEMBLE, R=R, max_trial=mt, max_round=mr)
        rec = run_assembly(oracle.consensus(text, 1), [mask], file, rec_offs, len(texts), cfg)
        g = gold[name]
        printed = [r for r in rec["rounds"] if r["found"]]                    # a round without a match ends the loop unprinted
        assert [r["ref_len"] for r in printed] == g["consensus_len"], name
        assert [r["text_sha"] for r in printed] == g["consensus_sha"], name
        assert [[f[0], f[4], f[5], f[6]] for r in rec["rounds"] for f in r["found"]] == g["found"], name
        assert hashlib.sha256(g["last_consensus"].encode()).hexdigest()[:32] == g["consensus_sha"][-1]
    assert len(gold["unlocked"]["found"]) > 100 and gold["unlocked"]["consensus_len"][-1] > 3 * len(text)


def test_locator_cli_golden(oracle):
    """The stdout of the reference's own `locator` main, unmodified (tests/golden/locator_cli.json: contig file, pattern,
    reads on stdin, R = 0.15, its seq_aligner<40000,6000>): the oracle's locator driver prints the same rows."""
    from cons_scenarios import LOCATOR_CLI, locator_cli_inputs
    gold = gold_json("locator_cli.json")
    contig, texts = locator_cli_inputs()
    reads = np.frombuffer(b"".join(texts), np.uint8)
    offs = np.cumsum([0] + [len(t) for t in texts]).astype(np.uint64)
    rows, st = oracle.locator(np.frombuffer(contig, np.uint8), oracle.mask_from_pattern(LOCATOR_CLI["pattern"]), 0.15, reads, offs,
                              50, 500, maxn=40000, maxm=6000, nthreads=4)
    got = [[int(r["nseq"]), int(r["pos"]), int(r["cost"]), int(r["seglen"])] for r in rows if r["found"]]
    assert got == gold["rows"] and len(got) > 250
