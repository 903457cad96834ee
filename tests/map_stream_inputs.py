"""Inputs of the streamed-mapping tests (pba_map_stream), built from seeds so that their composition can be judged on the CPU
from tests/map_ref.py alone (tests/test_map_stream_cpu.py) before the GPU test relies on it (tests/test_gpu_map_stream.py).

world(): 4 contigs -- 5 kb, 3 kb, 12 bases and an empty one -- and 150 reads of 500 - 1 400 bases at 15 % error drawn across
the two real contigs, about half of them reverse-complemented; every 10th read comes from another genome, every 15th is
100 - 400 bases long, below min_len = 500.
"""
import numpy as np

from map_ref import mutate, rand_text, rc

WORLD_SEED = 4901
CONTIG_LENS = [5000, 3000, 12, 0]
N_READS, ERR, R, TRIALS, MIN_LEN = 150, 0.15, 0.30, 50, 500
BATCH_SIZES = [37, 1, 0, 64, 5, 43]


def world(seed: int = WORLD_SEED):
    """(contigs, reads, flipped)"""
    rng = np.random.default_rng(seed)
    contigs = [rand_text(rng, n) for n in CONTIG_LENS]
    other = rand_text(rng, 6000)
    real = [c for c, n in enumerate(CONTIG_LENS) if n >= MIN_LEN]
    w = np.array([CONTIG_LENS[c] for c in real], float)
    reads = []
    for i in range(N_READS):
        T = other if i % 10 == 4 else contigs[real[int(rng.choice(len(real), p=w / w.sum()))]]
        L = int(rng.integers(100, 401)) if i % 15 == 7 else int(rng.integers(500, 1401))
        span = L + L // 5 + 20                                  # mutated, then cut: the read has exactly L bases
        s = int(rng.integers(0, len(T) - span + 1))
        reads.append(mutate(rng, T[s:s + span], ERR)[:L])
        assert len(reads[-1]) == L
    flipped = rng.integers(0, 2, N_READS).astype(bool)
    reads = [rc(x) if f else x for x, f in zip(reads, flipped)]
    return contigs, reads, flipped


def composition(rows, n_second_walk: int, reads):
    """What the world is for, as conditions on pba_map_row rows (the reference's or the engine's)."""
    found = rows[rows["found"] == 1]
    lens = np.array([len(x) for x in reads])
    return {
        "plus": int((found["strand"] == 1).sum()) >= 30,
        "minus": int((found["strand"] == -1).sum()) >= 30,
        "nowhere": int(((rows["found"] == 0) & (lens >= MIN_LEN)).sum()) >= 10,
        "short": int((rows["nseq"] < 0).sum()) >= 5 and int((lens < MIN_LEN).sum()) == int((rows["nseq"] < 0).sum()),
        "contigs": sorted(set(found["contig"].tolist())) == [c for c, n in enumerate(CONTIG_LENS) if n >= MIN_LEN],
        "second_walk": n_second_walk > 0,
    }


def batches_of(reads, sizes=BATCH_SIZES):
    out, at = [], 0
    for n in sizes:
        out.append(reads[at:at + n]); at += n
    assert at == len(reads)
    return out


def rows_tsv(rows) -> bytes:
    """What examples/map_stream_gpu.cpp prints: one line per read."""
    cols = ("read", "nseq", "found", "strand", "contig", "j", "pos", "cost", "seglen", "matlen_a", "matlen_b", "diag_cost", "n_pairs",
            "r_beg", "r_end", "c_beg", "c_end")
    return b"".join(("\t".join(str(int(r[c])) for c in cols) + "\n").encode() for r in rows)
