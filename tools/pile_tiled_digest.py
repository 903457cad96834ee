#!/usr/bin/env python3
"""Digest of a pile-up evolved with votes on a set just above the long-segment threshold (the 70 001-base contig of
tests/polish_helpers.py: edge_case, votes on the first and last box of a tile, next to short segments).  Run it once with the
product and once with PBA_LIB_PATH=<a tools/build_variant.py build with -DPBA_PILE_LONG_SEG=1000000>, which keeps the
per-target kernels: the two lines must be equal -- the tiled kernels give byte for byte what the per-target ones give."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
from map_ref import rand_text
from polish_helpers import R, edge_case
from pacbioassembly_amd import Context, Pileup, engine as eng

ctx = Context(0)
T, reads = edge_case(711)
rng = np.random.default_rng(5)
texts = [rand_text(rng, 4097), T, b"", rand_text(rng, 1), rand_text(rng, 4096)]
S = ctx.seqs_from_list(texts, strict_acgt=True)
Rd = ctx.seqs_from_list(reads, strict_acgt=True)
ix = ctx.index_build_set(S, eng.mask_from_pattern("111*11*11*1*1111"))
rows, _ = ctx.map_reads(ix, S, Rd, R, strands=1)
pile = Pileup(ctx, S)
_, n_voted = pile.vote_mapped(Rd, rows, R)
boxes = hashlib.sha256(b"".join(x.tobytes() for x in pile.dump(1))).hexdigest()[:16]
out, crows = pile.evolve()
text = hashlib.sha256(b"\n".join(out.get_text(i) for i in range(out.count))).hexdigest()[:16]
print("pile_tiled_digest voted", n_voted, "len_out", crows["len_out"].tolist(), "boxes", boxes, "text", text)
