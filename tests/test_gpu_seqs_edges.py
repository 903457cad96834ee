"""Every resident maker of a sequence set -- pba_seqs_from_text, _from_device_text, _from_records, _from_device_packed,
pba_seqs_revcomp -- on the reads that sit on every edge of the layout (tests/seqs_edge_inputs.py): the same 18 reads through
each of them give the counts, lengths, bytes, offsets, texts and bit planes that the layout kind promises (the
host arithmetic alone is held to numpy in tests/test_seq_layout_cpu.py, a stream's slots to these sets in
tests/test_gpu_map_stream.py).  All comparisons are exact.  Needs a real MI355X (-m gpu)."""
import numpy as np
import pytest

from map_stream_inputs import R
from pacbioassembly_amd import engine as eng
from pacbioassembly_amd.engine import PBA_KERNEL_BITVEC
from seqs_edge_inputs import EDGE_LENGTHS, host_packed, np_revcomp, self_pairs
from test_gpu_stream import export_bytes, random_reads

pytestmark = pytest.mark.gpu
ROTS = [0, 17, 8]            # the empty read first; 4 097 first; 31 first and 17 last


def on_device(a):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()
    torch.cuda.synchronize()                  # (the engine runs on its own stream)
    return d


def text_offsets(texts):
    """where the text layout puts every sequence, and where it ends"""
    pk = [((len(t) + 3) // 4 + 15) & ~15 for t in texts]
    return np.concatenate([[0], np.cumsum(pk)]).astype(np.uint64) if texts else np.zeros(1, np.uint64)


def check_set(ctx, S, texts, packed_bytes, want_bytes, want_offs, ref, ref_ids, base):
    """S holds `texts`: the figures, the exported bytes and offsets, every text, and -- the planes -- every read against the
    read ref_ids[i] of the text set `ref`, whose rows against itself are `base`"""
    assert S.count == len(texts) and S.max_len == max((len(t) for t in texts), default=0) and not S.non_acgt
    assert S.lengths().tolist() == [len(t) for t in texts] and S.packed_bytes == packed_bytes
    got, offs, lens = export_bytes(S)
    assert offs.tolist() == [int(o) for o in want_offs] and lens.tolist() == [len(t) for t in texts]
    assert got.shape == want_bytes.shape and (got == want_bytes).all()
    assert [S.get_text(i) for i in range(len(texts))] == texts
    pairs = self_pairs(texts)
    pairs["b_seq"] = [ref_ids[i] for i in pairs["a_seq"]]
    res = ctx.align_batch(S, ref, pairs, R, kernel=PBA_KERNEL_BITVEC)
    assert (res["cost"] == 0).all() and (res["rc"] == pairs["b_len"]).all()
    assert len(res) == len(base) and (res == base).all()


@pytest.mark.parametrize("rot", ROTS)
def test_every_maker_on_the_edge_reads(ctx, rot):
    lengths = EDGE_LENGTHS[rot:] + EDGE_LENGTHS[:rot]
    reads = random_reads(lengths, 900 + rot)
    n, ids = len(reads), list(range(len(reads)))
    assert n == 18 and (rot != 0 or lengths[0] == 0) and (rot != 17 or lengths[0] == 4097) and (rot != 8 or (lengths[0], lengths[-1]) == (31, 17))
    offs = text_offsets(reads)
    sets = []

    # the text set: pba_seqs_from_text; what every other set is held against
    T = ctx.seqs_from_list(reads, strict_acgt=True)
    sets.append(T)
    base = ctx.align_batch(T, T, self_pairs(reads), R, kernel=PBA_KERNEL_BITVEC)
    t_bytes = host_packed(reads, offs[:-1])
    assert len(t_bytes) == int(offs[-1])
    check_set(ctx, T, reads, int(offs[-1]), t_bytes, offs[:-1], T, ids, base)

    # pba_seqs_from_device_text
    text, toff = eng.concat(reads)
    d_text, d_toff = on_device(text), on_device(toff.astype(np.int64))
    D = ctx.seqs_from_device_text(d_text.data_ptr(), d_toff.data_ptr(), n, text.size, max(lengths))
    sets.append(D)
    check_set(ctx, D, reads, int(offs[-1]), t_bytes, offs[:-1], T, ids, base)

    # pba_seqs_from_records: the file is the arena, the empty read is dropped
    recs = [eng.text2bin(t) for t in reads]
    file = b"".join(recs)
    starts = np.concatenate([[0], np.cumsum([len(r) for r in recs])])[:-1]
    kept_ids = [i for i in ids if lengths[i] > 0]
    kept = [reads[i] for i in kept_ids]
    payload = (starts[kept_ids] + 4).astype(np.uint64)
    f_bytes = np.frombuffer(file, np.uint8)
    assert len(kept) == 17
    Rec = ctx.seqs_from_records(file, 0, 1 << 30)
    sets.append(Rec)
    check_set(ctx, Rec, kept, len(file), f_bytes, payload, T, kept_ids, base)

    # pba_seqs_from_device_packed: the export of the text set, and the record image with its payload offsets
    d_exp = on_device(t_bytes)
    P1 = ctx.seqs_from_device_packed(d_exp.data_ptr(), len(t_bytes), offs[:-1], np.array(lengths, np.uint32))
    sets.append(P1)
    check_set(ctx, P1, reads, len(t_bytes), t_bytes, offs[:-1], T, ids, base)
    d_file = on_device(f_bytes)
    P2 = ctx.seqs_from_device_packed(d_file.data_ptr(), len(file), payload, np.array([len(t) for t in kept], np.uint32))
    sets.append(P2)
    check_set(ctx, P2, kept, len(file), f_bytes, payload, T, kept_ids, base)

    # pba_seqs_revcomp: every sequence (no flip, all-ones flip), every other one
    flipped = [np_revcomp(t) for t in reads]
    mixed = [flipped[i] if i & 1 else reads[i] for i in ids]
    exported = {}
    for name, texts, flip in (("all", flipped, None), ("ones", flipped, np.ones(n, np.uint8)), ("alternating", mixed, np.arange(n) & 1)):
        want = ctx.seqs_from_list(texts, strict_acgt=True)
        want_base = ctx.align_batch(want, want, self_pairs(texts), R, kernel=PBA_KERNEL_BITVEC)
        Q = ctx.seqs_revcomp(T, flip)
        sets += [want, Q]
        check_set(ctx, Q, texts, int(offs[-1]), host_packed(texts, offs[:-1]), offs[:-1], want, ids, want_base)
        exported[name] = export_bytes(Q)[0]
    for i in ids:                                          # an alternating flip: forward bytes at even indices, revcomp bytes at odd
        lo, hi = int(offs[i]), int(offs[i + 1])
        src = exported["all"] if i & 1 else t_bytes
        assert (exported["alternating"][lo:hi] == src[lo:hi]).all(), i
    assert (exported["ones"] == exported["all"]).all()
    for S in sets:
        S.close()


@pytest.mark.parametrize("reads", [[], [b"", b"", b""]], ids=["no reads", "only empty reads"])
def test_sets_without_a_base_build_and_hold_zero_bytes(ctx, reads):
    T = ctx.seqs_from_list(reads, strict_acgt=True)
    Q = ctx.seqs_revcomp(T)
    for S in (T, Q):
        assert S.count == len(reads) and S.max_len == 0 and S.packed_bytes == 0 and not S.non_acgt
        assert S.lengths().tolist() == [0] * len(reads)
        got, offs, _ = export_bytes(S)
        assert got.size == 0 and offs.tolist() == [0] * len(reads)
        assert [S.get_text(i) for i in range(len(reads))] == reads
    T.close(); Q.close()
