"""The per-base evidence rule of include/pba.h (pba_qual) restated in plain numpy: the expectation
pba_qual_phred, pba_pileup_evolve_qual, pba_qual_summary, pba_qual_low_spans and pba_seqs_write_fastq are held to, shared by
tests/test_qual_cpu.py and tests/test_gpu_qual.py.  Nothing here calls the library.

A fresh pile-up has sel = weight on the target's own base, sup = 0, tot = 1.  Box i yields the selection's character if
2 * max4(sel) > tot and then the suppliment's if 2 * max4(sup) > tot; each carries agree (the max4 it was elected from),
depth = min(tot - 1, 65535), src = i (| SUP for the suppliment's) and qv = phred(agree, N, qmax) with N = tot - 1 + weight."""
import numpy as np

SUP = 0x80000000
QMAX = 60
D = (1000, 1258, 1584, 1995, 2511, 3162, 3981, 5011, 6309, 7943)          # floor(1000 * 10^(r / 10))
S = tuple(D[q % 10] * 10 ** (q // 10) for q in range(QMAX + 1))

ROW_DTYPE = np.dtype([(n, "<i4") for n in ("seq", "len", "n_sel", "n_sup", "n_unvoted", "n_below", "n_low_runs", "min_qv",
                                           "max_depth", "pad")] + [("sum_qv", "<u8"), ("sum_depth", "<u8")])
SPAN_DTYPE = np.dtype([(n, "<i4") for n in ("seq", "beg", "end", "min_qv")])


def phred(agree: int, n: int, qmax: int = QMAX) -> int:
    """The largest q in [0, qmax] with (max(n - agree, 0) + 1) * S[q] <= (n + 2) * 1000, in Python integers; -1 for a qmax
    outside [0, 60]."""
    if qmax < 0 or qmax > QMAX:
        return -1
    against = max(int(n) - int(agree), 0)
    return max(q for q in range(qmax + 1) if q == 0 or (against + 1) * S[q] <= (int(n) + 2) * 1000)


def phred_array(agree, n, qmax: int = QMAX) -> np.ndarray:
    """phred over arrays (u64 products: below 2^63 for n < 2^31 + 65 535).  S rises with q, so the answer is the number of
    q in [1, qmax] that hold."""
    agree = np.asarray(agree, np.uint64)
    n = np.asarray(n, np.uint64)
    lhs = np.where(n > agree, n - agree, np.uint64(0)) + np.uint64(1)
    rhs = (n + np.uint64(2)) * np.uint64(1000)
    out = np.zeros(agree.shape, np.uint8)
    for q in range(1, qmax + 1):
        out += lhs * np.uint64(S[q]) <= rhs
    return out


def threshold_n(q: int, against: int = 0) -> int:
    """The smallest N >= against at which `against` dissenting observations still reach q."""
    return max(-(-(against + 1) * S[q] // 1000) - 2, against, 0)


def phred_grid():
    """(agree, n) pairs on the rule's edges: for every q in 0..60 and 0 / 1 / 3 / 20 dissenting observations the exact threshold
    pair and the pairs one below and one above it; agree > N; N = 2^31 + 65 534; the worked values of the header."""
    pairs = [(1, 1), (20, 20), (15, 20), (8, 8), (7, 7), (9, 5), (5, 5), (65535, 65535), (0, 0), (0, 1), (7, 0), (65535, 1),
             (65535, 2 ** 31 + 65534), (0, 2 ** 31 + 65534), (2 ** 31, 2 ** 31 + 65534), (2 ** 32 - 1, 5), (2 ** 32 - 1, 2 ** 31 + 65534)]
    for q in range(QMAX + 1):
        for against in (0, 1, 3, 20):
            n0 = threshold_n(q, against)
            for n in (n0 - 1, n0, n0 + 1):
                if n >= against and n - against < 2 ** 32:
                    pairs.append((n - against, n))
    a = np.array([p[0] for p in pairs], np.uint32)
    n = np.array([p[1] for p in pairs], np.uint64)
    return a, n


def evidence(sel, sup, tot, weight: int, qmax: int = QMAX) -> dict:
    """What evolve makes of one target's dump (sel[n, 4], sup[n, 4], tot[n]): {"text", "qv", "depth", "agree", "src"}, one
    entry per emitted character, the selection's before the suppliment's."""
    sel = np.asarray(sel).astype(np.int64).reshape(-1, 4)
    sup = np.asarray(sup).astype(np.int64).reshape(-1, 4)
    tot = np.asarray(tot).astype(np.int64)
    n = len(tot)
    keep = np.stack([2 * sel.max(axis=1) > tot, 2 * sup.max(axis=1) > tot], axis=1)          # V, S: a tie does not win
    agree = np.stack([sel.max(axis=1), sup.max(axis=1)], axis=1)
    base = np.stack([sel.argmax(axis=1), sup.argmax(axis=1)], axis=1)                         # the first of equal counters: A, C, G, T
    pos = np.arange(n, dtype=np.int64)
    src = np.stack([pos, pos | SUP], axis=1)
    depth = np.repeat(np.minimum(tot - 1, 65535)[:, None], 2, axis=1)
    big_n = np.repeat((tot - 1 + weight)[:, None], 2, axis=1)
    m = keep.reshape(-1)
    agree, base, src, depth, big_n = (x.reshape(-1)[m] for x in (agree, base, src, depth, big_n))
    return {"text": bytes(b"ACGT"[k] for k in base), "qv": phred_array(agree, big_n, qmax), "depth": depth.astype(np.uint16),
            "agree": agree.astype(np.uint16), "src": src.astype(np.uint32)}


def _runs(low):
    """[beg, end) of every maximal run of True."""
    x = np.concatenate([[False], np.asarray(low, bool), [False]]).astype(np.int8)
    d = np.diff(x)
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def summary(lengths, qv, depth, src, qmin: int) -> np.ndarray:
    """One row per sequence over back-to-back arrays."""
    rows = np.zeros(len(lengths), ROW_DTYPE)
    at = 0
    for s, ln in enumerate(int(x) for x in lengths):
        q, d, sc = (np.asarray(a[at:at + ln]).astype(np.int64) for a in (qv, depth, src))
        at += ln
        r = rows[s]
        r["seq"], r["len"] = s, ln
        r["n_sup"] = int((sc >= SUP).sum()); r["n_sel"] = ln - int(r["n_sup"])
        r["n_unvoted"] = int((d == 0).sum()); r["n_below"] = int((q < qmin).sum()); r["n_low_runs"] = len(_runs(q < qmin))
        r["min_qv"] = int(q.min()) if ln else -1
        r["max_depth"] = int(d.max()) if ln else 0
        r["sum_qv"], r["sum_depth"] = int(q.sum()), int(d.sum())
    return rows


def low_spans(lengths, qv, qmin: int, min_run: int = 1) -> np.ndarray:
    """The maximal runs of qv < qmin inside one sequence of at least min_run bases, with their smallest qv, by (seq, beg)."""
    out = []
    at = 0
    for s, ln in enumerate(int(x) for x in lengths):
        q = np.asarray(qv[at:at + ln]).astype(np.int64)
        at += ln
        for b, e in _runs(q < qmin):
            if e - b >= min_run:
                out.append((s, b, e, int(q[b:e].min())))
    return np.array(out, SPAN_DTYPE) if out else np.zeros(0, SPAN_DTYPE)


def fastq_image(texts, quals, names=None, first_id: int = 0) -> bytes:
    """'@' name '\\n' bases '\\n' "+\\n" quals '\\n' per record; the decimal id (first_id on) where no names are given."""
    out = []
    for k, (t, q) in enumerate(zip(texts, quals)):
        name = str(first_id + k).encode() if names is None else (names[k] if isinstance(names[k], bytes) else str(names[k]).encode())
        out.append(b"@" + name + b"\n" + t + b"\n+\n" + bytes(int(x) + 33 for x in q) + b"\n")
    return b"".join(out)
